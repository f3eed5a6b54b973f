"""Mixed-precision training step of the plain CycleGAN ``Generator``: fp16 storage / fp16 MFMA / fp32 accumulation, no autograd.

What the reference's pre-training loop runs under ``torch.cuda.amp.autocast()`` (pretrain.py:159-166 on the layers of
pretrain.py:60-97), as an explicit forward / backward plan in the style of ``HalfPlainGeneratorPlan``:

  forward    eight ``plain_conv_f16_kernel`` launches (csrc/infer_f16_plain.hip); the six convolutions in front of a BatchNorm
             store ``z = conv(x) + bias`` as NHWC fp16 and ``mstg_f16_train_bn_fwd`` normalises it with BATCH statistics
             (fp32, two-pass), applies the activation and updates the running statistics; stem (LeakyReLU) and head (tanh,
             NCHW fp16) run as in inference.
  loss       masked L1 mean in fp32 on the fp16 image, fused with the gradient that enters the chain (L1 sign, mask, tanh
             backward, loss scale), ``mstg_f16_train_head_loss_bwd``.
  backward   per layer: BatchNorm + activation backward on fp16 (``mstg_f16_train_bn_bwd``, mask recomputed from ``z``), the
             weight gradient on ``wgrad_f16_kernel`` (csrc/train_f16_plain.hip), and the input gradient as a
             ``plain_conv_f16_kernel`` launch on the OPPOSITE-kind pack of the same weight: the input gradient of
             ``Conv2d(k4,s2,p1)`` with weight (O,I,4,4) is ``ConvTranspose2d(k4,s2,p1)`` of that tensor read as (Cin=O, Cout=I,4,4),
             and the other way round.  The head's gradient has 3 channels: it is written NHWC padded to 8 and the head's
             input-gradient pack is built from the weight padded to (C,8,4,4) with zeros.

Parameters stay the module's fp32 tensors; gradients are written unscaled, in fp32, into the ``p.grad`` views of
``FlatAdam.grad``.  The six convolution biases in front of a BatchNorm get exact zeros (the norm removes them).
The loss scale lives on the device (``fstate`` = {scale, 1 / scale}; ``istate`` = {skipped steps, good steps, last step ok}).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._lib import ACT_LEAKY02, ACT_NONE, ACT_RELU, ACT_TANH
from .infer_plain import PackedPlainConv, check_width

BN_LAYERS = (("encoder", 2, 3, 0, ACT_LEAKY02), ("encoder", 5, 6, 0, ACT_LEAKY02), ("encoder", 8, 9, 0, ACT_LEAKY02),
             ("decoder", 0, 1, 1, ACT_RELU), ("decoder", 3, 4, 1, ACT_RELU), ("decoder", 6, 7, 1, ACT_RELU))


def auto_loss_scale(numel: int) -> float:
    """2 ** ceil(log2(numel)): the per-element gradient of a mean over ``numel`` elements, 1 / numel, lands in [0.5, 1]."""
    if numel < 1:
        raise ValueError(f"loss scale: numel must be positive, got {numel}")
    return float(2 ** (int(numel) - 1).bit_length())


def check_loss_scale(value) -> float:
    """A loss scale given as a number must be a positive power of two, so that unscaling is exact."""
    v = float(value)
    if not (v > 0.0 and math.isfinite(v) and math.frexp(v)[0] == 0.5):
        raise ValueError(f"loss_scale must be 'auto' or a positive power of two, got {value!r}")
    return v


def check_generator(gen) -> int:
    """Raise for a ``Generator`` the fp16 training kernels do not serve (needs no GPU); returns ``channels``."""
    channels = gen.encoder[0].out_channels
    try:
        check_width(channels)
    except RuntimeError:
        raise RuntimeError(f"mstg_hip mixed-precision training of the plain Generator is built for channels a multiple of 8 up "
                           f"to 64, got channels={channels}; train other widths with amp=False") from None
    return channels


def _args():
    from .ops import _p, _stream, _timed
    return _p, _stream, _timed


def make_state(loss_scale: float, device):
    """(fstate, istate) of a step: {scale, 1 / scale} fp32 and {skipped steps, good steps, last step ok} int32, on the device."""
    fstate = torch.tensor([loss_scale, 1.0 / loss_scale], dtype=torch.float32, device=device)
    istate = torch.zeros(3, dtype=torch.int32, device=device)
    return fstate, istate


def _f16(t, name):
    if not t.is_cuda or t.dtype != torch.float16 or not t.is_contiguous():
        raise RuntimeError(f"mstg_hip fp16 training: {name} must be a contiguous fp16 GPU tensor")
    return t


def bn_workspace(C_, device):
    nbytes = _lib.load().mstg_f16_train_bn_workspace_bytes(1 << 20, C_)
    if nbytes == 0:
        raise RuntimeError("mstg_hip fp16 training: " + _lib.load().mstg_last_error().decode())
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def image_nhwc8(x):
    """(N,3,H,W) fp32 -> (N,H,W,8) fp16, channels 3..7 zero."""
    _p, _stream, _timed = _args()
    N, _, H, W = x.shape
    out = torch.empty((N, H, W, 8), dtype=torch.float16, device=x.device)
    _timed("train_img_nhwc8_kernel", 0, x.numel() * 4 + out.numel() * 2, lambda: _lib.check(
        _lib.load().mstg_f16_train_image_nhwc8(_p(x), _p(out), N, H, W, _stream()), "mstg_f16_train_image_nhwc8"))
    return out


def bn_fwd(z, gamma, beta, running_mean, running_var, act, eps=1e-5, momentum=0.1, ws=None):
    """Training-mode BatchNorm2d + activation on NHWC fp16 ``z`` -> (y fp16, mean fp32 [C], rstd fp32 [C])."""
    _p, _stream, _timed = _args()
    _f16(z, "z")
    C_ = z.shape[-1]
    P = z.numel() // C_
    ws = bn_workspace(C_, z.device) if ws is None else ws
    y = torch.empty_like(z)
    mean = torch.empty(C_, dtype=torch.float32, device=z.device)
    rstd = torch.empty_like(mean)
    nb = z.numel() * 2
    _timed("train_bn_apply_kernel", 0, 0, lambda: _lib.check(_lib.load().mstg_f16_train_bn_fwd(
        _p(z), _p(gamma), _p(beta), P, C_, act, eps, momentum, _p(running_mean), _p(running_var), _p(mean), _p(rstd), _p(y),
        _p(ws), ws.numel() * 4, _stream()), "mstg_f16_train_bn_fwd"), f"P{P} C{C_}",
        split={"train_chan_partial_kernel": (5.0 * z.numel(), 2 * nb), "train_bn_apply_kernel": (4.0 * z.numel(), 2 * nb)})
    return y, mean, rstd


def bn_bwd(z, dy, gamma, beta, mean, rstd, act, fstate, dgamma, dbeta, ws=None):
    """Backward of ``bn_fwd``: dz fp16; dgamma / dbeta (fp32, times 1 / loss scale) are written into the given tensors."""
    _p, _stream, _timed = _args()
    _f16(z, "z"), _f16(dy, "dy")
    C_ = z.shape[-1]
    P = z.numel() // C_
    ws = bn_workspace(C_, z.device) if ws is None else ws
    dz = torch.empty_like(z)
    nb = z.numel() * 2
    _timed("train_bn_bwd_apply_kernel", 0, 0, lambda: _lib.check(_lib.load().mstg_f16_train_bn_bwd(
        _p(z), _p(dy), _p(gamma), _p(beta), _p(mean), _p(rstd), P, C_, act, _p(fstate), _p(dgamma), _p(dbeta), _p(dz),
        _p(ws), ws.numel() * 4, _stream()), "mstg_f16_train_bn_bwd"), f"P{P} C{C_}",
        split={"train_chan_partial_kernel": (8.0 * z.numel(), 2 * nb), "train_bn_bwd_apply_kernel": (10.0 * z.numel(), 3 * nb)})
    return dz


def act_bwd(a, da, act):
    """dz = da * act'(a) from the activation's output (ReLU / LeakyReLU(0.2)), fp16."""
    _p, _stream, _timed = _args()
    _f16(a, "a"), _f16(da, "da")
    dz = torch.empty_like(a)
    _timed("train_act_bwd_kernel", a.numel(), 6 * a.numel(), lambda: _lib.check(
        _lib.load().mstg_f16_train_act_bwd(_p(a), _p(da), _p(dz), a.numel(), act, _stream()), "mstg_f16_train_act_bwd"))
    return dz


def head_loss_bwd(y, real, mask, fstate):
    """y: fp16 (N,3,H,W) head image -> (loss: 0-dim fp32, unscaled; dz: (N,H,W,8) fp16 gradient at the head's pre-activation)."""
    _p, _stream, _timed = _args()
    _f16(y, "y")
    N, _, H, W = y.shape
    lib = _lib.load()
    ws = torch.empty(max(lib.mstg_f16_train_loss_workspace_bytes(N, H, W) // 4, 1), dtype=torch.float32, device=y.device)
    loss = torch.empty((), dtype=torch.float32, device=y.device)
    dz = torch.empty((N, H, W, 8), dtype=torch.float16, device=y.device)
    _timed("train_head_loss_bwd_kernel", 12.0 * y.numel(), y.numel() * 10 + dz.numel() * 2, lambda: _lib.check(
        lib.mstg_f16_train_head_loss_bwd(_p(y), _p(real), _p(mask), N, H, W, _p(fstate), _p(loss), _p(dz), _p(ws), ws.numel() * 4,
                                         _stream()), "mstg_f16_train_head_loss_bwd"))
    return loss, dz


def wgrad_workspace_bytes(N, h, w, Cs, Cb, CbOut) -> int:
    nbytes = _lib.load().mstg_f16_train_wgrad_workspace_bytes(N, h, w, Cs, Cb, CbOut)
    if nbytes == 0:
        raise RuntimeError("mstg_hip fp16 training: " + _lib.load().mstg_last_error().decode())
    return nbytes


def wgrad(S, B, CbOut, fstate, dW, ws=None):
    """dW (Cs, CbOut, 4, 4) fp32 = (1 / loss scale) * sum S[n,y,x,s] * B[n,2y+ky-1,2x+kx-1,b]; S (N,h,w,Cs), B (N,2h,2w,Cb) NHWC
    fp16.  Conv2d: S = dZ, B = X; ConvTranspose2d: S = X, B = dZ."""
    _p, _stream, _timed = _args()
    _f16(S, "S"), _f16(B, "B")
    N, h, w, Cs = S.shape
    Cb = B.shape[-1]
    if tuple(B.shape[:3]) != (N, 2 * h, 2 * w):
        raise RuntimeError(f"mstg_hip fp16 wgrad: the big map must be (N,2h,2w,Cb), got {tuple(B.shape)} for {tuple(S.shape)}")
    if dW.dtype != torch.float32 or not dW.is_contiguous() or dW.numel() != Cs * CbOut * 16:
        raise RuntimeError("mstg_hip fp16 wgrad: dW must be a contiguous fp32 tensor of Cs * CbOut * 16 elements")
    nbytes = wgrad_workspace_bytes(N, h, w, Cs, Cb, CbOut)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=S.device)
    flops = 2.0 * N * h * w * Cs * CbOut * 16
    _timed("wgrad_f16_kernel", flops, S.numel() * 2 + B.numel() * 2 + dW.numel() * 4, lambda: _lib.check(
        _lib.load().mstg_f16_train_wgrad(_p(S), _p(B), N, h, w, Cs, Cb, CbOut, _p(fstate), _p(dW), _p(ws), ws.numel() * 4,
                                         _stream()), "mstg_f16_train_wgrad"), f"N{N} {h}x{w} Cs{Cs} Cb{CbOut}")
    return dW


def bias_grad(dz, Cvalid, fstate, out, ws=None):
    """out[c] = (1 / loss scale) * sum over pixels of dz[..., c], c < Cvalid (stem and head bias gradients)."""
    _p, _stream, _timed = _args()
    _f16(dz, "dz")
    C_ = dz.shape[-1]
    P = dz.numel() // C_
    ws = bn_workspace(C_, dz.device) if ws is None else ws
    _timed("train_chan_partial_kernel", dz.numel(), dz.numel() * 2, lambda: _lib.check(
        _lib.load().mstg_f16_train_bias_grad(_p(dz), P, C_, Cvalid, _p(fstate), _p(out), _p(ws), ws.numel() * 4, _stream()),
        "mstg_f16_train_bias_grad"))
    return out


def scale_update(norm, fstate, istate):
    _p, _stream, _ = _args()
    _lib.check(_lib.load().mstg_f16_train_scale_update(_p(norm), _p(fstate), _p(istate), _stream()), "mstg_f16_train_scale_update")


def guarded_adam_step(opt, istate):
    """``FlatAdam.step`` that the device turns into a no-op when the step just checked by ``scale_update`` was not finite; the
    bias corrections use ``opt``'s step count plus the good steps counted on the device."""
    from . import ops
    _p, _stream, _ = _args()
    opt.check_views()
    g = opt.param_groups[0]
    ops.bump_pack_epoch()  # parameter memory is about to change behind torch's version counters
    _lib.check(_lib.load().mstg_f16_train_adam(_p(opt.flat), _p(opt.grad), _p(opt.exp_avg), _p(opt.exp_avg_sq), opt.flat.numel(),
                                               g["lr"], g["betas"][0], g["betas"][1], g["eps"], opt.step_base, _p(istate),
                                               _stream()), "mstg_f16_train_adam")


class PlainGeneratorTrainPlan:
    """fp16 packs (forward + input-gradient pack per layer) of a plain ``Generator`` and one forward / backward over them."""

    def __init__(self, gen):
        check_generator(gen)
        e, d = gen.encoder, gen.decoder
        if e[0].weight.device.type != "cuda":
            raise RuntimeError("mstg_hip fp16 training: move the generator to the GPU first (no CPU path)")
        self.gen = gen
        self.stem = PackedPlainConv(0, e[0].weight, None, e[0].bias, ACT_LEAKY02, src_nchw_f32=1)
        self.convs, self.dgrads = [], []
        for part, ci, bi, kind, act in BN_LAYERS:
            seq = getattr(gen, part)
            self.convs.append(PackedPlainConv(kind, seq[ci].weight, None, seq[ci].bias, ACT_NONE))
            self.dgrads.append(PackedPlainConv(1 - kind, seq[ci].weight, None, None, ACT_NONE))
        self.head = PackedPlainConv(1, d[9].weight, None, d[9].bias, ACT_TANH, dst_nchw=1)
        self.head_wpad = torch.zeros((d[9].weight.shape[0], 8, 4, 4), dtype=torch.float32, device=d[9].weight.device)
        self.head_wpad[:, :3].copy_(d[9].weight.detach())
        self.head_dgrad = PackedPlainConv(0, self.head_wpad, None, None, ACT_NONE)
        self.bn_ws = bn_workspace(512, e[0].weight.device)
        self.wg_ws = {}

    def repack(self):
        """After the optimizer has changed the weights: pack them again (fifteen small launches)."""
        e, d = self.gen.encoder, self.gen.decoder
        self.stem.repack(e[0].weight, None, e[0].bias)
        for (part, ci, bi, kind, act), conv, dg in zip(BN_LAYERS, self.convs, self.dgrads):
            m = getattr(self.gen, part)[ci]
            conv.repack(m.weight, None, m.bias)
            dg.repack(m.weight, None, None)
        self.head.repack(d[9].weight, None, d[9].bias)
        self.head_wpad[:, :3].copy_(d[9].weight.detach())
        self.head_dgrad.repack(self.head_wpad, None, None)

    def _wgrad_ws(self, N, H, W):
        key = (N, H, W)
        if key not in self.wg_ws:
            C_ = self.gen.encoder[0].out_channels
            need, h, w = 0, H // 2, W // 2
            need = max(need, wgrad_workspace_bytes(N, h, w, C_, 8, 3))  # stem and head
            widths = (C_, 2 * C_, 4 * C_, 8 * C_)
            for i in range(3):  # encoder.{2,5,8} and decoder.{6,3,0}: small map (h/2, w/2, widths[i+1]), big map (h, w, widths[i])
                h, w = h // 2, w // 2
                need = max(need, wgrad_workspace_bytes(N, h, w, widths[i + 1], widths[i], widths[i]))
            self.wg_ws = {key: torch.empty(need // 4, dtype=torch.float32, device=self.gen.encoder[0].weight.device)}
        return self.wg_ws[key]

    @torch.no_grad()
    def forward_backward(self, x, real, mask, fstate):
        """x, real, mask: (N,3,H,W) fp32 on the GPU.  Writes every ``p.grad`` (which must exist, fp32, contiguous: the views
        ``FlatAdam`` attaches) and the BatchNorm running statistics; returns the unscaled loss (0-dim fp32 device tensor)."""
        gen = self.gen
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"Generator expects (N,3,H,W), got {tuple(x.shape)}")
        N, _, H, W = x.shape
        if H % 16 or W % 16:
            raise RuntimeError(f"Generator: H and W must be multiples of 16 (four stride-2 stages), got {H}x{W}")
        if not x.is_cuda:
            raise RuntimeError("mstg_hip: input must live on the GPU (this package has no CPU path)")
        if real.shape != x.shape:
            raise RuntimeError(f"mstg_hip fp16 training: real image {tuple(real.shape)} does not match the input {tuple(x.shape)}")
        x = x.float().contiguous()
        real = real.float().contiguous()
        mask = mask.float().expand_as(x).contiguous()
        ws, wg_ws = self.bn_ws, self._wgrad_ws(N, H, W)
        e, d = gen.encoder, gen.decoder

        x8 = image_nhwc8(x)
        acts, zs, stats = [self.stem(x)], [], []
        for (part, ci, bi, kind, act), conv in zip(BN_LAYERS, self.convs):
            bn = getattr(gen, part)[bi]
            z = conv(acts[-1])
            y, mean, rstd = bn_fwd(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, act, bn.eps, bn.momentum, ws)
            bn.num_batches_tracked += 1
            zs.append(z)
            stats.append((mean, rstd))
            acts.append(y)
        img = self.head(acts[-1])
        loss, dz = head_loss_bwd(img, real, mask, fstate)

        wgrad(acts[-1], dz, 3, fstate, d[9].weight.grad, wg_ws)  # ConvTranspose2d: S = input, B = dZ
        bias_grad(dz, 3, fstate, d[9].bias.grad, ws)
        da = self.head_dgrad(dz)
        for i in range(len(BN_LAYERS) - 1, -1, -1):
            part, ci, bi, kind, act = BN_LAYERS[i]
            conv, bn = getattr(gen, part)[ci], getattr(gen, part)[bi]
            dz = bn_bwd(zs[i], da, bn.weight, bn.bias, stats[i][0], stats[i][1], act, fstate, bn.weight.grad, bn.bias.grad, ws)
            if kind == 1:
                wgrad(acts[i], dz, dz.shape[-1], fstate, conv.weight.grad, wg_ws)
            else:
                wgrad(dz, acts[i], acts[i].shape[-1], fstate, conv.weight.grad, wg_ws)
            conv.bias.grad.zero_()  # in front of a BatchNorm: the gradient is exactly zero
            da = self.dgrads[i](dz)
        dz = act_bwd(acts[0], da, ACT_LEAKY02)
        wgrad(dz, x8, 3, fstate, e[0].weight.grad, wg_ws)
        bias_grad(dz, dz.shape[-1], fstate, e[0].bias.grad, ws)
        return loss
