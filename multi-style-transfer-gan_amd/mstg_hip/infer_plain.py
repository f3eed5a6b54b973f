"""Inference-only forward of the plain CycleGAN ``Generator`` in fp16 storage / fp16 MFMA / fp32 accumulation, BatchNorm folded.

What ``batch_process_images.py:210-211`` runs under ``torch.no_grad()`` for its ``cyclegan`` mode is ``Generator.forward``
(batch_process_images.py:20-58 == pretrain.py:60-97) in eval mode.  There ``nn.BatchNorm2d`` is a per-channel scale and shift known
before the launch, so every norm (and the activation behind it) goes into the epilogue of the convolution in front of it and the
forward is eight launches of ``plain_conv_f16_kernel`` (csrc/infer_f16_plain.hip): activations NHWC fp16 between them, the fp32
NCHW image read by the stem, the fp16 NCHW image written by the head.

The filters are packed once (inference: weights are frozen); ``Generator.half_inference()`` builds a ``HalfPlainGeneratorPlan``
and re-builds it after a ``load_state_dict``.  Widths: ``channels`` a multiple of 8 up to 64 (layer widths up to 512).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import ACT_LEAKY02, ACT_NONE, ACT_RELU, ACT_TANH, F16PlainDesc

MAX_LAYER_CHANNELS = 512  # csrc/infer_f16_plain.hip

TAP_NAMES = ("encoder.0", "encoder.2", "encoder.5", "encoder.8", "decoder.0", "decoder.3", "decoder.6")


def check_width(channels: int) -> None:
    """Raise for a ``Generator(channels)`` no fp16 kernel serves (needs no GPU)."""
    if channels < 8 or channels % 8 or channels * 8 > MAX_LAYER_CHANNELS:
        raise RuntimeError(f"mstg_hip fp16 inference of the plain Generator is built for channels a multiple of 8 up to 64 "
                           f"(layer widths up to {MAX_LAYER_CHANNELS}; 64 is what every caller of the reference builds), got "
                           f"channels={channels}; the fp32 forward serves other widths")


def fold_batchnorm(conv_bias, gamma, beta, running_mean, running_var, eps):
    """Eval-mode ``BatchNorm2d(conv(x) + conv_bias)`` as ``conv_nobias(x) * scale + shift`` per output channel, in fp32:
    ``scale = gamma * rsqrt(running_var + eps)``, ``shift = beta + (conv_bias - running_mean) * scale``."""
    scale = gamma.detach().float() * torch.rsqrt(running_var.detach().float() + eps)
    bias = torch.zeros_like(scale) if conv_bias is None else conv_bias.detach().float()
    shift = beta.detach().float() + (bias - running_mean.detach().float()) * scale
    return scale, shift


def plain_desc(kind, N, H, W, Cin, Cout, K=4, src_nchw_f32=0, dst_nchw=0, act=ACT_NONE) -> F16PlainDesc:
    Ho, Wo = (2 * H, 2 * W) if kind == 1 else (H // 2, W // 2)
    return F16PlainDesc(kind, N, H, W, Cin, Ho, Wo, Cout, K, src_nchw_f32, dst_nchw, act)


class PackedPlainConv:
    """One ``nn.Conv2d(k4,s2,p1)`` (kind 0) or ``nn.ConvTranspose2d(k4,s2,p1)`` (kind 1) with its filter packed for the fp16
    kernel and the epilogue ``act(acc * scale + shift)``; ``scale`` / ``shift``: fp32 per output channel (None: 1 / 0)."""

    def __init__(self, kind, weight, scale, shift, act=ACT_NONE, src_nchw_f32=0, dst_nchw=0):
        if weight.device.type != "cuda":
            raise RuntimeError("mstg_hip fp16 inference: move the generator to the GPU first (no CPU path)")
        self.kind, self.act, self.src_nchw_f32, self.dst_nchw = kind, act, src_nchw_f32, dst_nchw
        self.Cin, self.Cout = (weight.shape[0], weight.shape[1]) if kind == 1 else (weight.shape[1], weight.shape[0])
        self.K = weight.shape[2]
        lib = _lib.load()
        d = self.desc(1, 16, 16)  # the packed layout depends on the layer, not on N / H / W
        nbytes = lib.mstg_f16_plain_plan_bytes(C.byref(d))
        if nbytes == 0:
            raise RuntimeError(f"mstg_hip fp16 inference: unsupported layer (kind {kind}, {self.Cin}->{self.Cout}, k{self.K}): "
                               + lib.mstg_last_error().decode())
        self.blob = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
        self.repack(weight, scale, shift)

    def repack(self, weight, scale, shift):
        """Pack again from tensors of the shapes the layer was built with (training: once per optimizer step)."""
        from .ops import _p, _stream
        dev = self.blob.device
        keep = [weight.detach().float().contiguous()]
        keep += [None if t is None else t.detach().float().contiguous().to(dev) for t in (scale, shift)]
        d = self.desc(1, 16, 16)
        _lib.check(_lib.load().mstg_f16_plain_pack(C.byref(d), _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(self.blob),
                                                   self.blob.numel(), _stream()), "mstg_f16_plain_pack")
        self._keep = keep  # the pack kernel reads them asynchronously

    def desc(self, N, H, W) -> F16PlainDesc:
        return plain_desc(self.kind, N, H, W, self.Cin, self.Cout, self.K, self.src_nchw_f32, self.dst_nchw, self.act)

    def __call__(self, x):
        """x: NHWC fp16 (N,H,W,Cin), or the NCHW fp32 image for the stem -> NHWC fp16, or the NCHW fp16 image for the head."""
        from .ops import _p, _stream, _timed
        if not x.is_cuda or not x.is_contiguous():
            raise RuntimeError("mstg_hip fp16 conv: x must be a contiguous GPU tensor")
        if self.src_nchw_f32:
            N, Cin, H, W = x.shape
            want = torch.float32
        else:
            N, H, W, Cin = x.shape
            want = torch.float16
        if Cin != self.Cin or x.dtype != want:
            raise RuntimeError(f"mstg_hip fp16 conv: expected {self.Cin} channels of {want}, got {tuple(x.shape)} {x.dtype}")
        d = self.desc(N, H, W)
        shape = (N, self.Cout, d.Ho, d.Wo) if self.dst_nchw else (N, d.Ho, d.Wo, self.Cout)
        y = torch.empty(shape, dtype=torch.float16, device=x.device)
        flops = 2.0 * N * d.Ho * d.Wo * self.Cin * self.Cout * (4 if self.kind == 1 else 16)
        nbytes = x.numel() * x.element_size() + y.numel() * 2
        _timed("plain_conv_f16_kernel", flops, nbytes, lambda: _lib.check(
            _lib.load().mstg_f16_plain_fwd(C.byref(d), _p(self.blob), _p(x), _p(y), _stream()), "mstg_f16_plain_fwd"),
            f"k{self.kind} N{N} {H}x{W} {self.Cin}->{self.Cout}")
        return y


class HalfPlainGeneratorPlan:
    """Packed fp16 copy of a plain ``Generator``'s weights with its BatchNorms folded + the eight-launch inference forward."""

    def __init__(self, gen):
        e, d = gen.encoder, gen.decoder
        check_width(e[0].out_channels)
        if e[0].weight.device.type != "cuda":
            raise RuntimeError("mstg_hip fp16 inference: move the generator to the GPU first (no CPU path)")

        def folded(conv, bn):
            return fold_batchnorm(conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)

        self.layers = [PackedPlainConv(0, e[0].weight, None, e[0].bias, ACT_LEAKY02, src_nchw_f32=1)]
        for ci, bi in ((2, 3), (5, 6), (8, 9)):
            self.layers.append(PackedPlainConv(0, e[ci].weight, *folded(e[ci], e[bi]), ACT_LEAKY02))
        for ci, bi in ((0, 1), (3, 4), (6, 7)):
            self.layers.append(PackedPlainConv(1, d[ci].weight, *folded(d[ci], d[bi]), ACT_RELU))
        self.head = PackedPlainConv(1, d[9].weight, None, d[9].bias, ACT_TANH, dst_nchw=1)
        self.head_pre = PackedPlainConv(1, d[9].weight, None, d[9].bias, ACT_NONE, dst_nchw=1)  # parity taps only

    @torch.no_grad()
    def forward(self, x, taps=None):
        """x: (N,3,H,W) fp32 in [-1,1] on the GPU, H and W multiples of 16 -> (N,3,H,W) fp16.  ``taps`` (dict) receives the seven
        intermediate activations (NHWC fp16, keyed by the convolution's state_dict prefix) and ``pre_tanh`` (NCHW fp16)."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"Generator expects (N,3,H,W), got {tuple(x.shape)}")
        if x.shape[2] % 16 or x.shape[3] % 16:
            raise RuntimeError(f"Generator: H and W must be multiples of 16 (four stride-2 stages), got {x.shape[2]}x{x.shape[3]}")
        if not x.is_cuda:
            raise RuntimeError("mstg_hip: input must live on the GPU (this package has no CPU path)")
        h = x.float().contiguous()
        for name, layer in zip(TAP_NAMES, self.layers):
            h = layer(h)
            if taps is not None:
                taps[name] = h
        if taps is not None:
            taps["pre_tanh"] = self.head_pre(h)
        return self.head(h)
