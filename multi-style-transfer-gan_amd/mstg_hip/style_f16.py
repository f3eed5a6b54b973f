"""Mixed-precision multi-style loss: fp16 VGG features and Gram matrices in the forward, bf16 gradients in the backward
(csrc/style_f16.hip, ``style_loss.MultiStyleGramLoss(..., precision="mixed")``).

The gradients of this loss are 1e-7 and below and shrink with 1 / (C H W), so fp16 gradients would need a loss scale; bf16 has
fp32's exponent range and needs none: no scale, no skipped steps, no state.  The forward keeps fp16 (three more mantissa bits),
because the loss is a difference of Gram matrices.  Accumulation is fp32 everywhere, the loss value and ``dL/dy`` are fp32, and
autograd never sees a 16-bit tensor: the whole loss is ONE ``autograd.Function``.

This module holds the packed layers (re-packed when a weight changes: the stamp ``ops.py`` uses for its filter packs), the stage
functions (one C-ABI call each) and the loss function.  The weights are frozen: there is no weight gradient.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import LOSS_MSE, STYLE16_BF16, STYLE16_F16, Style16ConvDesc

MAX_CHANNELS = 512  # csrc/style_f16.hip
PRECISIONS = ("fp32", "mixed")
# launches of one loss forward + backward on the VGG16 topology (10 convolutions, 3 pools, 4 taps), filter packs aside:
#   forward : 10 conv + 3 pool + 4 x (Gram slabs + reduce) + 4 x (MSE partials + final) + 1 sum = 30
#   backward: 4 MSE gradient + 4 x (symmetrise + Gram backward) + 10 input gradients + 3 pool   = 25
LAUNCHES_FWD, LAUNCHES_BWD = 30, 25


def check_precision(precision) -> str:
    if precision not in PRECISIONS:
        raise ValueError(f"style loss precision must be one of {PRECISIONS}, got {precision!r}")
    return precision


def check_channels(channels) -> None:
    """Raise for layer widths the 16-bit kernels do not serve (needs no GPU)."""
    for c in channels:
        if c < 16 or c % 16 or c > MAX_CHANNELS:
            raise RuntimeError(f"mstg_hip mixed-precision style loss: every layer width must be a multiple of 16 up to {MAX_CHANNELS}, "
                               f"got {c} (widths {tuple(channels)}); precision=\"fp32\" serves other widths")


def check_image(shape) -> None:
    if len(shape) != 4 or shape[1] != 3:
        raise RuntimeError(f"mstg_hip mixed-precision style loss expects (N,3,H,W), got {tuple(shape)}")
    if shape[2] % 8 or shape[3] % 8 or shape[2] < 8 or shape[3] < 8:
        raise RuntimeError(f"mstg_hip mixed-precision style loss: H and W must be multiples of 8 (three 2x2 max-pools), got "
                           f"{shape[2]}x{shape[3]}")


def conv_desc(dtype, N, H, W, Cin, Cout, stem=0, image_grad=0, flip=0, relu=0) -> Style16ConvDesc:
    return Style16ConvDesc(dtype, N, H, W, Cin, Cout, stem, image_grad, flip, relu)


def kernel_name(d: Style16ConvDesc) -> str:
    """The kernel variant a launch of ``d`` takes (the library's one routing function; needs no GPU)."""
    name = _lib.load().mstg_style16_conv_kernel_name(C.byref(d))
    if name is None:
        raise RuntimeError("mstg_hip style conv: " + _lib.load().mstg_last_error().decode())
    return name.decode()


def _args():
    from .ops import _p, _stream, _timed, _ws
    return _p, _stream, _timed, _ws


def _ws(nbytes, device):
    from . import ops
    return ops._ws(nbytes, device)  # looked up per call: the memory-contract guard of the tests replaces it


_TORCH_DTYPE = {STYLE16_F16: torch.float16, STYLE16_BF16: torch.bfloat16}


class PackedStyleConv:
    """One 3x3 stride-1 pad-1 convolution with its filter packed for ``style_conv16_kernel``.  ``flip``: ``weight`` is the
    (Cin, Cout, 3, 3) filter of the layer whose INPUT gradient this convolution computes."""

    def __init__(self, dtype, weight, bias=None, relu=0, stem=0, image_grad=0, flip=0):
        if weight.device.type != "cuda":
            raise RuntimeError("mstg_hip mixed-precision style loss: move the feature stack to the GPU first (no CPU path)")
        self.dtype, self.relu, self.stem, self.image_grad, self.flip = dtype, relu, stem, image_grad, flip
        self.Cout, self.Cin = (int(weight.shape[1]), int(weight.shape[0])) if flip else (int(weight.shape[0]), int(weight.shape[1]))
        lib = _lib.load()
        d = self.desc(1, 8, 8)  # the packed layout depends on the layer, not on N / H / W
        nbytes = lib.mstg_style16_conv_plan_bytes(C.byref(d))
        if nbytes == 0:
            raise RuntimeError(f"mstg_hip style conv: unsupported layer ({self.Cin}->{self.Cout}): " + lib.mstg_last_error().decode())
        self.blob = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
        self.repack(weight, bias)

    def desc(self, N, H, W) -> Style16ConvDesc:
        return conv_desc(self.dtype, N, H, W, self.Cin, self.Cout, self.stem, self.image_grad, self.flip, self.relu)

    def repack(self, weight, bias):
        _p, _stream, _, _ = _args()
        keep = [weight.detach().float().contiguous(), None if bias is None else bias.detach().float().contiguous()]
        d = self.desc(1, 8, 8)
        _lib.check(_lib.load().mstg_style16_conv_pack(C.byref(d), _p(keep[0]), _p(keep[1]), _p(self.blob), self.blob.numel(),
                                                      _stream()), "mstg_style16_conv_pack")
        self._keep = keep  # the pack kernel reads them asynchronously

    def __call__(self, x, mask=None):
        """x: NHWC (N,H,W,Cin) of the layer's 16-bit dtype, or the (N,3,H,W) fp32 image for the stem.  mask (nullable): fp16 NHWC of
        the destination's shape.  Returns NHWC of the dtype, or the (N,3,H,W) fp32 image gradient."""
        _p, _stream, _timed, _ = _args()
        want = torch.float32 if self.stem else _TORCH_DTYPE[self.dtype]
        if not x.is_cuda or not x.is_contiguous() or x.dtype != want or x.dim() != 4:
            raise RuntimeError(f"mstg_hip style conv: x must be a contiguous 4-d GPU tensor of {want}, got {tuple(x.shape)} {x.dtype}")
        N, Cin, H, W = x.shape if self.stem else (x.shape[0], x.shape[3], x.shape[1], x.shape[2])
        if Cin != self.Cin:
            raise RuntimeError(f"mstg_hip style conv: expected {self.Cin} channels, got {tuple(x.shape)}")
        d = self.desc(N, H, W)
        if self.image_grad:
            y = torch.empty((N, self.Cout, H, W), dtype=torch.float32, device=x.device)
        else:
            y = torch.empty((N, H, W, self.Cout), dtype=_TORCH_DTYPE[self.dtype], device=x.device)
        if mask is not None and (mask.dtype != torch.float16 or mask.shape != y.shape or not mask.is_contiguous()):
            raise RuntimeError("mstg_hip style conv: the ReLU mask is the fp16 NHWC activation of the destination's shape")
        flops = 2.0 * N * H * W * self.Cin * self.Cout * 9
        nbytes = x.numel() * x.element_size() + y.numel() * y.element_size()
        _timed("style_conv16_kernel", flops, nbytes, lambda: _lib.check(
            _lib.load().mstg_style16_conv_fwd(C.byref(d), _p(self.blob), _p(x), _p(mask), _p(y), _stream()), "mstg_style16_conv_fwd"),
            f"{'bf16' if self.dtype else 'f16'} N{N} {H}x{W} {self.Cin}->{self.Cout}")
        return y


# ---- stage functions -------------------------------------------------------------------------------------------------------------
def _nhwc(t, dtype, name):
    if not t.is_cuda or t.dtype != dtype or t.dim() != 4 or not t.is_contiguous():
        raise RuntimeError(f"mstg_hip style loss: {name} must be a contiguous NHWC GPU tensor of {dtype}, got {tuple(t.shape)} {t.dtype}")
    return t


def maxpool_fwd(x):
    """F.max_pool2d(x, 2) on fp16 NHWC -> (values fp16, arg-max slot bytes)."""
    _p, _stream, _, _ = _args()
    N, H, W, Cn = _nhwc(x, torch.float16, "pool input").shape
    y = torch.empty((N, H // 2, W // 2, Cn), dtype=torch.float16, device=x.device)
    idx = torch.empty((N, H // 2, W // 2, Cn), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().mstg_style16_maxpool_fwd(_p(x), _p(y), _p(idx), N, H, W, Cn, _stream()), "mstg_style16_maxpool_fwd")
    return y, idx


def maxpool_bwd(dy, idx, mask=None):
    """dy bf16 (N,H/2,W/2,C) routed through idx -> bf16 (N,H,W,C); mask: the fp16 pre-pool feature (zero where it is not > 0)."""
    _p, _stream, _, _ = _args()
    N, Ho, Wo, Cn = _nhwc(dy, torch.bfloat16, "pool grad_output").shape
    if idx.shape != dy.shape or idx.dtype != torch.uint8:
        raise RuntimeError("mstg_hip style loss: arg-max bytes do not match the pooled gradient")
    dx = torch.empty((N, 2 * Ho, 2 * Wo, Cn), dtype=torch.bfloat16, device=dy.device)
    if mask is not None and _nhwc(mask, torch.float16, "pool mask").shape != dx.shape:
        raise RuntimeError("mstg_hip style loss: the pool mask is the pre-pool feature")
    _lib.check(_lib.load().mstg_style16_maxpool_bwd(_p(dy), _p(idx), _p(mask), _p(dx), N, 2 * Ho, 2 * Wo, Cn, _stream()),
               "mstg_style16_maxpool_bwd")
    return dx


def gram_fwd(f):
    """G[n] = F[n]^T F[n] / (C H W): fp16 NHWC (N,H,W,C) -> fp32 (N,C,C)."""
    _p, _stream, _timed, _ = _args()
    lib = _lib.load()
    N, H, W, Cn = _nhwc(f, torch.float16, "gram input").shape
    g = torch.empty((N, Cn, Cn), dtype=torch.float32, device=f.device)
    nws = lib.mstg_style16_gram_workspace_bytes(N, H * W, Cn)
    if nws == 0:
        raise RuntimeError("mstg_style16_gram_fwd: " + lib.mstg_last_error().decode())
    ws = _ws(nws, f.device)
    _timed("style16_gram_fwd_kernel", 2.0 * N * H * W * Cn * Cn, 2.0 * N * H * W * Cn + 4.0 * N * Cn * Cn, lambda: _lib.check(
        lib.mstg_style16_gram_fwd(_p(f), _p(g), N, H * W, Cn, 1.0 / (Cn * H * W), _p(ws), ws.numel() * 4, _stream()), "mstg_style16_gram_fwd"))
    return g


def gram_bwd(f, dg, incoming=None):
    """[F > 0] * (F (dG + dG^T) / (C H W) + incoming), rounded once to bf16: the gradient in front of the tap's ReLU."""
    _p, _stream, _timed, _ = _args()
    lib = _lib.load()
    N, H, W, Cn = _nhwc(f, torch.float16, "gram input").shape
    if dg.dtype != torch.float32 or tuple(dg.shape) != (N, Cn, Cn) or not dg.is_contiguous():
        raise RuntimeError("mstg_hip style loss: dG must be contiguous fp32 (N,C,C)")
    if incoming is not None and _nhwc(incoming, torch.bfloat16, "incoming gradient").shape != f.shape:
        raise RuntimeError("mstg_hip style loss: the incoming gradient must have the feature's shape")
    df = torch.empty((N, H, W, Cn), dtype=torch.bfloat16, device=f.device)
    nws = lib.mstg_style16_gram_bwd_workspace_bytes(N, Cn)
    if nws == 0:
        raise RuntimeError("mstg_style16_gram_bwd: " + lib.mstg_last_error().decode())
    ws = _ws(nws, f.device)
    _timed("style16_gram_bwd_kernel", 2.0 * N * H * W * Cn * Cn, 4.0 * N * H * W * Cn, lambda: _lib.check(
        lib.mstg_style16_gram_bwd(_p(f), _p(dg), _p(incoming), _p(df), N, H * W, Cn, 1.0 / (Cn * H * W), _p(ws), ws.numel() * 4,
                                  _stream()), "mstg_style16_gram_bwd"))
    return df


# ---- the packed stack ------------------------------------------------------------------------------------------------------------
class StyleF16Layers:
    """fp16 forward packs and bf16 input-gradient packs of a ``VGGFeatures`` stack, re-packed when ``load_state_dict``, an in-place
    write, a move or a raw-pointer writer that bumps ``ops.PACK_EPOCH`` changes a weight."""

    def __init__(self, features):
        self.features = features
        self.convs = [getattr(features, f"conv{i}") for i in features.plan if i != "M"]
        check_channels([c.weight.shape[0] for c in self.convs])
        self.fwd, self.bwd, self.stamps = [None] * len(self.convs), [None] * len(self.convs), [None] * len(self.convs)

    def refresh(self):
        from .ops import _pack_stamp, _pack_storages
        for i, conv in enumerate(self.convs):
            stamp = _pack_stamp((conv.weight, conv.bias))
            if self.stamps[i] is not None and self.stamps[i][0] == stamp:
                continue
            first = i == 0
            if self.fwd[i] is None or self.fwd[i].blob.device != conv.weight.device:
                self.fwd[i] = PackedStyleConv(STYLE16_F16, conv.weight, conv.bias, relu=1, stem=int(first))
                self.bwd[i] = PackedStyleConv(STYLE16_BF16, conv.weight, None, image_grad=int(first), flip=1)
            else:
                self.fwd[i].repack(conv.weight, conv.bias)
                self.bwd[i].repack(conv.weight, None)
            self.stamps[i] = (stamp, _pack_storages((conv.weight, conv.bias)))
        return self

    def forward(self, y, keep=False):
        """y: (N,3,H,W) fp32 on the GPU -> the four fp16 NHWC tap features; ``keep``: also everything the backward reads, as
        (taps, acts, pools): acts[i] = ReLU output of convolution i, pools = [(pooled fp16, arg-max bytes)]."""
        check_image(y.shape)
        if not y.is_cuda:
            raise RuntimeError("mstg_hip: input must live on the GPU (this package has no CPU path)")
        if y.dtype != torch.float32:
            raise RuntimeError(f"mstg_hip mixed-precision style loss: the image must be float32, got {y.dtype}")
        self.refresh()
        from style_loss import VGG_TAPS
        h = y.contiguous()
        taps, acts, pools = [], [], []
        for item in self.features.plan:
            if item == "M":
                h, idx = maxpool_fwd(h)
                pools.append((h, idx))
                continue
            h = self.fwd[item](h)
            acts.append(h)
            if item in VGG_TAPS:
                taps.append(h)
        return (taps, acts, pools) if keep else taps

    def backward(self, acts, pools, dgs):
        """dL/dy (N,3,H,W) fp32 from the fp32 Gram gradients ``dgs`` (one per tap): bf16 between the kernels."""
        from style_loss import VGG_TAPS
        plan = self.features.plan
        tap_of = {ci: t for t, ci in enumerate(VGG_TAPS)}
        g, npool = None, len(pools)  # g: the gradient at the point the walk has reached
        for pos in range(len(plan) - 1, -1, -1):
            item = plan[pos]
            if item == "M":
                npool -= 1
                before = plan[pos - 1]  # a pool always follows a convolution
                # a tapped feature gets its ReLU mask in the Gram backward (which adds this gradient); any other one here
                g = maxpool_bwd(g, pools[npool][1], None if before in tap_of else acts[before])
                continue
            if item in tap_of:
                g = gram_bwd(acts[item], dgs[tap_of[item]], g)  # now the gradient in front of this layer's ReLU
            elif g is None:
                raise RuntimeError("mstg_hip style loss: the stack must end in a tapped layer")
            if item == 0:
                return self.bwd[0](g)
            src = plan[pos - 1]  # the layer's input: a convolution's ReLU output (masked here) or a pooled feature (no ReLU of its own)
            g = self.bwd[item](g, None if src == "M" else acts[src])
        raise RuntimeError("mstg_hip style loss: empty feature stack")


class MixedStyleLossFn(torch.autograd.Function):
    """sum_taps MSE(G(F(y)), target): fp32 (N,3,H,W) in, fp32 scalar out, fp32 dL/dy back."""

    @staticmethod
    def forward(ctx, y, layers, targets):
        _p, _stream, _, _ = _args()
        lib = _lib.load()
        taps, acts, pools = layers.forward(y, keep=True)
        grams = [gram_fwd(f) for f in taps]
        terms = torch.empty(len(taps), dtype=torch.float32, device=y.device)
        for l, (g, t) in enumerate(zip(grams, targets)):
            if t.shape != g.shape:
                raise RuntimeError(f"mstg_hip style loss: target {tuple(t.shape)} does not match the Gram matrix {tuple(g.shape)}")
            ws = _ws(lib.mstg_loss_workspace_bytes(g.numel()), y.device)
            _lib.check(lib.mstg_loss_mean_fwd(_p(g), _p(t), 0.0, g.numel(), LOSS_MSE, terms.data_ptr() + 4 * l, _p(ws), ws.numel() * 4,
                                              _stream()), "mstg_loss_mean_fwd")
        out = torch.empty(1, dtype=torch.float32, device=y.device)
        ptrs = (C.c_void_p * len(taps))(*[terms.data_ptr() + 4 * l for l in range(len(taps))])
        wts = (C.c_float * len(taps))(*([1.0] * len(taps)))
        _lib.check(lib.mstg_weighted_sum_fwd(ptrs, wts, len(taps), 1, _p(out), _stream()), "mstg_weighted_sum_fwd")
        ctx.layers, ctx.kept = layers, (acts, pools, grams, targets, terms)
        return out.reshape(())

    @staticmethod
    def backward(ctx, gout):
        _p, _stream, _, _ = _args()
        lib = _lib.load()
        acts, pools, grams, targets, _ = ctx.kept
        gout = gout.float().contiguous().reshape(1)
        dgs = []
        for g, t in zip(grams, targets):
            dg = torch.empty((g.shape[0], g.shape[1], g.shape[2]), dtype=torch.float32, device=g.device)
            _lib.check(lib.mstg_loss_mean_bwd(_p(g), _p(t), 0.0, g.numel(), LOSS_MSE, _p(gout), 1.0, _p(dg), None, _stream()),
                       "mstg_loss_mean_bwd")
            dgs.append(dg)
        return ctx.layers.backward(acts, pools, dgs), None, None
