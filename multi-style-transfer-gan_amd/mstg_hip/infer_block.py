"""Inference-only fp16 forward of the ``StructuralTransformerBlock``s between down2 and up1 of ``EnhancedGenerator``
(``half_inference(fp16_blocks=True)``), on the kernels of csrc/infer_f16_block.hip.

The block (structural_transformer.py:55-74) runs on fp16 tokens with an fp32 residual stream: the first kernel of the first block
reads down2's fp16 output, the last kernel of the last block writes the fp16 NHWC tensor that up1 reads.  Per block:

    gb  = style_mod(style)                               fp32 linear_tokens, (N, 2 dim) = g | b
    h   = x + struct_proj(s);  u = LN(h) (1 + g) + b     mstg_f16_ln_mod_fwd       h fp32, u fp16
    qkv = qkv(u)                                          mstg_f16_linear_fwd       fp16
    a   = softmax(q k^T / sqrt(D)) v                      mstg_f16_flash_attn_fwd   fp16
    h   = h + proj(a)                                     mstg_f16_linear_fwd       fp32 (residual epilogue)
    v   = LN(h)                                           mstg_f16_ln_mod_fwd       fp16
    m   = GELU(fc1(v))                                    mstg_f16_linear_fwd       fp16 (GELU epilogue)
    out = h + fc2(m)                                      mstg_f16_linear_fwd       fp32, fp16 behind the last block

and once per forward the structure map (mstg_structure_map), the token mean of down2's output and the style encoder's
Linear + ReLU (enhanced_generator.py:144-146).  The filters are packed once per plan; ``EnhancedGenerator``'s load_state_dict hook
drops the plan, so the packed block weights follow a load_state_dict like every other layer's.  Served head widths: 16, 32, 64.
"""
from __future__ import annotations

import torch

from . import _lib, ops
from ._lib import ACT_GELU, ACT_NONE, ACT_RELU
from .ops import _p, _stream, _timed

HEAD_WIDTHS = (16, 32, 64)  # csrc/infer_f16_block.hip
BLOCK_DIMS = (64, 128, 256)


def check_block(block) -> None:
    """Raise for a StructuralTransformerBlock no fp16 kernel serves (needs no GPU)."""
    dim, heads = int(block.dim), int(block.num_heads)
    D = dim // heads
    if D * heads != dim or D not in HEAD_WIDTHS:
        raise RuntimeError(f"mstg_hip fp16 transformer block: head width {D} (dim={dim}, {heads} heads) is not served; the fp16 "
                           f"kernels serve head widths 16, 32 and 64 (channels 16, 32 or 64 with the default 4 heads); the fp32 "
                           f"blocks (fp16_blocks=False) serve it")
    if dim not in BLOCK_DIMS:
        raise RuntimeError(f"mstg_hip fp16 transformer block: dim={dim} is not served (64, 128 or 256)")


def _f32(t):
    return None if t is None else t.detach().float().contiguous()


class PackedLinear:
    """One nn.Linear over tokens with its filter packed for blk_linear_f16_kernel (fp16 filter, fp32 bias)."""

    def __init__(self, weight, bias):
        self.Cout, self.Cin = int(weight.shape[0]), int(weight.shape[1])
        lib = _lib.load()
        nbytes = lib.mstg_f16_linear_plan_bytes(self.Cin, self.Cout)
        if nbytes == 0:
            raise RuntimeError(f"mstg_hip fp16 token GEMM: unsupported layer {self.Cin}->{self.Cout}: " + lib.mstg_last_error().decode())
        if weight.device.type != "cuda":
            raise RuntimeError("mstg_hip fp16 inference: move the generator to the GPU first (no CPU path)")
        self._keep = (_f32(weight), _f32(bias))  # the pack kernel reads them asynchronously
        self.blob = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
        _lib.check(lib.mstg_f16_linear_pack(_p(self._keep[0]), _p(self._keep[1]), self.Cin, self.Cout, _p(self.blob), nbytes, _stream()),
                   "mstg_f16_linear_pack")

    def __call__(self, x, act=ACT_NONE, residual=None, out_f16=True):
        """x: fp16 (N, L, Cin) -> (N, L, Cout) fp16 (out_f16) or fp32; residual: fp32 (N, L, Cout) added behind the activation."""
        if x.dtype != torch.float16 or not x.is_cuda or not x.is_contiguous() or x.shape[-1] != self.Cin:
            raise RuntimeError(f"mstg_hip fp16 token GEMM: x must be contiguous fp16 (N, L, {self.Cin}) on the GPU, got {tuple(x.shape)} {x.dtype}")
        N, L = x.shape[0], x.shape[1]
        if residual is not None and (residual.dtype != torch.float32 or residual.shape != (N, L, self.Cout) or not residual.is_contiguous()):
            raise RuntimeError("mstg_hip fp16 token GEMM: the residual is a contiguous fp32 (N, L, Cout) tensor")
        y = torch.empty((N, L, self.Cout), dtype=torch.float16 if out_f16 else torch.float32, device=x.device)
        nbytes = x.numel() * 2 + y.numel() * y.element_size() + (0 if residual is None else residual.numel() * 4)
        _timed("blk_linear_f16_kernel", 2.0 * N * L * self.Cin * self.Cout, nbytes, lambda: _lib.check(
            _lib.load().mstg_f16_linear_fwd(_p(self.blob), _p(x), _p(residual), _p(y), N, L, self.Cin, self.Cout, act, int(out_f16),
                                            _stream()), "mstg_f16_linear_fwd"), f"N{N} L{L} {self.Cin}->{self.Cout}")
        return y


def ln_mod(x, gamma, beta, eps, gb=None, smap=None, sp_w=None, sp_b=None, want_h=False):
    """u = LN(h) * (1 + g) + b as fp16 (N, L, dim); h = x (fp16 or fp32), or x + struct_proj(smap) with ``smap`` (N, L, 4) fp32.
    Returns (u, h) with h fp32 when ``want_h`` (needs smap), else (u, None)."""
    N, L, dim = x.shape
    u = torch.empty((N, L, dim), dtype=torch.float16, device=x.device)
    h = torch.empty((N, L, dim), dtype=torch.float32, device=x.device) if want_h else None
    nbytes = x.numel() * x.element_size() + u.numel() * 2 + (0 if h is None else h.numel() * 4)
    _timed("blk_ln_mod_f16_kernel", 0, nbytes, lambda: _lib.check(_lib.load().mstg_f16_ln_mod_fwd(
        _p(x), int(x.dtype == torch.float16), _p(smap), _p(sp_w), _p(sp_b), _p(gamma), _p(beta), _p(gb), _p(h), _p(u), N, L, dim,
        float(eps), _stream()), "mstg_f16_ln_mod_fwd"))
    return u, h


def token_mean(x):
    """x: fp16 (N, L, dim) -> fp32 (N, dim), the mean over the tokens."""
    N, L, dim = x.shape
    lib = _lib.load()
    out = torch.empty((N, dim), dtype=torch.float32, device=x.device)
    wsb = lib.mstg_f16_token_mean_workspace_bytes(N, L, dim)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=x.device)
    _timed("blk_token_mean_partial_kernel", 0, x.numel() * 2, lambda: _lib.check(
        lib.mstg_f16_token_mean(_p(x), _p(out), N, L, dim, _p(ws), ws.numel(), _stream()), "mstg_f16_token_mean"))
    return out


def flash_attention(qkv, heads):
    """softmax(q k^T / sqrt(D)) v per head over all tokens of an image: qkv fp16 (N, L, 3 heads D) -> fp16 (N, L, heads D)."""
    if qkv.dtype != torch.float16 or not qkv.is_cuda or not qkv.is_contiguous():
        raise RuntimeError("mstg_hip fp16 flash attention: qkv must be a contiguous fp16 GPU tensor")
    N, L, C3 = qkv.shape
    dim = C3 // 3
    D = dim // heads
    if dim * 3 != C3 or D * heads != dim:
        raise RuntimeError(f"mstg_hip fp16 flash attention: {C3} channels do not split into q|k|v x {heads} heads")
    out = torch.empty((N, L, dim), dtype=torch.float16, device=qkv.device)
    _timed(f"blk_flash_f16_kernel<{D}>", 4.0 * N * heads * L * L * D, 2.0 * (qkv.numel() + out.numel()), lambda: _lib.check(
        _lib.load().mstg_f16_flash_attn_fwd(_p(qkv), _p(out), N, L, heads, D, _stream()), "mstg_f16_flash_attn_fwd"),
        f"N{N} L{L} heads{heads} D{D}")
    return out


class HalfBlock:
    """Packed fp16 copy of one StructuralTransformerBlock + its forward."""

    def __init__(self, block):
        check_block(block)
        if block.qkv.weight.device.type != "cuda":
            raise RuntimeError("mstg_hip fp16 inference: move the generator to the GPU first (no CPU path)")
        self.dim, self.heads = block.dim, block.num_heads
        self.sp_w, self.sp_b = _f32(block.struct_proj.weight), _f32(block.struct_proj.bias)   # (dim, 4), (dim,)
        self.sm_w, self.sm_b = block.style_mod.weight, block.style_mod.bias  # fp32 linear_tokens on N x dim values, as the fp32 block
        self.n1 = (_f32(block.norm1.weight), _f32(block.norm1.bias), block.norm1.eps)
        self.n2 = (_f32(block.norm2.weight), _f32(block.norm2.bias), block.norm2.eps)
        self.qkv = PackedLinear(block.qkv.weight, block.qkv.bias)
        self.proj = PackedLinear(block.proj.weight, block.proj.bias)
        self.fc1 = PackedLinear(block.fc1.weight, block.fc1.bias)
        self.fc2 = PackedLinear(block.fc2.weight, block.fc2.bias)

    def forward(self, x, smap, style, out_f16=True):
        """x: tokens (N, L, dim), fp16 or fp32; smap: (N, L, 4) fp32 structure map; style: (N, dim) fp32 -> (N, L, dim) fp16
        (out_f16) or fp32."""
        gb = ops.linear_tokens(style, self.sm_w, self.sm_b)             # (N, 2 dim): g | b
        u, h = ln_mod(x, self.n1[0], self.n1[1], self.n1[2], gb=gb, smap=smap, sp_w=self.sp_w, sp_b=self.sp_b, want_h=True)
        a = flash_attention(self.qkv(u), self.heads)
        h = self.proj(a, residual=h, out_f16=False)
        v, _ = ln_mod(h, self.n2[0], self.n2[1], self.n2[2])
        return self.fc2(self.fc1(v, act=ACT_GELU), residual=h, out_f16=out_f16)


class HalfBlocksPlan:
    """The chain of fp16 blocks between down2 and up1 (enhanced_generator.py:216-225)."""

    def __init__(self, gen, blocks):
        self.blocks = [HalfBlock(b) for b in blocks]
        lin = gen.style_encoder[2]
        self.style_w, self.style_b = lin.weight, lin.bias

    def forward(self, h, x):
        """h: down2's output, NHWC fp16 (N, H/4, W/4, dim); x: the (N, 3, H, W) fp32 image -> NHWC fp16 for up1."""
        N, H4, W4, dim = h.shape
        tokens = h.reshape(N, H4 * W4, dim)
        smap = ops.structure_map(x)                                           # (N, H/4, W/4, 4) == (N, L, 4)
        style = ops.linear_tokens(token_mean(tokens), self.style_w, self.style_b, act=ACT_RELU)
        for i, blk in enumerate(self.blocks):
            tokens = blk.forward(tokens, smap, style, out_f16=i == len(self.blocks) - 1)
        return tokens.reshape(N, H4, W4, dim)
