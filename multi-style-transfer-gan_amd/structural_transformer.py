"""``structural_transformer`` module named by the reference (enhanced_generator.py:4) -- BUILD-DEFINED, parity unpinned.

The reference snapshot does not contain this file: there is no source, no trained weight and no test for
``StructuralTransformerBlock``; only its call shape is known -- ctor kwarg ``dim``; ``block(x, style, orig_input)`` with tokens
(N, HW/16, dim), style vector (N, dim), the input image (N,3,H,W); returns tokens of x's shape (enhanced_generator.py:115,
218-225).  Every caller of the reference builds ``num_transformer_blocks=1`` (enhanced_train.py:18-19, advanced_transform.py:29,
batch_process_images.py:95, direct_transform.py:35), so the block has to exist, construct and train; what it computes is this
build's definition (restated for the CPU in oracle/restatement.py::structural_transformer_block, which is what the tests compare
against).  A ``.pth`` written by the reference with such a block carries ``transformer_blocks.0.*`` keys of unknown names and
shapes: it cannot load into this (or any) re-implementation strictly.

Definition -- a pre-norm transformer block whose first norm is modulated by the style vector and whose input carries a
structure signal taken from the image itself:

    s   = structure_map(orig_input)            (N, L, 4): per 4x4-pixel cell mean R, G, B and mean |dx|+|dy| of the luminance
    h   = x + struct_proj(s)                                                          Linear(4 -> dim)
    g,b = style_mod(style).chunk(2)                                                   Linear(dim -> 2 dim), zero-initialised
    u   = LayerNorm(h; norm1) * (1 + g) + b                                           (style modulation; identity at init)
    h   = h + proj(softmax(q k^T / sqrt(d)) v),  q,k,v = qkv(u) split into heads      full attention over all L tokens
    out = h + fc2(GELU(fc1(LayerNorm(h; norm2))))                                     MLP ratio 2

Everything runs on the HIP kernels: the Linear layers as 1x1 convolutions over the token grid (implicit-GEMM, with their weight
gradients), LayerNorm + modulation, GELU and the structure map as fused element-wise kernels, attention as a flash-style fp32
MFMA kernel that never materialises the L x L matrix (L = 4096 at 256x256, 65536 at 1024x1024).  ``structure_map`` is treated
as a constant of the input image (no gradient flows into ``orig_input`` through it).  ``block.attention_precision = "mixed"``
(default ``"fp32"``; ``EnhancedGenerator.set_attention_precision``) runs the attention, forward and backward, on the 16-bit MFMA
kernels of csrc/flash_f16_train.hip with fp32 accumulation, softmax and results; head widths 16, 32 and 64.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from mstg_hip import ops
from mstg_hip.ops import ACT_GELU


class StructuralTransformerBlock(nn.Module):
    is_identity = False
    # "fp32" (default) or "mixed": the attention's kernels (ops.flash_attention).  A plain attribute read in forward: not a
    # constructor argument, not in the state_dict; EnhancedGenerator.set_attention_precision sets it on every block.
    attention_precision = "fp32"

    def __init__(self, dim, num_heads=4, mlp_ratio=2):
        super().__init__()
        if dim % (4 * num_heads) or dim // num_heads not in (8, 16, 32, 64):
            raise ValueError(f"StructuralTransformerBlock: dim={dim} with {num_heads} heads needs a head width of 8, 16, 32 or 64")
        self.dim, self.num_heads = dim, num_heads
        self.struct_proj = nn.Linear(4, dim)
        self.style_mod = nn.Linear(dim, 2 * dim)
        self.norm1 = nn.LayerNorm(dim)
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)
        self.norm2 = nn.LayerNorm(dim)
        self.fc1 = nn.Linear(dim, mlp_ratio * dim)
        self.fc2 = nn.Linear(mlp_ratio * dim, dim)
        nn.init.zeros_(self.style_mod.weight)  # no modulation until trained
        nn.init.zeros_(self.style_mod.bias)

    def forward(self, x, style, orig_input):
        ops.check_attention_precision(self.attention_precision, self.dim // self.num_heads)
        if x.dim() != 3 or x.shape[-1] != self.dim:
            raise RuntimeError(f"StructuralTransformerBlock(dim={self.dim}) got tokens of shape {tuple(x.shape)}")
        N, L, dim = x.shape
        if style is None or style.shape != (N, dim):
            raise RuntimeError(f"StructuralTransformerBlock: style must be ({N}, {dim})")
        if orig_input.dim() != 4 or (orig_input.shape[2] // 4) * (orig_input.shape[3] // 4) != L:
            raise RuntimeError("StructuralTransformerBlock: the token count must be (H/4) * (W/4) of the input image")
        s = ops.structure_map(orig_input).reshape(N, L, 4)
        # Linear(4 -> dim): the 1x1-conv kernels want the input channels padded to a multiple of 4 -- they are
        h = ops.add(x, ops.linear_tokens(s, self.struct_proj.weight, self.struct_proj.bias))
        mod = ops.linear_tokens(style, self.style_mod.weight, self.style_mod.bias)   # (N, 2 dim)
        g, b = mod[:, :dim].contiguous(), mod[:, dim:].contiguous()
        u = ops.layer_norm_mod(h, self.norm1.weight, self.norm1.bias, g, b, self.norm1.eps)
        qkv = ops.linear_tokens(u, self.qkv.weight, self.qkv.bias)
        a = ops.flash_attention(qkv, self.num_heads, self.attention_precision)
        h = ops.add(h, ops.linear_tokens(a, self.proj.weight, self.proj.bias))
        v = ops.layer_norm_mod(h, self.norm2.weight, self.norm2.bias, None, None, self.norm2.eps)
        m = ops.activation(ops.linear_tokens(v, self.fc1.weight, self.fc1.bias), ACT_GELU)  # GELU' needs the pre-activation
        return ops.add(h, ops.linear_tokens(m, self.fc2.weight, self.fc2.bias))
