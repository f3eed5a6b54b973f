"""CPU statements of the mixed-precision training attention (csrc/flash_f16_train.hip; the contract in include/mstg_hip.h), torch
only, float64 wherever the contract names no rounding.

``yardstick``       softmax attention and its gradient in float64 on the fp16-rounded qkv
``emulate``         the contract with a rounding at each point it names: qh = fp16(qkv), qb = bf16(qkv), P -> fp16 for P v_h, out and lse
                    stored as fp32, dO_b = bf16(dO), bf16(P) for dV, delta = sum_keys P dP, dS = bf16(P (dP - delta)); every sum in float64
``block_emulated``  StructuralTransformerBlock.forward from the definition in structural_transformer.py's docstring in float64, with
                    either attention substituted (autograd runs the substituted backward)
"""
import math

import torch
import torch.nn.functional as F


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel_l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def r_f16(x):
    """float64 -> the fp32 value the device forms -> fp16 (round-to-nearest-even), back in float64"""
    return x.float().half().double()


def r_bf16(x):
    return x.float().bfloat16().double()


def r_f32(x):
    return x.float().double()


def heads_of(t, heads):
    """(N, L, heads D) -> (N, heads, L, D)"""
    N, L, dim = t.shape
    return t.reshape(N, L, heads, dim // heads).transpose(1, 2)


def tokens_of(t):
    """(N, heads, L, D) -> (N, L, heads D)"""
    N, h, L, D = t.shape
    return t.transpose(1, 2).reshape(N, L, h * D)


def thirds(dqkv):
    return dict(zip(("dq", "dk", "dv"), dqkv.chunk(3, dim=-1)))


def yardstick(qkv, gy, heads):
    """(out, lse, dqkv) in float64 of softmax(q k^T / sqrt(D)) v on the fp16-rounded qkv; lse (N, heads, L)."""
    t = qkv.half().double().requires_grad_(True)
    q, k, v = (heads_of(u, heads) for u in t.chunk(3, dim=-1))
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    y = tokens_of(torch.softmax(s, dim=-1) @ v)
    (g,) = torch.autograd.grad((y * gy.double()).sum(), [t])
    return y.detach(), torch.logsumexp(s.detach(), dim=-1), g


def emulate_fwd(qkv, heads):
    qh = qkv.float().half().double()
    q, k, v = (heads_of(u, heads) for u in qh.chunk(3, dim=-1))
    scale = 1.0 / math.sqrt(q.shape[-1])
    S = q @ k.transpose(-1, -2)
    m = S.max(dim=-1, keepdim=True).values
    p = torch.exp(scale * (S - m))
    l = p.sum(dim=-1, keepdim=True)
    out = r_f32((r_f16(p) @ v) / l)
    lse = r_f32(scale * m + torch.log(l))
    return tokens_of(out), lse.squeeze(-1), S


def emulate_bwd(qkv, lse, S, gy, heads):
    qb = qkv.float().bfloat16().double()
    qB, kB, vB = (heads_of(u, heads) for u in qb.chunk(3, dim=-1))
    scale = 1.0 / math.sqrt(qB.shape[-1])
    dOb = r_bf16(heads_of(gy.float().double(), heads))
    P = torch.exp(scale * S - lse.unsqueeze(-1))
    dV = r_bf16(P).transpose(-1, -2) @ dOb
    dP = dOb @ vB.transpose(-1, -2)
    delta = (P * dP).sum(dim=-1, keepdim=True)  # from the P and dP that make dS: its rows sum to zero up to their rounding
    dS = r_bf16(P * (dP - delta))
    dQ = scale * (dS @ kB)
    dK = scale * (dS.transpose(-1, -2) @ qB)
    return torch.cat([tokens_of(dQ), tokens_of(dK), tokens_of(dV)], dim=-1)


def emulate(qkv, gy, heads):
    """(out, lse, dqkv) of the contract, float64 tensors holding the values the device is asked to produce."""
    out, lse, S = emulate_fwd(qkv, heads)
    return out, lse, emulate_bwd(qkv, lse, S, gy, heads)


class _EmulatedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads):
        out, lse, S = emulate_fwd(qkv, heads)
        ctx.heads = heads
        ctx.save_for_backward(qkv, lse, S)
        return out

    @staticmethod
    def backward(ctx, gy):
        qkv, lse, S = ctx.saved_tensors
        return emulate_bwd(qkv, lse, S, gy, ctx.heads), None


def exact_attention(qkv, heads):
    q, k, v = (heads_of(u, heads) for u in qkv.chunk(3, dim=-1))
    return tokens_of(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1]), dim=-1) @ v)


def structure_map(img):
    """(N, 3, H, W) -> (N, L, 4): per 4x4 cell mean R, G, B and mean |dx| + |dy| of the luminance (forward differences, none across
    the border)."""
    lum = 0.299 * img[:, 0] + 0.587 * img[:, 1] + 0.114 * img[:, 2]
    gx, gy = torch.zeros_like(lum), torch.zeros_like(lum)
    gx[:, :, :-1] = lum[:, :, 1:] - lum[:, :, :-1]
    gy[:, :-1, :] = lum[:, 1:, :] - lum[:, :-1, :]
    feats = torch.cat([img, (gx.abs() + gy.abs()).unsqueeze(1)], dim=1)
    return F.avg_pool2d(feats, 4).flatten(2).transpose(1, 2)


BLOCK_PARAMS = ("struct_proj", "style_mod", "norm1", "qkv", "proj", "norm2", "fc1", "fc2")


def block_emulated(params, x, style, img, heads=4, attention="emulated"):
    """The block in float64.  params: {"qkv.weight": tensor, ...} (float64 leaves); attention "emulated" or "exact"."""
    w = lambda n: (params[n + ".weight"], params[n + ".bias"])  # noqa: E731
    dim = x.shape[-1]
    s = structure_map(img.double()).detach()
    h = x + F.linear(s, *w("struct_proj"))
    g, b = F.linear(style, *w("style_mod")).chunk(2, dim=-1)
    u = F.layer_norm(h, (dim,), *w("norm1"), 1e-5) * (1 + g[:, None, :]) + b[:, None, :]
    qkv = F.linear(u, *w("qkv"))
    a = _EmulatedAttention.apply(qkv, heads) if attention == "emulated" else exact_attention(qkv, heads)
    h = h + F.linear(a, *w("proj"))
    m = F.gelu(F.linear(F.layer_norm(h, (dim,), *w("norm2"), 1e-5), *w("fc1")))
    return h + F.linear(m, *w("fc2"))
