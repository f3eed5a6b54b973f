"""fp16 StructuralTransformerBlock (csrc/infer_f16_block.hip, mstg_hip/infer_block.py, ``half_inference(fp16_blocks=True)``).

Bars.  Per kernel: relative L2 2e-3 against fp32 torch on the CPU evaluated on the SAME fp16-rounded operands (the per-kernel bar
of test_gpu_f16.py).  Whole block: 3e-3 against oracle.restatement.structural_transformer_block in fp32 on the fp16-rounded
tokens.  Whole generator: 3e-2 at the taps and pre-tanh, 2e-2 on the image, against this build's fp32 path (the bars of
test_f16_generator_with_transformer_block_vs_fp32_path).

Expected errors.  A CPU emulation with the oracle's arithmetic that rounds to fp16 at every GEMM operand, at P and at every stored
tensor (statistics, softmax and accumulation fp32) gives 2.0e-4 .. 2.9e-4 for the attention (L 240 / 1024 / 4096, D 16 / 32 / 64,
scores up to +-110) and 5.0e-4 .. 6.6e-4 for the block (C = 16 at 64x64 and 256x256, C = 64 at 64x64): the bars leave a margin of
3x or more for what a kernel adds to that model (summation order, v_exp_f32's 1-ulp error), both far below one fp16 rounding."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from f16_helpers import DEV, _lib_loaded, report, rnd  # noqa: F401

pytestmark = pytest.mark.gpu


def attn_ref(qkv, heads):
    """softmax(q k^T / sqrt(D)) v on the CPU in fp32, one (image, head) at a time; qkv (N, L, 3 heads D) -> (N, L, heads D)"""
    N, L, C3 = qkv.shape
    dim = C3 // 3
    D = dim // heads
    out = torch.empty((N, L, dim))
    for n in range(N):
        for hh in range(heads):
            q = qkv[n, :, hh * D:(hh + 1) * D]
            k = qkv[n, :, dim + hh * D:dim + (hh + 1) * D]
            v = qkv[n, :, 2 * dim + hh * D:2 * dim + (hh + 1) * D]
            out[n, :, hh * D:(hh + 1) * D] = torch.softmax(q @ k.T / math.sqrt(D), dim=-1) @ v
    return out


def row_argmax(qkv, heads):
    N, L, C3 = qkv.shape
    dim = C3 // 3
    D = dim // heads
    am = []
    for n in range(N):
        for hh in range(heads):
            q = qkv[n, :, hh * D:(hh + 1) * D]
            k = qkv[n, :, dim + hh * D:dim + (hh + 1) * D]
            am.append((q @ k.T).argmax(dim=-1))
    return torch.stack(am)


def make_qkv(N, L, heads, D, seed, scale=1.0, peak=None):
    """fp16 qkv (N, L, 3 heads D).  peak = "first" / "last": every query is 0.3 noise + one direction u per head and key 0 / key
    L - 1 is 4 u, so that every query's row maximum sits in the first / last key tile (score 4 sqrt(D) +- 1.2 against a maximum
    of about 6 over the other keys)."""
    t = rnd((N, L, 3, heads, D), seed, scale)
    if peak is not None:
        u = rnd((heads, D), seed + 1)
        u = u / u.norm(dim=-1, keepdim=True) * math.sqrt(D)
        t[:, :, 0] = 0.3 * t[:, :, 0] + u
        t[:, 0 if peak == "first" else L - 1, 1] = 4 * u
    return t.reshape(N, L, 3 * heads * D).half()


FLASH_CASES = [(D, N, L) for D in (16, 32, 64) for N in (1, 3) for L in (48, 112, 240, 4096)]


@pytest.mark.parametrize("D,N,L", FLASH_CASES, ids=[f"D{d}-N{n}-L{l}" for d, n, l in FLASH_CASES])
def test_flash_attention_f16(D, N, L):
    from mstg_hip import infer_block
    heads = 4
    qkv = make_qkv(N, L, heads, D, 1000 + D + N + L)
    qd = qkv.to(DEV)
    y = infer_block.flash_attention(qd, heads)
    y2 = infer_block.flash_attention(qd, heads)
    assert y.dtype == torch.float16 and y.shape == (N, L, heads * D) and torch.isfinite(y).all()
    assert torch.equal(y, y2)
    report(f"flash fp16 D{D} N{N} L{L}", rel_l2(y.float().cpu(), attn_ref(qkv.float(), heads)), 2e-3)
    if N == 3:
        y1 = infer_block.flash_attention(qd[1:2].contiguous(), heads)
        assert torch.equal(y[1:2], y1)  # image 1 of the batch == the image alone, bit for bit


SHARP_CASES = [(D, L, peak) for D in (16, 32, 64) for L in (240, 4096) for peak in (None, "first", "last")]


@pytest.mark.parametrize("D,L,peak", SHARP_CASES, ids=[f"D{c[0]}-L{c[1]}-{c[2] or 'sharp'}" for c in SHARP_CASES])
def test_flash_attention_f16_sharp_and_rescale_paths(D, L, peak):
    """Scores of about +-100 (the scores are not bounded), and every query's row maximum in the first / the last key tile."""
    from mstg_hip import infer_block
    heads, N = 4, 2
    scale = 4.5 if peak is None else 1.0  # sharp: q.k / sqrt(D) with standard deviation 20, extremes beyond +-90
    qkv = make_qkv(N, L, heads, D, 2000 + D + L, scale, peak)
    qf = qkv.float()
    dim = heads * D
    if peak is None:
        s = torch.stack([qf[n, :, h * D:(h + 1) * D] @ qf[n, :, dim + h * D:dim + (h + 1) * D].T for n in range(N) for h in range(heads)])
        smax = float(s.abs().max()) / math.sqrt(D)
        print(f"  max |score| {smax:.1f}")
        assert smax > 90
    else:
        am = row_argmax(qf, heads)
        want = 0 if peak == "first" else L - 1
        assert (am == want).all(), "the case does not put every row maximum where it says"
    y = infer_block.flash_attention(qkv.to(DEV), heads)
    assert torch.isfinite(y).all()
    report(f"flash fp16 D{D} L{L} {peak or 'scores ~ +-100'}", rel_l2(y.float().cpu(), attn_ref(qf, heads)), 2e-3)


def test_flash_attention_f16_1024_tokens_vs_fp32_kernel():
    """L = 65536 (a 1024x1024 image), N = 1, D = 16: against the fp32 flash_fwd_kernel (pinned to torch in
    test_gpu_transformer.py) on the same fp16-rounded qkv."""
    from mstg_hip import infer_block, ops
    heads, D, L = 4, 16, 65536
    qkv = make_qkv(1, L, heads, D, 3001).to(DEV)
    with torch.no_grad():
        y = infer_block.flash_attention(qkv, heads)
        ref = ops.flash_attention(qkv.float(), heads)
    assert torch.isfinite(y).all()
    report("flash fp16 D16 L65536 vs fp32 flash_fwd_kernel", rel_l2(y.float(), ref), 2e-3)


def linear_cases():
    out = []
    for dim in (64, 128, 256):
        out += [(dim, 3 * dim, "none", True), (dim, dim, "res", False), (dim, 2 * dim, "gelu", True), (2 * dim, dim, "res", False),
                (2 * dim, dim, "res", True)]
    return out


LIN = linear_cases()


@pytest.mark.parametrize("Cin,Cout,epi,out_f16", LIN, ids=[f"{a}-{b}-{c}-{'f16' if d else 'f32'}" for a, b, c, d in LIN])
def test_token_gemm(Cin, Cout, epi, out_f16):
    from mstg_hip import infer_block
    from mstg_hip._lib import ACT_GELU, ACT_NONE
    N, L = 2, 240  # 480 tokens: not a multiple of the 64-token tile
    w, b = rnd((Cout, Cin), 1, Cin ** -0.5), rnd((Cout,), 2, 0.1)
    x = rnd((N, L, Cin), 3).half()
    res = rnd((N, L, Cout), 4) if epi == "res" else None
    lin = infer_block.PackedLinear(w.to(DEV), b.to(DEV))
    y = lin(x.to(DEV), act=ACT_GELU if epi == "gelu" else ACT_NONE, residual=None if res is None else res.to(DEV), out_f16=out_f16)
    assert y.dtype == (torch.float16 if out_f16 else torch.float32)
    ref = F.linear(x.float(), w.half().float(), b)
    if epi == "gelu":
        ref = F.gelu(ref)
    if res is not None:
        ref = res + ref
    report(f"token GEMM {Cin}->{Cout} {epi} {'fp16' if out_f16 else 'fp32'} out", rel_l2(y.float().cpu(), ref), 2e-3)


@pytest.mark.parametrize("dim", [64, 128, 256])
@pytest.mark.parametrize("struct", [True, False])
@pytest.mark.parametrize("x_f16", [True, False])
def test_ln_mod(dim, struct, x_f16):
    from mstg_hip import infer_block
    N, L = 2, 240
    x = rnd((N, L, dim), 11) * 1.5 + 0.3
    if x_f16:
        x = x.half()
    gamma, beta = 1 + rnd((dim,), 12, 0.2), rnd((dim,), 13, 0.2)
    gb = rnd((N, 2 * dim), 14, 0.3)
    smap, spw, spb = rnd((N, L, 4), 15), rnd((dim, 4), 16, 0.5), rnd((dim,), 17, 0.1)
    d = lambda t: t.to(DEV).contiguous()
    if struct:
        u, hh = infer_block.ln_mod(d(x), d(gamma), d(beta), 1e-5, gb=d(gb), smap=d(smap), sp_w=d(spw), sp_b=d(spb), want_h=True)
        href = x.float() + F.linear(smap, spw, spb)
        report(f"struct_proj add dim{dim} x {'fp16' if x_f16 else 'fp32'}", rel_l2(hh.cpu(), href), 2e-3)
        uref = F.layer_norm(href, (dim,), gamma, beta, 1e-5) * (1 + gb[:, None, :dim]) + gb[:, None, dim:]
    else:
        u, hh = infer_block.ln_mod(d(x), d(gamma), d(beta), 1e-5)
        assert hh is None
        uref = F.layer_norm(x.float(), (dim,), gamma, beta, 1e-5)
    assert u.dtype == torch.float16
    report(f"LayerNorm{' + struct_proj' if struct else ''} + mod dim{dim} x {'fp16' if x_f16 else 'fp32'}", rel_l2(u.float().cpu(), uref), 2e-3)


@pytest.mark.parametrize("dim,N,L", [(64, 2, 4096), (64, 3, 240), (128, 1, 1200), (256, 2, 48), (64, 1, 65536)])
def test_token_mean(dim, N, L):
    from mstg_hip import infer_block
    x = (rnd((N, L, dim), 21) + 0.5).half()
    m = infer_block.token_mean(x.to(DEV))
    report(f"token mean dim{dim} N{N} L{L}", rel_l2(m.cpu(), x.float().mean(dim=1)), 2e-3)
    if N > 1:
        assert torch.equal(m[1:2], infer_block.token_mean(x[1:2].to(DEV)))


def _block_weights(C, seed, nblocks=1):
    from oracle import restatement as R
    return R.make_state_dict(R.generator_spec_with_blocks(C, nblocks), seed)


@pytest.mark.parametrize("C,H,W", [(16, 64, 64), (32, 64, 64), (64, 64, 64), (16, 256, 256)])
def test_block_vs_oracle(C, H, W):
    """One block, fp16 kernels, against the oracle's block in fp32 on the fp16-rounded tokens and the same style vector."""
    from mstg_hip import infer_block, ops
    from oracle import restatement as R
    from structural_transformer import StructuralTransformerBlock
    sd = _block_weights(C, 500 + C)
    p = "transformer_blocks.0"
    assert float(sd[p + ".style_mod.weight"].abs().max()) > 0  # the modulation is exercised
    dim, N = 4 * C, 2
    blk = StructuralTransformerBlock(dim)
    blk.load_state_dict({k[len(p) + 1:]: v for k, v in sd.items() if k.startswith(p + ".")})
    blk.to(DEV)
    L = (H // 4) * (W // 4)
    x = rnd((N, L, dim), 501).half()
    style = F.relu(rnd((N, dim), 502))
    img = R.make_input((N, 3, H, W), 503)
    hb = infer_block.HalfBlock(blk)
    with torch.no_grad():
        smap = ops.structure_map(img.to(DEV))
        y = hb.forward(x.to(DEV), smap, style.to(DEV), out_f16=True)
    assert y.dtype == torch.float16 and torch.isfinite(y).all()
    ref = R.structural_transformer_block(sd, p, x.float(), style, img)
    report(f"fp16 block C{C} {H}x{W} vs oracle", rel_l2(y.float().cpu(), ref), 3e-3)


def _gen(C, nblocks, seed):
    import enhanced_generator as eg
    m = eg.EnhancedGenerator(channels=C, num_transformer_blocks=nblocks)
    m.load_state_dict(_block_weights(C, seed, nblocks))
    return m.to(DEV).eval()


GEN_CASES = [(16, 1, (2, 3, 64, 64)), (16, 1, (1, 3, 48, 80)), (16, 1, (1, 3, 256, 256)), (64, 3, (1, 3, 64, 64)),
             (16, 1, (1, 3, 1024, 1024))]


@pytest.mark.parametrize("C,nblocks,shape", GEN_CASES, ids=[f"C{c}-b{b}-{s[0]}x{s[2]}x{s[3]}" for c, b, s in GEN_CASES])
def test_generator_fp16_blocks_vs_fp32_path(C, nblocks, shape):
    from oracle import restatement as R
    m = _gen(C, nblocks, 600 + C + nblocks)
    x = R.make_input(shape, 601).to(DEV)
    t32, t16, t16d = {}, {}, {}
    with torch.no_grad():
        y32 = m.forward_taps(x, t32)
        m.half_inference()
        y16d = m.forward_taps(x, t16d)
        m.half_inference(fp16_blocks=True)
        y16 = m.forward_taps(x, t16)
        y16b = m(x)
    assert y16.dtype == torch.float16 and torch.isfinite(y16).all() and torch.equal(y16, y16b)
    tag = f"C{C} blocks{nblocks} {shape[0]}x{shape[2]}x{shape[3]}"
    print(f"  [drift] {tag}: fp16_blocks vs default half: out rel-L2 {rel_l2(y16.float(), y16d.float()):.2e}, "
          f"pre_tanh {rel_l2(t16['pre_tanh'].float(), t16d['pre_tanh'].float()):.2e}; default half vs fp32: out "
          f"{rel_l2(y16d.float(), y32):.2e}")
    for k in ("down2", "up1", "up2", "pre_tanh"):
        report(f"fp16 blocks vs fp32 {tag} tap {k}", rel_l2(t16[k].float(), t32[k]), 3e-2)
    report(f"fp16 blocks vs fp32 {tag} out", rel_l2(y16.float(), y32), 2e-2)


def test_generator_fp16_blocks_batch_64_1024():
    """Batch 64 at 1024x1024 (qkv of 64 x 65536 x 192 halves, > 2^31 bytes of activations): finite, and samples 0 and 63 equal
    their batch-1 runs bit for bit."""
    from oracle import restatement as R
    m = _gen(16, 1, 611)
    m.half_inference(fp16_blocks=True)
    g = torch.Generator().manual_seed(612)
    x = (torch.rand((64, 3, 1024, 1024), generator=g) * 2 - 1).to(DEV)
    with torch.no_grad():
        y = m(x)
        y0, y63 = m(x[0:1].contiguous()), m(x[63:64].contiguous())
    assert torch.isfinite(y).all()
    assert torch.equal(y[0:1], y0) and torch.equal(y[63:64], y63)


def test_contract_default_half_unchanged_by_round_trip():
    from oracle import restatement as R
    m = _gen(16, 1, 621)
    x = R.make_input((2, 3, 64, 64), 622).to(DEV)
    with torch.no_grad():
        m.half_inference()
        y_a = m(x)
        m.half_inference(fp16_blocks=True)
        y_b = m(x)
        m.half_inference(fp16_blocks=False)
        y_c = m(x)
        m.half_inference()
        y_d = m(x)
    assert torch.equal(y_a, y_c) and torch.equal(y_a, y_d) and not torch.equal(y_a, y_b)


def test_contract_switch_validated_at_call_time():
    from structural_transformer import StructuralTransformerBlock
    m = _gen(16, 1, 631)
    m.transformer_blocks[0] = StructuralTransformerBlock(64, num_heads=8).to(DEV)  # head width 8: served by the fp32 kernels
    m.half_inference()
    with pytest.raises(RuntimeError, match="head width 8"):
        m.half_inference(fp16_blocks=True)
    m0 = _gen(16, 0, 632)
    x = torch.zeros((1, 3, 64, 64), device=DEV)
    with torch.no_grad():
        y_a = m0.half_inference()(x)
        y_b = m0.half_inference(fp16_blocks=True)(x)  # no blocks: accepted, no effect
    assert torch.equal(y_a, y_b)


def test_contract_block_weights_follow_load_state_dict():
    from oracle import restatement as R
    m = _gen(16, 1, 641)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = R.make_input((1, 3, 64, 64), 642).to(DEV)
    m.half_inference(fp16_blocks=True)
    with torch.no_grad():
        y1 = m(x)
        sd2 = {k: v.clone() for k, v in sd.items()}
        for k in sd2:
            if k.startswith("transformer_blocks.0.fc2."):
                sd2[k] = sd2[k] * 1.5 + 0.01
        m.load_state_dict(sd2)
        y2 = m(x)
        m.load_state_dict(sd)
        y3 = m(x)
    assert not torch.equal(y1, y2) and torch.equal(y1, y3)


def test_contract_graph_replay_and_switch():
    from oracle import restatement as R
    m = _gen(16, 1, 651)
    x = R.make_input((1, 3, 256, 256), 652).to(DEV)
    with torch.no_grad():
        m.half_inference(fp16_blocks=True)
        y_eager = m(x)
        m.half_inference()
        y_default = m(x)
        m.graph_inference()
        y_g_default = m(x)                         # captured without the switch
        assert torch.equal(y_g_default, y_default)
        m.half_inference(fp16_blocks=True)
        y_g = m(x)                                 # the switch turned on after the capture
        y_g2 = m(x)                                # replay
    assert torch.equal(y_g, y_eager) and torch.equal(y_g2, y_eager) and not torch.equal(y_g, y_default)


def test_contract_autograd_keeps_fp32_path():
    from oracle import restatement as R
    m = _gen(16, 1, 661)
    m.half_inference(fp16_blocks=True)
    x = R.make_input((1, 3, 64, 64), 662).to(DEV)
    y = m(x)
    assert y.dtype == torch.float32 and y.requires_grad
    y.float().mean().backward()
    assert m.transformer_blocks[0].qkv.weight.grad is not None
