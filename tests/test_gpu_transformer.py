"""BUILD-DEFINED StructuralTransformerBlock (structural_transformer.py; csrc/transformer.hip) through the C ABI, against the
oracle's restatement of the same definition and against plain torch for the generic pieces (LayerNorm, softmax attention).
PARITY UNPINNED: the reference's file is missing from its snapshot; what is checked is kernel == definition."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def report(name, err, tol):
    print(f"  [parity] {name:64s} rel-L2 {err:.2e} (tol {tol:.0e})")
    assert err <= tol, f"{name}: {err:.3e} > {tol:.0e}"


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def test_structure_map_vs_oracle():
    from mstg_hip import ops
    from oracle import restatement as R
    x = R.make_input((2, 3, 32, 48), 1)
    s = ops.structure_map(x.to(DEV))
    report("structure_map", rel_l2(s.reshape(2, -1, 4), R.structure_map(x)), 1e-6)


@pytest.mark.parametrize("N,L,dim,mod", [(2, 64, 32, True), (1, 200, 64, True), (2, 96, 256, False), (1, 33, 128, True)])
def test_layer_norm_mod_vs_torch(N, L, dim, mod):
    from mstg_hip import ops
    x, ga, be = rnd((N, L, dim), 1) * 2 + 0.3, 1 + 0.1 * rnd((dim,), 2), 0.1 * rnd((dim,), 3)
    gm, bm = (0.2 * rnd((N, dim), 4), 0.2 * rnd((N, dim), 5)) if mod else (None, None)
    gy = rnd((N, L, dim), 6)
    leaves = [t.clone().requires_grad_(True) for t in (x, ga, be)] + ([t.clone().requires_grad_(True) for t in (gm, bm)] if mod else [])
    ref = F.layer_norm(leaves[0], (dim,), leaves[1], leaves[2], 1e-5)
    if mod:
        ref = ref * (1 + leaves[3][:, None]) + leaves[4][:, None]
    gr = torch.autograd.grad((ref * gy).sum(), leaves)
    dl = [t.to(DEV).requires_grad_(True) for t in (x, ga, be)] + ([t.to(DEV).requires_grad_(True) for t in (gm, bm)] if mod else [])
    y = ops.layer_norm_mod(dl[0], dl[1], dl[2], dl[3] if mod else None, dl[4] if mod else None)
    gg = torch.autograd.grad((y * gy.to(DEV)).sum(), dl)
    report(f"ln_mod dim{dim} y", rel_l2(y, ref), 1e-5)
    for name, a, b in zip(("dx", "dgamma", "dbeta", "dgmod", "dbmod"), gg, gr):
        report(f"ln_mod dim{dim} {name}", rel_l2(a, b), 2e-5)


@pytest.mark.parametrize("N,L,heads,D", [(2, 64, 4, 8), (1, 96, 4, 16), (1, 200, 2, 32), (1, 130, 4, 64), (1, 1024, 4, 16)])
def test_flash_attention_vs_torch(N, L, heads, D):
    from mstg_hip import ops
    dim = heads * D
    qkv = rnd((N, L, 3 * dim), 1, 0.8)
    gy = rnd((N, L, dim), 2)

    def ref_attn(t):
        q, k, v = (u.reshape(N, L, heads, D).transpose(1, 2) for u in t.chunk(3, dim=-1))
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D), dim=-1) @ v
        return a.transpose(1, 2).reshape(N, L, dim)

    tr = qkv.clone().double().requires_grad_(True)
    yr = ref_attn(tr)
    (gr,) = torch.autograd.grad((yr * gy.double()).sum(), [tr])
    tg = qkv.to(DEV).requires_grad_(True)
    y = ops.flash_attention(tg, heads)
    (gg,) = torch.autograd.grad((y * gy.to(DEV)).sum(), [tg])
    report(f"flash attention L{L} heads{heads} D{D} out", rel_l2(y, yr), 1e-5)
    report(f"flash attention L{L} heads{heads} D{D} dqkv", rel_l2(gg, gr), 2e-5)


# ---- the edges of the token kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 4, 4), (3, 3, 20, 36)])
def test_structure_map_borders(shape):
    """The right and bottom borders drop their forward difference; a single-cell image is all border."""
    from mstg_hip import ops
    from oracle import restatement as R
    x = R.make_input(shape, 2)
    s = ops.structure_map(x.to(DEV))
    report(f"structure_map {shape}", rel_l2(s.reshape(shape[0], -1, 4), R.structure_map(x.double())), 1e-6)


# ln_mod_bwd_kernel splits L into chunks of up to 512 tokens (at most 64 of them) and ln_mod_reduce_kernel adds them; a thread row
# serves 64 channels at a time, so dim = 96, 160, 200, 252 leave the last 64-channel chunk partly filled
LN_EDGES = [(1, 1, 4, True), (3, 5, 8, True), (2, 33, 96, True), (1, 70, 160, False), (2, 17, 200, True), (1, 40, 252, True),
            (2, 1100, 32, True),   # three chunks, the last one shorter
            (1, 513, 64, False),   # two chunks
            (1, 33000, 32, True)]  # the cap of 64 chunks


@pytest.mark.parametrize("N,L,dim,mod", LN_EDGES)
def test_layer_norm_mod_edges_vs_fp64(N, L, dim, mod):
    """Against fp64 F.layer_norm plus modulation at the bars of test_layer_norm_mod_vs_torch.  dgamma and dbeta of the two long cases
    add N * L >= 2200 products in fp32: their bar is max(2e-5, 4 * d32), d32 the distance of torch's own fp32 evaluation on the CPU
    from fp64 (printed; the margin of 4 is test_generator_with_block_vs_oracle's for one fp32 evaluation against another).
    The MI355X run printed d32 = 2.1e-07 / 1.7e-07 (L = 1100) and 9.7e-07 / 1.3e-06 (L = 33000), so the bar stayed 2e-5; the kernel
    sat at 1.3e-07 / 1.1e-07 and 1.6e-07 / 2.6e-07."""
    from mstg_hip import ops
    x, ga, be = rnd((N, L, dim), 1) * 2 + 0.3, 1 + 0.1 * rnd((dim,), 2), 0.1 * rnd((dim,), 3)
    ts = [x, ga, be] + ([0.2 * rnd((N, dim), 4), 0.2 * rnd((N, dim), 5)] if mod else [])
    gy = rnd((N, L, dim), 6)

    def ref(dtype):
        leaves = [t.to(dtype).requires_grad_(True) for t in ts]
        y = F.layer_norm(leaves[0], (dim,), leaves[1], leaves[2], 1e-5)
        if mod:
            y = y * (1 + leaves[3][:, None]) + leaves[4][:, None]
        return y.detach(), torch.autograd.grad((y * gy.to(dtype)).sum(), leaves)

    yr, gr = ref(torch.float64)
    dl = [t.to(DEV).requires_grad_(True) for t in ts]
    y = ops.layer_norm_mod(dl[0], dl[1], dl[2], dl[3] if mod else None, dl[4] if mod else None)
    gg = torch.autograd.grad((y * gy.to(DEV)).sum(), dl)
    report(f"ln_mod N{N} L{L} dim{dim} y", rel_l2(y, yr), 1e-5)
    tols = {}
    if N * L >= 2200:
        _, g32 = ref(torch.float32)
        for j, name in ((1, "dgamma"), (2, "dbeta")):
            d32 = rel_l2(g32[j], gr[j])
            print(f"  [parity] ln_mod N{N} L{L} dim{dim} {name}: torch fp32 (CPU) vs fp64 {d32:.2e}")
            tols[name] = max(2e-5, 4.0 * d32)
    for name, a, b in zip(("dx", "dgamma", "dbeta", "dgmod", "dbmod"), gg, gr):
        report(f"ln_mod N{N} L{L} dim{dim} {name}", rel_l2(a, b), tols.get(name, 2e-5))


def _flash_ref(qkv, gy, heads, dtype):
    N, L, C3 = qkv.shape
    dim = C3 // 3
    D = dim // heads
    t = qkv.to(dtype).requires_grad_(True)
    q, k, v = (u.reshape(N, L, heads, D).transpose(1, 2) for u in t.chunk(3, dim=-1))
    a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D), dim=-1) @ v
    y = a.transpose(1, 2).reshape(N, L, dim)
    (g,) = torch.autograd.grad((y * gy.to(dtype)).sum(), [t])
    return y.detach(), g


def _flash_hip(qkv, gy, heads):
    from mstg_hip import ops
    tg = qkv.to(DEV).requires_grad_(True)
    y = ops.flash_attention(tg, heads)
    (gg,) = torch.autograd.grad((y * gy.to(DEV)).sum(), [tg])
    return y.detach(), gg


@pytest.mark.parametrize("N,L,heads,D", [(2, 130, 2, 16), (3, 5, 1, 8), (2, 127, 1, 64), (1, 65, 4, 32), (2, 15, 4, 8)])
def test_flash_attention_ragged_tiles_of_several_images(N, L, heads, D):
    """N > 1 with L % 64 != 0: the tail of an image's last key tile lies in the next image's tokens, whose scores are masked; L < 16 is
    less than one MFMA tile of keys."""
    dim = heads * D
    qkv, gy = rnd((N, L, 3 * dim), 1, 0.8), rnd((N, L, dim), 2)
    yr, gr = _flash_ref(qkv, gy, heads, torch.float64)
    y, gg = _flash_hip(qkv, gy, heads)
    report(f"flash attention N{N} L{L} heads{heads} D{D} out", rel_l2(y, yr), 1e-5)
    report(f"flash attention N{N} L{L} heads{heads} D{D} dqkv", rel_l2(gg, gr), 2e-5)


def test_flash_attention_single_token():
    """One token: the softmax is exactly 1, so out == v and dv == d_out bit for bit, and nothing reaches q and k."""
    qkv, gy = rnd((1, 1, 24), 3, 0.8), rnd((1, 1, 8), 4)
    y, gg = _flash_hip(qkv, gy, 1)
    assert torch.equal(y.cpu(), qkv[..., 16:])
    assert torch.equal(gg[..., 16:].cpu(), gy)
    assert float(gg[..., :16].abs().max()) <= 1e-5


def test_flash_attention_large_logits():
    """q and k scaled by 6 (v left alone): the logits reach about +-100 and the softmax is nearly one-hot, so the running maximum
    carries the result.  The rounding of a logit of size 100 alone moves a probability by 1e-5: the bar is max(existing bar,
    4 * d32), d32 the distance of torch's own fp32 evaluation on the CPU from fp64 (printed).  The MI355X run printed max |logit|
    111.2, d32 = 1.17e-06 (out) and 3.17e-06 (dqkv) -- the existing bars stood -- and the kernel at 1.17e-06 and 3.55e-06."""
    N, L, heads, D = 1, 200, 2, 64
    dim = heads * D
    qkv, gy = rnd((N, L, 3 * dim), 1, 0.8), rnd((N, L, dim), 2)
    qkv[..., :2 * dim] *= 6.0
    yr, gr = _flash_ref(qkv, gy, heads, torch.float64)
    q, k = (u.reshape(N, L, heads, D).transpose(1, 2).double() for u in qkv.chunk(3, dim=-1)[:2])
    big = float((q @ k.transpose(-1, -2) / math.sqrt(D)).abs().max())
    print(f"  [parity] flash attention large logits: max |logit| {big:.1f}")
    assert big > 80
    y32, g32 = _flash_ref(qkv, gy, heads, torch.float32)
    d32y, d32g = rel_l2(y32, yr), rel_l2(g32, gr)
    print(f"  [parity] flash attention large logits: torch fp32 (CPU) vs fp64 out {d32y:.2e} dqkv {d32g:.2e}")
    y, gg = _flash_hip(qkv, gy, heads)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gg).all())
    report("flash attention large logits out", rel_l2(y, yr), max(1e-5, 4.0 * d32y))
    report("flash attention large logits dqkv", rel_l2(gg, gr), max(2e-5, 4.0 * d32g))


def test_flash_attention_reads_no_token_past_the_last():
    """The kernels mask the scores of keys past L, so what a key tile's tail holds cannot show in the result as long as it is
    finite (0 * finite = 0) -- the next image's tokens are.  What fa_stage's own bound (t0 + t < L) keeps out is memory behind the
    tensor: here qkv and d_out are the heads of larger buffers whose tails (64 token rows, one full tile) hold NaN, handed to the C
    ABI as pointers.  A staged row from there turns every output into NaN (0 * NaN)."""
    from mstg_hip import _lib
    lib = _lib.load()
    N, L, heads, D = 2, 70, 2, 16
    dim = heads * D
    qkv, gy = rnd((N, L, 3 * dim), 7, 0.8), rnd((N, L, dim), 8)
    yr, gr = _flash_ref(qkv, gy, heads, torch.float64)
    nan = float("nan")
    qkv_b = torch.cat([qkv.reshape(-1), torch.full((64 * 3 * dim,), nan)]).to(DEV)
    gy_b = torch.cat([gy.reshape(-1), torch.full((64 * dim,), nan)]).to(DEV)
    out = torch.empty((N, L, dim), device=DEV)
    lse, delta = torch.empty((N, heads, L), device=DEV), torch.empty((N, heads, L), device=DEV)
    dqkv = torch.empty((N, L, 3 * dim), device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.mstg_flash_attn_fwd(qkv_b.data_ptr(), out.data_ptr(), lse.data_ptr(), N, L, heads, D, st), "mstg_flash_attn_fwd")
    _lib.check(lib.mstg_flash_attn_bwd(qkv_b.data_ptr(), out.data_ptr(), lse.data_ptr(), gy_b.data_ptr(), dqkv.data_ptr(), delta.data_ptr(),
                                       N, L, heads, D, st), "mstg_flash_attn_bwd")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all())
    report("flash attention, NaN behind the tensor: out", rel_l2(out, yr), 1e-5)
    report("flash attention, NaN behind the tensor: dqkv", rel_l2(dqkv, gr), 2e-5)


@pytest.mark.parametrize("C_,shape", [(8, (2, 3, 32, 32)), (16, (1, 3, 64, 48))])
def test_block_vs_oracle(C_, shape):
    from oracle import restatement as R
    import structural_transformer as stx
    dim = 4 * C_
    sd = R.make_state_dict(R.transformer_block_spec(dim, "b"), 11)
    sd["b.style_mod.weight"] = 0.05 * rnd(tuple(sd["b.style_mod.weight"].shape), 12)  # the module zero-initialises it
    blk = stx.StructuralTransformerBlock(dim)
    blk.load_state_dict({k[2:]: v for k, v in sd.items()})
    blk.to(DEV)
    N, L = shape[0], (shape[2] // 4) * (shape[3] // 4)
    x, style, img = rnd((N, L, dim), 13), rnd((N, dim), 14).abs(), R.make_input(shape, 15)
    gy = rnd((N, L, dim), 16)
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xr, sr = x.clone().requires_grad_(True), style.clone().requires_grad_(True)
    yr = R.structural_transformer_block(sdr, "b", xr, sr, img)
    names = list(sd)
    gr = torch.autograd.grad((yr * gy).sum(), [xr, sr] + [sdr[k] for k in names])
    xg, sg = x.to(DEV).requires_grad_(True), style.to(DEV).requires_grad_(True)
    y = blk(xg, sg, img.to(DEV))
    params = dict(blk.named_parameters())
    gg = torch.autograd.grad((y * gy.to(DEV)).sum(), [xg, sg] + [params[k[2:]] for k in names])
    report(f"block dim{dim} out", rel_l2(y, yr), 2e-5)
    for name, a, b in zip(["dx", "dstyle"] + names, gg, gr):
        report(f"block dim{dim} d {name}", rel_l2(a, b), 1e-4)


@pytest.mark.parametrize("C_,shape", [(8, (2, 3, 32, 32)), (16, (1, 3, 64, 64))])
def test_generator_with_block_vs_oracle(C_, shape):
    """EnhancedGenerator(num_transformer_blocks=1) -- what every caller of the reference builds -- forward and all gradients
    (style encoder included: it is live now, enhanced_generator.py:142-147,216) against the oracle; strict state_dict round trip."""
    import enhanced_generator as eg
    from oracle import restatement as R
    spec = R.generator_spec_with_blocks(C_, 1)
    sd = R.make_state_dict(spec, 21)
    sd["transformer_blocks.0.style_mod.weight"] = 0.05 * rnd(tuple(sd["transformer_blocks.0.style_mod.weight"].shape), 22)
    m = eg.EnhancedGenerator(channels=C_, num_transformer_blocks=1)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == spec
    m.load_state_dict(sd)  # strict
    m.to(DEV)
    x = R.make_input(shape, 23)
    xg = x.to(DEV).requires_grad_(True)
    taps = {}
    y = m.forward_taps(xg, taps)
    names = [k for k, _ in m.named_parameters()]
    grads = torch.autograd.grad(y.abs().mean(), [xg] + list(m.parameters()))
    sdr = {k: v.clone().double().requires_grad_(True) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    tr = {}
    yr = R.generator_forward(sdr, xr, tr, num_blocks=1)
    gr = torch.autograd.grad(yr.abs().mean(), [xr] + [sdr[k] for k in names])
    report(f"G[blocks=1, C={C_}] pre_tanh", rel_l2(taps["pre_tanh"], tr["pre_tanh"]), 1e-4)
    report(f"G[blocks=1, C={C_}] out", rel_l2(y, yr), 1e-4)
    with torch.no_grad():
        sv = m._style_vector(taps["down2"])
    report(f"G[blocks=1, C={C_}] style vector (a9)", rel_l2(sv, R.style_encoder(sdr, tr["down2"])), 1e-5)
    # the same gradients from the oracle run in fp32: at these sizes the fp32 evaluation of the network sits percents away from
    # fp64 (ReLU-mask flips); the bar is "within 2e-3 of fp64, or no further from it than 1.5x the fp32 oracle"
    sd32 = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    x32 = x.clone().requires_grad_(True)
    g32 = torch.autograd.grad(R.generator_forward(sd32, x32, None, num_blocks=1).abs().mean(), [x32] + [sd32[k] for k in names])
    num = den = num32 = numo = 0.0
    for n, a, b, c in zip(["dx"] + names, grads, gr, g32):
        if n.endswith(".bias") and not n.startswith(("transformer_blocks", "style_encoder")) and not n.endswith(("qkv.bias", "proj.bias", "output.0.bias")):
            continue  # conv biases in front of an InstanceNorm: exactly-zero gradient (rounding noise in any implementation)
        num += float((a.cpu().double() - b).pow(2).sum())
        num32 += float((c.double() - b).pow(2).sum())
        numo += float((a.cpu().double() - c.double()).pow(2).sum())
        den += float(b.pow(2).sum())
    d32 = (num32 / den) ** 0.5
    print(f"  [parity] G[blocks=1, C={C_}] fp32 oracle vs fp64 oracle: {d32:.2e}")
    # One draw of a flip-driven error: tests/test_gpu_models.py::test_train_step_gradient_distance_distribution measures how two
    # correct fp32 evaluations of this network family scatter around fp64 ON THE SAME DRAW -- they flip different masks, the ratio of
    # their distances ranges over 0.2 ... 4 across 96 samples while the distributions agree (medians within 4 %).  The round-2 bar
    # "1.5 x the fp32 oracle's distance" on a single draw asserted more than that scatter allows; the bar is the scatter's edge.
    # The distance between the two fp32 evaluations follows from the two fp64 distances (triangle inequality) and is printed.
    print(f"  [parity] G[blocks=1, C={C_}] all gradients vs oracle (fp32): {(numo / den) ** 0.5:.2e}")
    report(f"G[blocks=1, C={C_}] all gradients vs oracle (fp64)", (num / den) ** 0.5, max(2e-3, 4.0 * d32))
    # round trip: a state_dict written by this module loads back strictly, inference callers' pattern (eval + no_grad)
    m2 = eg.EnhancedGenerator(channels=C_, num_transformer_blocks=1)
    m2.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    m2.to(DEV).eval()
    with torch.no_grad():
        assert torch.equal(m2(x.to(DEV)), m.eval()(x.to(DEV)))


def test_train_step_with_blocks_runs_and_is_deterministic():
    import enhanced_train

    def run():
        torch.manual_seed(5)
        m = enhanced_train.EnhancedCycleGAN(channels=8, device=torch.device(DEV))  # reference default: num_transformer_blocks=1
        assert len(m.G_AB.transformer_blocks) == 1 and not m.G_AB.transformer_blocks[0].is_identity
        g = torch.Generator().manual_seed(6)
        a = (torch.rand((2, 3, 64, 64), generator=g) * 2 - 1).to(DEV)
        b = (torch.rand((2, 3, 64, 64), generator=g) * 2 - 1).to(DEV)
        out = [m.train_step(a, b) for _ in range(2)]
        return out, m.g_optimizer.flat.clone()

    o1, f1 = run()
    o2, f2 = run()
    assert all(math.isfinite(v) for d in o1 for v in d.values())
    assert o1 == o2 and torch.equal(f1, f2)
    # the block's parameters received gradients and moved
    torch.manual_seed(5)
    fresh = enhanced_train.EnhancedCycleGAN(channels=8, device=torch.device(DEV))
    moved = (fresh.g_optimizer.flat - f1).abs().max()
    assert float(moved) > 0
