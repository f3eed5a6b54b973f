"""Mixed-precision training attention (csrc/flash_f16_train.hip; ops.flash_attention(..., precision="mixed")) on the device, through
the C entries and through the autograd function, against tests/flash_f16_train_ref.py.

Every launch of the attention tests runs under guard_helpers.memory_contract (red zones round every output, workspace and upload;
inputs bit-compared afterwards), and so does the block test; the generator and step tests run the same kernels inside the
model.  Every kernel is launched twice into separate buffers and the two results are compared bit for bit.

Bars.  out <= 2e-3 against float64 attention on the fp16-rounded qkv (the project's per-kernel fp16 bar); lse <= 2e-5 (the per-op
fp32 bar); dqkv and each of its thirds <= 2 x the distance the CPU emulation of the contract has from the same yardstick, computed
here (the rule of test_gpu_style_f16.py::test_whole_loss_against_the_emulation), and for the randn * 0.8 inputs also <= 8e-3 (the
bf16 bar).  Device, emulation and bar are printed side by side."""
import functools
import math

import pytest
import torch

import flash_f16_train_ref as ref
from f16_helpers import DEV, _lib_loaded  # noqa: F401
from guard_helpers import memory_contract

pytestmark = pytest.mark.gpu

THIRDS = ("dq", "dk", "dv")


@functools.lru_cache(maxsize=None)
def case(N, L, heads, D, scale=0.8, gscale=1.0, qk_mul=1.0):
    """inputs, yardstick and emulation of one case, computed once and never modified"""
    dim = heads * D
    qkv, gy = ref.rnd((N, L, 3 * dim), 1, scale), ref.rnd((N, L, dim), 2) * gscale
    if qk_mul != 1.0:
        qkv[..., :2 * dim] *= qk_mul
    yard, emu = ref.yardstick(qkv, gy, heads), ref.emulate(qkv, gy, heads)
    return qkv, gy, yard, emu


def device_c(qkv, gy, heads):
    """cast, forward, backward through the C entries, each launched twice; returns CPU tensors (out, lse, dqkv)"""
    from mstg_hip import _lib, ops
    lib = _lib.load()
    N, L, C3 = qkv.shape
    dim = C3 // 3
    D = dim // heads
    st = torch.cuda.current_stream().cuda_stream
    with memory_contract() as mc:
        q, g = qkv.to(DEV), gy.to(DEV)
        res = []
        for _ in range(2):
            qh = torch.empty((N, L, C3), dtype=torch.float16, device=DEV)
            qb = torch.empty((N, L, C3), dtype=torch.bfloat16, device=DEV)
            out = torch.empty((N, L, dim), dtype=torch.float32, device=DEV)
            lse = torch.empty((N, heads, L), dtype=torch.float32, device=DEV)
            dqkv = torch.empty((N, L, C3), dtype=torch.float32, device=DEV)
            ws = ops._ws(lib.mstg_f16_flash_attn_train_bwd_workspace_bytes(N, L, heads, D), DEV)
            _lib.check(lib.mstg_f16_attn_cast_qkv(q.data_ptr(), qh.data_ptr(), qb.data_ptr(), N, L, heads, D, st), "cast")
            _lib.check(lib.mstg_f16_flash_attn_train_fwd(qh.data_ptr(), out.data_ptr(), lse.data_ptr(), N, L, heads, D, st), "fwd")
            _lib.check(lib.mstg_f16_flash_attn_train_bwd(qh.data_ptr(), qb.data_ptr(), lse.data_ptr(), g.data_ptr(),
                                                         dqkv.data_ptr(), ws.data_ptr(), ws.numel() * 4, N, L, heads, D, st), "bwd")
            for t in (qh, qb, out, lse, dqkv):
                mc.assert_written(t)
            res.append([t.cpu() for t in (qh, qb, out, lse, dqkv)])
        assert mc.outputs >= 10 and mc.workspaces == 2 and mc.uploads == 2
    for a, b, name in zip(res[0], res[1], ("qh", "qb", "out", "lse", "dqkv")):
        assert torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                           b.view(torch.int16 if b.element_size() == 2 else torch.int32)), f"two launches differ: {name}"
    assert torch.equal(res[0][0], qkv.half()) and torch.equal(res[0][1], qkv.bfloat16())  # round-to-nearest-even, both copies
    return res[0][2], res[0][3], res[0][4]


def device_ops(qkv, gy, heads, **kw):
    from mstg_hip import ops
    with memory_contract():
        tg = qkv.to(DEV).requires_grad_(True)
        y = ops.flash_attention(tg, heads, **kw)
        (gg,) = torch.autograd.grad((y * gy.to(DEV)).sum(), [tg])
        y, gg = y.detach().cpu(), gg.cpu()
    return y, gg


def device_both(qkv, gy, heads):
    """the C entries and the autograd function agree bit for bit"""
    out, lse, dqkv = device_c(qkv, gy, heads)
    y, gg = device_ops(qkv, gy, heads, precision="mixed")
    assert torch.equal(y, out) and torch.equal(gg, dqkv), "ops.flash_attention(precision='mixed') differs from the C entries"
    return out, lse, dqkv


def check(tag, dev, yard, emu, cap=8e-3):
    """dev, yard, emu: (out, lse, dqkv).  cap: the bf16 bar on top of the 2 x rule, None for inputs it was not measured on."""
    d_out, d_lse = ref.rel_l2(dev[0], yard[0]), ref.rel_l2(dev[1], yard[1])
    print(f"  [{tag}] out : device {d_out:.3e}  emulation {ref.rel_l2(emu[0], yard[0]):.3e}  bar 2e-3")
    print(f"  [{tag}] lse : device {d_lse:.3e}  emulation {ref.rel_l2(emu[1], yard[1]):.3e}  bar 2e-5")
    rows = [("dqkv", dev[2], yard[2], emu[2])] + [(k, a, b, c) for k, a, b, c in zip(
        THIRDS, ref.thirds(dev[2]).values(), ref.thirds(yard[2]).values(), ref.thirds(emu[2]).values())]
    fails = []
    for k, a, b, c in rows:
        d, e = ref.rel_l2(a, b), ref.rel_l2(c, b)
        bar = 2 * e if cap is None else min(2 * e, cap)
        print(f"  [{tag}] {k:4s}: device {d:.3e}  emulation {e:.3e}  bar {bar:.3e}")
        if not d <= bar:
            fails.append((k, d, bar))
    assert bool(torch.isfinite(dev[0]).all()) and bool(torch.isfinite(dev[1]).all()) and bool(torch.isfinite(dev[2]).all())
    assert d_out <= 2e-3, d_out
    assert d_lse <= 2e-5, d_lse
    assert not fails, fails


SHAPES = [(3, 5, 1, 16),      # fewer tokens than one MFMA block
          (2, 15, 4, 16),
          (1, 65, 4, 32),     # one full tile + 1
          (2, 127, 1, 64),
          (2, 130, 2, 16),    # two tiles + ragged, several images and heads
          (1, 200, 2, 32),
          (1, 1024, 4, 16)]


@pytest.mark.parametrize("N,L,heads,D", SHAPES)
def test_against_yardstick_and_emulation(N, L, heads, D):
    qkv, gy, yard, emu = case(N, L, heads, D)
    check(f"N{N} L{L} h{heads} D{D}", device_both(qkv, gy, heads), yard, emu)


def test_single_token_forward_and_dv():
    """One token: the softmax is 1, so out is the fp16-rounded v (to the last fp32 bits: p = exp2 of a rounding residue) and dv is
    dO up to the bf16 rounding of dO."""
    qkv, gy = ref.rnd((1, 1, 48), 3, 0.8), ref.rnd((1, 1, 16), 4)
    out, lse, dqkv = device_both(qkv, gy, 1)
    assert ref.rel_l2(out, qkv[..., 32:].half()) <= 1e-6
    assert ref.rel_l2(lse, ref.yardstick(qkv, gy, 1)[1]) <= 2e-5  # scale * q_h . k_h + ln 1
    d = ref.rel_l2(dqkv[..., 32:], gy)
    print(f"  [single token] dv against dO: {d:.3e} (bar 8e-3)")
    assert d <= 8e-3


def test_single_token_dq_dk_vanish():
    """One token: nothing reaches q and k; the bar is 1e-5 absolute.  It holds because delta is the sum over keys of P dP, from
    the same P and dP that dS is made of: with L = 1, dS = P (dP - P dP) and P = 1 up to the fp32 rounding of the log-sum-exp.
    (delta = sum_d dO out from the fp32 tensors, as the fp32 kernels form it, left 3.146e-3 here: dP sees the bf16 operands.)"""
    qkv, gy = ref.rnd((1, 1, 48), 3, 0.8), ref.rnd((1, 1, 16), 4)
    _, _, dqkv = device_both(qkv, gy, 1)
    emu = ref.emulate(qkv, gy, 1)[2]
    print(f"  [single token] max |dq|, |dk|: device {float(dqkv[..., :32].abs().max()):.3e}  emulation {float(emu[..., :32].abs().max()):.3e}"
          f"  bar 1e-5")
    assert float(dqkv[..., :32].abs().max()) <= 1e-5


def test_tiny_incoming_gradient_keeps_its_bits():
    """gy * 1e-7: bf16 has fp32's range, so the same bars hold and no third of the gradient is flushed to zero."""
    N, L, heads, D = 2, 130, 2, 16
    qkv, gy, yard, emu = case(N, L, heads, D, 0.8, 1e-7)
    dev = device_both(qkv, gy, heads)
    check("gy x 1e-7", dev, yard, emu)
    for k, t in ref.thirds(dev[2]).items():
        assert float(t.abs().max()) > 0, k


def test_sharp_rows():
    """randn * 3: near one-hot rows; the 2 x rule only."""
    qkv, gy, yard, emu = case(1, 200, 4, 16, 3.0)
    check("sharp rows", device_both(qkv, gy, 4), yard, emu, cap=None)


def test_large_logits():
    """The construction of test_gpu_transformer.py::test_flash_attention_large_logits: q and k scaled by 6, scores above 80."""
    N, L, heads, D = 1, 200, 2, 64
    qkv, gy, yard, emu = case(N, L, heads, D, 0.8, 1.0, 6.0)
    q, k = (ref.heads_of(u, heads).double() for u in qkv.chunk(3, dim=-1)[:2])
    big = float((q @ k.transpose(-1, -2) / math.sqrt(D)).abs().max())
    print(f"  [large logits] max |logit| {big:.1f}")
    assert big > 80
    check("large logits", device_both(qkv, gy, heads), yard, emu, cap=None)


def test_image_of_a_batch_equals_the_image_alone():
    qkv, gy, _, _ = case(2, 130, 2, 16)
    qkv3, gy3 = torch.cat([qkv, qkv[:1] * 0.5]), torch.cat([gy, gy[:1] * 2.0])
    batch = device_c(qkv3, gy3, 2)
    alone = device_c(qkv3[1:2].contiguous(), gy3[1:2].contiguous(), 2)
    for name, a, b in zip(("out", "lse", "dqkv"), batch, alone):
        assert torch.equal(a[1:2], b), name


def test_default_is_the_fp32_path():
    qkv, gy, _, _ = case(2, 130, 2, 16)
    y0, g0 = device_ops(qkv, gy, 2)
    y1, g1 = device_ops(qkv, gy, 2, precision="fp32")
    assert torch.equal(y0, y1) and torch.equal(g0, g1)
    ym, _ = device_ops(qkv, gy, 2, precision="mixed")
    assert not torch.equal(ym, y0)  # the switch does switch


def test_refusals_on_the_device():
    from mstg_hip import ops
    with pytest.raises(RuntimeError, match="head width 8"):
        ops.flash_attention(torch.zeros(1, 8, 96, device=DEV), 4, precision="mixed")
    with pytest.raises(ValueError, match="precision"):
        ops.flash_attention(torch.zeros(1, 8, 96, device=DEV), 4, precision="bf16")


# ---- the block ---------------------------------------------------------------------------------------------------------------
def test_block_against_the_float64_block():
    """StructuralTransformerBlock(64) (D = 16) on (1, 3, 64, 48), L = 192, attention_precision = "mixed", non-zero style_mod.
    Output <= 3e-3 against the float64 block (the block bar of test_gpu_f16_block.py).  dx, dstyle and every parameter gradient
    <= 2 x the distance block_emulated (float64 with the emulated attention) has from the float64 block.  Where that distance is
    below 5e-5 the attention does not reach the gradient (fc2.bias: the same sum in both float64 statements, distance 0) and the bar
    is 1e-4 instead, the fp32 kernels' own gradient bar against the oracle (test_gpu_transformer.py::test_block_vs_oracle): the
    emulation models none of their rounding.  The smallest other distance is 1.5e-4 (proj.bias).  Both runs sit under the red-zone
    guard."""
    from oracle import restatement as R
    from structural_transformer import StructuralTransformerBlock
    dim, shape = 64, (1, 3, 64, 48)
    sd = R.make_state_dict(R.transformer_block_spec(dim, "b"), 11)
    sd["b.style_mod.weight"] = 0.05 * ref.rnd(tuple(sd["b.style_mod.weight"].shape), 12)
    sd = {k[2:]: v for k, v in sd.items()}
    names = list(sd)
    N, L = shape[0], (shape[2] // 4) * (shape[3] // 4)
    x, style, img, gy = ref.rnd((N, L, dim), 13), ref.rnd((N, dim), 14).abs(), R.make_input(shape, 15), ref.rnd((N, L, dim), 16)

    def cpu(attention):
        p = {k: v.clone().double().requires_grad_(True) for k, v in sd.items()}
        xr, sr = x.double().requires_grad_(True), style.double().requires_grad_(True)
        y = ref.block_emulated(p, xr, sr, img, 4, attention)
        return y.detach(), torch.autograd.grad((y * gy.double()).sum(), [xr, sr] + [p[k] for k in names])

    y64, g64 = cpu("exact")
    yem, gem = cpu("emulated")
    blk = StructuralTransformerBlock(dim)
    blk.load_state_dict(sd)
    blk.to(DEV)
    blk.attention_precision = "mixed"
    res = []
    for _ in range(2):
        with memory_contract():
            xg, sg = x.to(DEV).requires_grad_(True), style.to(DEV).requires_grad_(True)
            y = blk(xg, sg, img.to(DEV))
            params = dict(blk.named_parameters())
            gg = torch.autograd.grad((y * gy.to(DEV)).sum(), [xg, sg] + [params[k] for k in names])
            res.append((y.detach().cpu(), [t.cpu() for t in gg]))
    assert torch.equal(res[0][0], res[1][0]) and all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1])), "two runs differ"
    y, gg = res[0]
    d = ref.rel_l2(y, y64)
    print(f"  [block] out: device {d:.3e}  emulation {ref.rel_l2(yem, y64):.3e}  bar 3e-3")
    fails = []
    for name, a, b, c in zip(["dx", "dstyle"] + names, gg, g64, gem):
        dd, e = ref.rel_l2(a, b), ref.rel_l2(c, b)
        bar = 2 * e if e >= 5e-5 else 1e-4
        print(f"  [block] d {name:20s}: device {dd:.3e}  emulation {e:.3e}  bar {bar:.3e}")
        if not dd <= bar:
            fails.append((name, dd, bar))
    assert d <= 3e-3
    assert not fails, fails


# ---- generator and step --------------------------------------------------------------------------------------------------------
def test_generator_mixed_against_the_fp32_path():
    """EnhancedGenerator(16, 1) at 1x3x64x64: the image within 2e-2 of the fp32 path's (the bar test_gpu_f16_block.py holds a forward
    that is 16-bit throughout to)."""
    import enhanced_generator as eg
    from oracle import restatement as R
    sd = R.make_state_dict(R.generator_spec_with_blocks(16, 1), 21)
    sd["transformer_blocks.0.style_mod.weight"] = 0.05 * ref.rnd(tuple(sd["transformer_blocks.0.style_mod.weight"].shape), 22)
    m = eg.EnhancedGenerator(16, 1)
    m.load_state_dict(sd)
    m.to(DEV)
    x = R.make_input((1, 3, 64, 64), 23).to(DEV)
    with torch.no_grad():
        y32 = m(x)
        ymx = m.set_attention_precision("mixed")(x)
        y32b = m.set_attention_precision("fp32")(x)
    assert torch.equal(y32, y32b) and not torch.equal(ymx, y32)
    d = ref.rel_l2(ymx, y32)
    print(f"  [generator] mixed attention against the fp32 path: image {d:.3e} (bar 2e-2)")
    assert d <= 2e-2


STEP_C, STEP_SHAPE = 16, (2, 3, 64, 64)


def build_step(precision, checkpointing=False):
    import enhanced_train
    from oracle import restatement as R
    torch.manual_seed(1234)
    model = enhanced_train.EnhancedCycleGAN(channels=STEP_C, num_transformer_blocks=1, device=torch.device(DEV),
                                            gradient_checkpointing=checkpointing, attention_precision=precision)
    sds = [R.make_state_dict(R.generator_spec_with_blocks(STEP_C, 1), 81), R.make_state_dict(R.generator_spec_with_blocks(STEP_C, 1), 82),
           R.make_state_dict(R.discriminator_spec(STEP_C), 83), R.make_state_dict(R.discriminator_spec(STEP_C), 84)]
    for s, seed in zip(sds[:2], (85, 86)):
        k = "transformer_blocks.0.style_mod.weight"
        s[k] = 0.05 * ref.rnd(tuple(s[k].shape), seed)
    for m, sd in zip((model.G_AB, model.G_BA, model.D_A, model.D_B), sds):
        m.load_state_dict(sd)
    return model


def run_step(model):
    from oracle import restatement as R
    a, b = R.make_input(STEP_SHAPE, 90).to(DEV), R.make_input(STEP_SHAPE, 91).to(DEV)
    before = model.g_optimizer.flat.clone()
    losses = model.train_step(a, b)
    return losses, before, model.g_optimizer.flat.clone(), model.d_optimizer.flat.clone()


_STEPS = {}


def steps():
    if not _STEPS:
        _STEPS["fp32"] = run_step(build_step("fp32"))
        _STEPS["mixed"] = run_step(build_step("mixed"))
    return _STEPS


def test_step_mixed():
    s = steps()
    l32, lmx, before, g, d = s["fp32"][0], *s["mixed"]
    lmx2, _, g2, d2 = run_step(build_step("mixed"))
    assert lmx2 == lmx and torch.equal(g2, g) and torch.equal(d2, d), "two runs from one seed differ"
    assert all(math.isfinite(v) for v in lmx.values()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(d).all())
    assert not torch.equal(before, g), "the generator parameters did not move"
    assert len(lmx) == 5
    for k in lmx:
        rel = abs(lmx[k] - l32[k]) / abs(l32[k])
        print(f"  [step] {k:16s} mixed {lmx[k]:.7e}  fp32 {l32[k]:.7e}  relative {rel:.2e} (bar 2e-2)")
    assert any(lmx[k] != l32[k] for k in lmx), "the mixed step ran the fp32 attention"
    for k in lmx:
        assert abs(lmx[k] - l32[k]) <= 2e-2 * abs(l32[k]), k


def test_step_checkpointing_recomputes_with_the_same_precision():
    lmx, _, g, d = steps()["mixed"]
    model = build_step("mixed", checkpointing=True)
    assert all(b.attention_precision == "mixed" for G in (model.G_AB, model.G_BA) for b in G.transformer_blocks)
    lck, _, gck, dck = run_step(model)
    assert lck == lmx and torch.equal(gck, g) and torch.equal(dck, d)


def test_environment_selects_the_precision(monkeypatch):
    monkeypatch.setenv("MSTG_ATTN_PRECISION", "mixed")
    model = build_step(None)
    assert model.attention_precision == "mixed"
    assert all(b.attention_precision == "mixed" for G in (model.G_AB, model.G_BA) for b in G.transformer_blocks)
    losses, _, g, _ = run_step(model)
    assert losses == steps()["mixed"][0] and torch.equal(g, steps()["mixed"][2])
    assert build_step("fp32").attention_precision == "fp32"  # an argument wins over the environment
    monkeypatch.setenv("MSTG_ATTN_PRECISION", "half")
    with pytest.raises(ValueError, match="precision"):
        build_step(None)
    monkeypatch.delenv("MSTG_ATTN_PRECISION")
    assert build_step(None).attention_precision == "fp32"
