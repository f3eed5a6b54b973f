"""Mixed-precision multi-style loss (csrc/style_f16.hip, mstg_hip/style_f16.py, style_loss.py precision="mixed").

Per kernel, teacher-forced (the method of tests/test_gpu_f16_train.py): the yardstick is torch on the CPU in float64 on the SAME
16-bit-rounded operands, so only the summation order and the one output rounding differ.  Bars: 2e-5 relative L2 for fp32 outputs
(the per-op fp32 bar), 2e-3 for fp16 outputs (the per-kernel fp16 bar), 8e-3 for bf16 outputs (the fp16 bar times the ratio of unit
roundoffs, 2^-9 / 2^-11).  Every kernel is launched twice and must give the same bits, under guard_helpers.memory_contract.

Whole loss: (2,3,32,32), width_div=4; yardstick oracle/restatement.py in float64 on the fp16-rounded weights; the device's loss,
four tap features and dL/dy must each lie within 2 x the distance the CPU emulation of the design (tests/style_f16_ref.py) has
from that yardstick.  Measured values are printed next to their bars."""
import pytest
import torch
import torch.nn.functional as F

import style_f16_ref as E
from conftest import rel_l2
from f16_helpers import DEV, _lib_loaded, report, rnd  # noqa: F401
from guard_helpers import memory_contract

pytestmark = pytest.mark.gpu

F16, BF16 = 0, 1
DT = {F16: torch.float16, BF16: torch.bfloat16}
BAR = {F16: 2e-3, BF16: 8e-3}
TAG = {F16: "f16", BF16: "bf16"}


def rd(t, dtype):
    """round to the 16-bit format and back (CPU, fp32)"""
    return t.to(DT[dtype]).float()


def up(t_nchw, dtype):
    """NCHW fp32 on the CPU -> NHWC 16-bit on the device"""
    return t_nchw.permute(0, 2, 3, 1).contiguous().to(DT[dtype]).to(DEV)


def nchw(t_nhwc):
    return t_nhwc.float().permute(0, 3, 1, 2)


def relu_mask(shape, seed):
    """an activation-like fp16 mask operand: about half its entries zero, some of them -0.0"""
    m = F.relu(rnd(shape, seed)).half()
    flat = m.view(-1)
    zeros = (flat == 0).nonzero().view(-1)
    flat[zeros[::3]] = -0.0
    assert 0.3 < float((m == 0).float().mean()) < 0.7
    assert bool((torch.signbit(m) & (m == 0)).any()) and bool((~torch.signbit(m) & (m == 0)).any())
    return m


CONV_CASES = [
    # name, N, H, W, Cin, Cout
    ("1x8x8 16->16 (less than one tile)", 1, 8, 8, 16, 16),
    ("3x8x8 16->32 (tiles span images)", 3, 8, 8, 16, 32),
    ("2x5x7 48->80 (odd sides, channels no power of two)", 2, 5, 7, 48, 80),
    ("2x4x4 512->512 (K = 4608)", 2, 4, 4, 512, 512),
    ("1x1x1 64->64 (all border)", 1, 1, 1, 64, 64),
    ("1x2x2 64->64 (all border)", 1, 2, 2, 64, 64),
]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv(case, dtype):
    """the layer itself (bias + ReLU) and the input-gradient form (flipped, transposed filter) without and with the ReLU mask"""
    from mstg_hip.style_f16 import PackedStyleConv
    name, N, H, W, Cin, Cout = case
    x = rd(rnd((N, Cin, H, W), 11), dtype)
    w = rnd((Cout, Cin, 3, 3), 12, (2.0 / (Cin * 9)) ** 0.5)
    b = rnd((Cout,), 13, 0.1)
    dz = rd(rnd((N, Cout, H, W), 14), dtype)
    mask = relu_mask((N, H, W, Cin), 15)
    ref = F.relu(F.conv2d(x.double(), rd(w, dtype).double(), b.double(), padding=1))
    ref_dx = F.conv_transpose2d(dz.double(), rd(w, dtype).double(), None, padding=1)
    with memory_contract(check_inputs=True) as mc:
        wd, bd = w.to(DEV), b.to(DEV)
        layer = PackedStyleConv(dtype, wd, bd, relu=1)
        xd = up(x, dtype)
        y, y2 = layer(xd), layer(xd)
        dgrad = PackedStyleConv(dtype, wd, None, flip=1)
        dzd, md = up(dz, dtype), mask.to(DEV)
        dx, dx2 = dgrad(dzd), dgrad(dzd)
        dxm, dxm2 = dgrad(dzd, md), dgrad(dzd, md)
        torch.cuda.synchronize()
    assert mc.outputs >= 8 and mc.uploads >= 5
    assert y.dtype == DT[dtype] and tuple(y.shape) == (N, H, W, Cout) and tuple(dx.shape) == (N, H, W, Cin)
    report(f"conv {TAG[dtype]} {name}", rel_l2(nchw(y), ref), BAR[dtype])
    report(f"input gradient {TAG[dtype]} {name}", rel_l2(nchw(dx), ref_dx), BAR[dtype])
    keep = (mask > 0).permute(0, 3, 1, 2)
    report(f"input gradient {TAG[dtype]} {name}, ReLU mask", rel_l2(nchw(dxm), ref_dx * keep), BAR[dtype])
    assert float(nchw(dxm).cpu()[~keep].abs().max()) == 0.0, "-0.0 and +0.0 both count as not > 0"
    for a, a2 in ((y, y2), (dx, dx2), (dxm, dxm2)):
        assert torch.equal(a.view(torch.int16), a2.view(torch.int16)), "two launches differ"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("Cw", [16, 64])
def test_stem_and_image_gradient(Cw, dtype):
    """3 -> Cw from the fp32 NCHW image (rounded while staging) and Cw -> 3 to the fp32 NCHW image gradient, at 2 x 16 x 24"""
    from mstg_hip.style_f16 import PackedStyleConv
    N, H, W = 2, 16, 24
    x = rnd((N, 3, H, W), 21).clamp(-1, 1)
    w = rnd((Cw, 3, 3, 3), 22, (2.0 / 27) ** 0.5)
    b = rnd((Cw,), 23, 0.1)
    dz = rd(rnd((N, Cw, H, W), 24), dtype)
    ref = F.relu(F.conv2d(rd(x, dtype).double(), rd(w, dtype).double(), b.double(), padding=1))
    ref_dx = F.conv_transpose2d(dz.double(), rd(w, dtype).double(), None, padding=1)
    with memory_contract(check_inputs=True) as mc:
        wd, bd = w.to(DEV), b.to(DEV)
        stem = PackedStyleConv(dtype, wd, bd, relu=1, stem=1)
        xd = x.to(DEV)
        y, y2 = stem(xd), stem(xd)
        grad = PackedStyleConv(dtype, wd, None, image_grad=1, flip=1)
        dzd = up(dz, dtype)
        dx, dx2 = grad(dzd), grad(dzd)
        torch.cuda.synchronize()
    assert mc.outputs >= 6
    assert y.dtype == DT[dtype] and tuple(y.shape) == (N, H, W, Cw)
    assert dx.dtype == torch.float32 and tuple(dx.shape) == (N, 3, H, W)
    report(f"stem {TAG[dtype]} 3->{Cw}", rel_l2(nchw(y), ref), BAR[dtype])
    report(f"image gradient {TAG[dtype]} {Cw}->3 (fp32 out)", rel_l2(dx, ref_dx), 2e-5)
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)) and torch.equal(dx, dx2), "two launches differ"


def planted_ties(shape, seed):
    """fp16 NCHW values with ties planted in every window position: all four equal, each pair equal (as the maximum), and zeros"""
    x = rnd(shape, seed).half()
    N, C_, H, W = shape
    pats = [(0, 1, 2, 3), (0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (1, 2, 3), (0, 2, 3)]
    k = 0
    for n in range(N):
        for oy in range(H // 2):
            for ox in range(W // 2):
                for c in range(0, C_, 5):
                    pat = pats[k % len(pats)]
                    k += 1
                    for s in pat:
                        x[n, c, 2 * oy + (s >> 1), 2 * ox + (s & 1)] = 8.0 if k % 2 else 0.0
                    if k % 2 == 0:  # zeros tie as the maximum only when the rest is negative
                        for s in set(range(4)) - set(pat):
                            x[n, c, 2 * oy + (s >> 1), 2 * ox + (s & 1)] = -1.0
    return x


@pytest.mark.parametrize("shape", [(2, 16, 8, 8), (1, 48, 6, 10)], ids=["2x8x8x16", "1x6x10x48"])
def test_maxpool_forward_and_backward_are_bit_equal_to_torch(shape):
    from mstg_hip import style_f16
    N, C_, H, W = shape
    x = planted_ties(shape, 31)
    ref, ridx = F.max_pool2d(x.float(), 2, return_indices=True)
    oy = torch.arange(H // 2).view(1, 1, -1, 1)
    ox = torch.arange(W // 2).view(1, 1, 1, -1)
    slot = ((ridx // W - 2 * oy) * 2 + (ridx % W - 2 * ox)).to(torch.uint8)
    assert all(int((slot == s).sum()) > 0 for s in range(4))
    dy = rnd((N, C_, H // 2, W // 2), 32).bfloat16()
    want = F.max_unpool2d(dy.float(), ridx, 2, output_size=(H, W)).bfloat16()
    want_m = (want.float() * (x > 0)).bfloat16()
    with memory_contract(check_inputs=True):
        xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
        y, idx = style_f16.maxpool_fwd(xd)
        y2, idx2 = style_f16.maxpool_fwd(xd)
        dyd = dy.permute(0, 2, 3, 1).contiguous().to(DEV)
        dx, dx2 = style_f16.maxpool_bwd(dyd, idx), style_f16.maxpool_bwd(dyd, idx)
        dxm, dxm2 = style_f16.maxpool_bwd(dyd, idx, xd), style_f16.maxpool_bwd(dyd, idx, xd)
        torch.cuda.synchronize()
    assert torch.equal(y.cpu().permute(0, 3, 1, 2), ref.half()), "values"
    assert torch.equal(idx.cpu().permute(0, 3, 1, 2), slot), "arg-max slots (first maximum in window order)"
    bits = lambda t: t.contiguous().view(torch.int16)  # noqa: E731
    # a routed zero and an unrouted position are both zero; compare values, and bits where the gradient was routed
    got, got_m = dx.cpu().permute(0, 3, 1, 2), dxm.cpu().permute(0, 3, 1, 2)
    assert torch.equal(got.float(), want.float()) and torch.equal(got_m.float(), want_m.float())
    routed = F.max_unpool2d(torch.ones_like(dy).float(), ridx, 2, output_size=(H, W)) > 0
    assert torch.equal(bits(got)[routed], bits(want)[routed])
    assert torch.equal(bits(y), bits(y2)) and torch.equal(idx, idx2) and torch.equal(bits(dx), bits(dx2)) and torch.equal(bits(dxm), bits(dxm2))


GRAM_CASES = [(2, 64, 64, 64), (1, 24, 40, 48), (2, 2, 2, 512)]
GRAM_IDS = ["2x64x64 C64", "1x24x40 C48", "2x2x2 C512"]


def gram_feature(N, H, W, C_, seed):
    return F.relu(rnd((N, H, W, C_), seed) + 0.2).half()


@pytest.mark.parametrize("shape", GRAM_CASES, ids=GRAM_IDS)
def test_gram_forward(shape):
    from mstg_hip import style_f16
    N, H, W, C_ = shape
    f = gram_feature(N, H, W, C_, 41)
    m = f.double().reshape(N, H * W, C_)
    ref = torch.bmm(m.transpose(1, 2), m) / (C_ * H * W)
    with memory_contract(check_inputs=True) as mc:
        fd = f.to(DEV)
        g, g2 = style_f16.gram_fwd(fd), style_f16.gram_fwd(fd)
        torch.cuda.synchronize()
    assert mc.workspaces == 2 and g.dtype == torch.float32 and tuple(g.shape) == (N, C_, C_)
    report(f"gram forward {shape}", rel_l2(g, ref), 2e-5)
    assert torch.equal(g, g2), "two launches differ"


# the backward takes 256-pixel blocks once they give 512 workgroups: the smallest shapes that do, one with a ragged last block
# (65500 pixels = 255 blocks + 220 pixels = 13 fragments + 12) and two channel tiles
GRAM_BWD_CASES = GRAM_CASES + [(2, 256, 256, 64), (1, 250, 262, 128)]
GRAM_BWD_IDS = GRAM_IDS + ["2x256x256 C64 (256-pixel blocks)", "1x250x262 C128 (256-pixel blocks, ragged)"]


@pytest.mark.parametrize("with_incoming", [False, True], ids=["alone", "plus incoming"])
@pytest.mark.parametrize("shape", GRAM_BWD_CASES, ids=GRAM_BWD_IDS)
def test_gram_backward(shape, with_incoming):
    from mstg_hip import style_f16
    N, H, W, C_ = shape
    f = gram_feature(N, H, W, C_, 42)
    dg = rnd((N, C_, C_), 43, 1e-6)  # not symmetric: the kernel symmetrises
    scale = 1.0 / (C_ * H * W)
    m = f.double().reshape(N, H * W, C_)
    ref = scale * torch.bmm(m, dg.double() + dg.double().transpose(1, 2)).reshape(N, H, W, C_)
    inc = None
    if with_incoming:  # of the product's own size, so that neither term hides the other
        inc = (rnd((N, H, W, C_), 44) * float(ref.abs().mean())).bfloat16()
        ref = ref + inc.double()
    ref = ref * (f > 0)
    with memory_contract(check_inputs=True) as mc:
        fd, dgd = f.to(DEV), dg.to(DEV)
        incd = None if inc is None else inc.to(DEV)
        df, df2 = style_f16.gram_bwd(fd, dgd, incd), style_f16.gram_bwd(fd, dgd, incd)
        torch.cuda.synchronize()
    assert mc.workspaces == 2 and df.dtype == torch.bfloat16 and tuple(df.shape) == (N, H, W, C_)
    report(f"gram backward {shape} {'+ incoming' if with_incoming else ''}", rel_l2(df.float(), ref), 8e-3)
    assert float(df.float().cpu()[f <= 0].abs().max()) == 0.0
    assert torch.equal(df.view(torch.int16), df2.view(torch.int16)), "two launches differ"


@pytest.mark.parametrize("shape", GRAM_BWD_CASES[:4], ids=GRAM_BWD_IDS[:4])
def test_gram_backward_has_no_fp16_intermediate(shape):
    """dG and dG * 2^-40: the second result is the first times 2^-40 EXACTLY.  Everything stays far above fp32's and bf16's
    subnormals (dG ~ 1e-6 * 2^-40 ~ 1e-18; the bf16 tail of it 2^-8 of that); an fp16 intermediate anywhere flushes."""
    from mstg_hip import style_f16
    N, H, W, C_ = shape
    f = gram_feature(N, H, W, C_, 45)
    dg = rnd((N, C_, C_), 46, 1e-6)
    inc = (rnd((N, H, W, C_), 47) * 1e-9).bfloat16()
    k = 2.0 ** -40
    with memory_contract(check_inputs=True):
        fd = f.to(DEV)
        a = style_f16.gram_bwd(fd, dg.to(DEV))
        b = style_f16.gram_bwd(fd, (dg * k).to(DEV))
        ai = style_f16.gram_bwd(fd, dg.to(DEV), inc.to(DEV))
        bi = style_f16.gram_bwd(fd, (dg * k).to(DEV), (inc.float() * k).bfloat16().to(DEV))
        torch.cuda.synchronize()
    assert float(a.float().abs().max()) > 0.0
    print(f"  [range] {shape}: largest |dF| {float(a.float().abs().max()):.2e}, scaled {float(b.float().abs().max()):.2e}")
    assert torch.equal(b.float(), a.float() * k)
    assert torch.equal(bi.float(), ai.float() * k)


# ---- whole loss --------------------------------------------------------------------------------------------------------------------
_REF = {}


def whole_loss_reference():
    """computed once, shared, never modified: inputs, the float64 yardstick on fp16-rounded weights, the emulation, the bars"""
    if not _REF:
        sd, y, styles = E.loss_inputs()
        yard = E.yardstick(E.rounded_weights(sd), y, styles, E.WEIGHTS3)
        yard32 = E.yardstick(sd, y, styles, E.WEIGHTS3)
        emu = E.emulate(sd, y, styles, E.WEIGHTS3)
        dist = {"loss": abs(float(emu["loss"]) - float(yard["loss"])) / float(yard["loss"]), "dy": rel_l2(emu["dy"], yard["dy"]),
                "feats": [rel_l2(a, b) for a, b in zip(emu["feats"], yard["feats"])]}
        _REF.update(sd=sd, y=y, styles=styles, yard=yard, yard32=yard32, emu=emu, dist=dist)
    return _REF


def mixed_loss(sd, styles, weights):
    import style_loss as sl
    feats = sl.VGGFeatures(width_div=E.WIDTH_DIV, precision="mixed")
    feats.load_state_dict(sd)
    feats.to(DEV)
    return sl.MultiStyleGramLoss(feats, [s.to(DEV) for s in styles], weights, precision="mixed")


def test_whole_loss_against_the_emulation():
    """Measured on the MI355X (device distance from the float64 yardstick / the emulation's own / bar = 2 x emulation): see DESIGN.md,
    "Mixed-precision multi-style loss"."""
    from mstg_hip import ops, style_f16
    r = whole_loss_reference()
    yard, dist = r["yard"], r["dist"]
    mod = mixed_loss(r["sd"], r["styles"], E.WEIGHTS3)
    y = r["y"].to(DEV).requires_grad_(True)
    loss = mod(y)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and "MixedStyleLossFn" in type(loss.grad_fn).__name__
    loss.backward()
    assert y.grad.dtype == torch.float32 and y.grad.shape == y.shape and bool(torch.isfinite(y.grad).all())
    print(f"  weight rounding alone (fp32 weights vs fp16-rounded, float64, no bar): loss {abs(float(r['yard32']['loss']) - float(yard['loss'])) / float(yard['loss']):.2e}, "
          f"dL/dy {rel_l2(r['yard32']['dy'], yard['dy']):.2e}")
    print(f"  loss: device {float(loss):.9e}  float64 {float(yard['loss']):.9e}  emulation {float(r['emu']['loss']):.9e}")
    with torch.no_grad():
        feats = mod.features(y.detach())
    assert all(f.dtype == torch.float16 for f in feats)
    errs = {"loss": abs(float(loss) - float(yard["loss"])) / float(yard["loss"]), "dy": rel_l2(y.grad, yard["dy"]),
            "feats": [rel_l2(nchw(f), ref) for f, ref in zip(feats, yard["feats"])]}
    for l in range(4):
        print(f"  [whole] tap {l}: device {errs['feats'][l]:.3e}  emulation {dist['feats'][l]:.3e}  bar {2 * dist['feats'][l]:.3e}")
    print(f"  [whole] loss : device {errs['loss']:.3e}  emulation {dist['loss']:.3e}  bar {2 * dist['loss']:.3e}")
    print(f"  [whole] dL/dy: device {errs['dy']:.3e}  emulation {dist['dy']:.3e}  bar {2 * dist['dy']:.3e}; largest entry {float(y.grad.abs().max()):.2e}")
    # a second forward + backward gives the same bits; its launches are counted
    y2 = r["y"].to(DEV).requires_grad_(True)
    ops.KernelTimer.start()
    try:
        loss2 = mod(y2)
        loss2.backward()
        torch.cuda.synchronize()
        kernels = ops.KernelTimer.kernels()
    finally:
        ops.KernelTimer.stop()
    print(f"  launches of one loss forward + backward: {len(kernels)} (design: {style_f16.LAUNCHES_FWD} + {style_f16.LAUNCHES_BWD})")
    assert len(kernels) == style_f16.LAUNCHES_FWD + style_f16.LAUNCHES_BWD, [k for k, _ in kernels]
    assert torch.equal(loss2, loss) and torch.equal(y2.grad, y.grad), "two runs differ"
    for l in range(4):
        assert errs["feats"][l] <= 2 * dist["feats"][l], (l, errs["feats"][l], dist["feats"][l])
    assert errs["loss"] <= 2 * dist["loss"], (errs["loss"], dist["loss"])
    assert errs["dy"] <= 2 * dist["dy"], (errs["dy"], dist["dy"])


def test_a_style_scored_against_itself_is_exactly_zero():
    r = whole_loss_reference()
    ref = r["styles"][1][:1].contiguous()
    mod = mixed_loss(r["sd"], [ref], (1.0,))
    y = ref.to(DEV).requires_grad_(True)
    loss = mod(y)
    loss.backward()
    assert float(loss) == 0.0
    assert float(y.grad.abs().max()) == 0.0
    # and not because everything is zero
    other = r["styles"][2][:1].contiguous().to(DEV).requires_grad_(True)
    lo = mod(other)
    lo.backward()
    assert float(lo) > 0.0 and float(other.grad.abs().max()) > 0.0


def test_packs_follow_the_weights():
    """load_state_dict and an in-place write re-pack: the features equal those of a stack built with the new weights"""
    import style_loss as sl
    r = whole_loss_reference()
    y = r["y"].to(DEV)
    sd2 = E.R.make_state_dict(E.R.vgg_spec(E.WIDTH_DIV), 78)

    def fresh(sd):
        f = sl.VGGFeatures(width_div=E.WIDTH_DIV, precision="mixed")
        f.load_state_dict(sd)
        return f.to(DEV)

    a, b = fresh(r["sd"]), fresh(sd2)
    fa, fb = a(y), b(y)
    assert not torch.equal(fa[0], fb[0])
    a.load_state_dict(sd2)
    for u, v in zip(a(y), fb):
        assert torch.equal(u, v)
    with torch.no_grad():
        a.conv3.weight.mul_(0.5)
        b.conv3.weight.mul_(0.5)
    changed = a(y)
    for u, v in zip(changed, b(y)):
        assert torch.equal(u, v)
    assert torch.equal(changed[0], fb[0]) and not torch.equal(changed[1], fb[1])  # conv3 feeds taps 1..3 only
