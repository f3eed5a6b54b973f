"""Mixed-precision pre-training step of the plain Generator (csrc/train_f16_plain.hip, mstg_hip/train_plain.py,
pretrain.PretrainStep(amp=True)).

Per kernel, teacher-forced: the yardstick is torch on the CPU evaluated on the SAME fp16-rounded operands (in fp64 where the
checked output is fp32, so that the yardstick's own summation error over up to 32 768 pixels does not eat the bar), so only the
summation order and the one output rounding differ.  Bars: 2e-5 relative L2 for fp32 outputs (the per-op fp32 bar of
tests/test_gpu_ops.py), 2e-3 for fp16 outputs (the per-kernel fp16 bar of tests/test_gpu_f16_plain.py).  Every kernel is launched
twice and must give the same bits.

Whole step: against the committed reference vectors (tests/golden/pretrain_amp_c8_64x64.npz, tools/make_pretrain_amp_golden.py):
the whole parameter gradient within 2 x the distance the reference itself has under autocast on the same draw, every parameter
tensor within 0.3 of its fp64 gradient (a cap that separates error classes -- a lost, doubled, mis-scaled or sign-flipped tensor
sits at >= 0.5 -- not a precision claim), the six biases in front of a BatchNorm exactly zero, the loss within 2^-11.
Measured values are printed next to their bars."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD, ROOT, rel_l2
from f16_helpers import (ACT_LEAKY02, ACT_NONE, ACT_RELU, DEV, LAYER_CASES, STEM_HEAD_CASES, _lib_loaded, h, nhwc16, report,  # noqa: F401
                         rnd)

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
ACTS = {ACT_NONE: lambda t: t, ACT_RELU: F.relu, ACT_LEAKY02: lambda t: F.leaky_relu(t, 0.2)}


def state(scale=4.0):
    from mstg_hip import train_plain
    return train_plain.make_state(scale, DEV)


# ---- weight gradient ------------------------------------------------------------------------------------------------------------
def conv_transpose_weight_grad(x, dz):
    """dW (Cin, Cout, 4, 4) of ConvTranspose2d(k4,s2,p1) from autograd, in the dtype of the operands."""
    w = torch.zeros((x.shape[1], dz.shape[1], 4, 4), dtype=x.dtype, requires_grad=True)
    F.conv_transpose2d(x, w, None, 2, 1).backward(dz)
    return w.grad


@pytest.mark.parametrize("case", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_wgrad_layer(case):
    from mstg_hip import train_plain
    name, kind, N, H, W, Cin, Cout, _ = case
    x = rnd((N, Cin, H, W), 11) * 1.5 + 0.3
    dz = rnd((N, Cout, 2 * H, 2 * W) if kind == 1 else (N, Cout, H // 2, W // 2), 12)
    fstate, _ = state(4.0)
    if kind == 1:
        S, B, shape = nhwc16(x), nhwc16(dz), (Cin, Cout, 4, 4)
        ref = conv_transpose_weight_grad(h(x).double(), h(dz).double())
    else:
        S, B, shape = nhwc16(dz), nhwc16(x), (Cout, Cin, 4, 4)
        ref = torch.nn.grad.conv2d_weight(h(x).double(), shape, h(dz).double(), stride=2, padding=1)
    dW = train_plain.wgrad(S, B, shape[1], fstate, torch.full(shape, 7.0, device=DEV))
    dW2 = train_plain.wgrad(S, B, shape[1], fstate, torch.empty(shape, device=DEV))
    report("wgrad " + name, rel_l2(dW, ref / 4.0), 2e-5)
    assert torch.equal(dW, dW2), "two launches differ"


@pytest.mark.parametrize("case", STEM_HEAD_CASES, ids=[c[0] for c in STEM_HEAD_CASES])
def test_wgrad_stem_and_head(case):
    from mstg_hip import train_plain
    name, N, H, W, Cw = case
    fstate, _ = state(4.0)
    # stem: Conv2d(3, C): the fp32 image is read as fp16 NHWC padded to 8 channels
    x = rnd((N, 3, H, W), 13).clamp(-1, 1)
    dz = rnd((N, Cw, H // 2, W // 2), 14)
    x8 = train_plain.image_nhwc8(x.to(DEV))
    assert tuple(x8.shape) == (N, H, W, 8) and torch.equal(x8[..., :3].cpu(), h(x).permute(0, 2, 3, 1).half()) and float(x8[..., 3:].abs().max()) == 0.0
    ref = torch.nn.grad.conv2d_weight(h(x).double(), (Cw, 3, 4, 4), h(dz).double(), stride=2, padding=1)
    dW = train_plain.wgrad(nhwc16(dz), x8, 3, fstate, torch.empty((Cw, 3, 4, 4), device=DEV))
    dW2 = train_plain.wgrad(nhwc16(dz), x8, 3, fstate, torch.empty((Cw, 3, 4, 4), device=DEV))
    report("wgrad stem " + name, rel_l2(dW, ref / 4.0), 2e-5)
    assert torch.equal(dW, dW2)
    # head: ConvTranspose2d(C, 3): the gradient of the image is NHWC padded to 8 channels
    a = F.relu(rnd((N, Cw, H // 2, W // 2), 15))
    dzh = rnd((N, 3, H, W), 16, 0.5)
    ref = conv_transpose_weight_grad(h(a).double(), h(dzh).double())
    dzh8 = train_plain.image_nhwc8(dzh.to(DEV))
    dW = train_plain.wgrad(nhwc16(a), dzh8, 3, fstate, torch.empty((Cw, 3, 4, 4), device=DEV))
    dW2 = train_plain.wgrad(nhwc16(a), dzh8, 3, fstate, torch.empty((Cw, 3, 4, 4), device=DEV))
    report("wgrad head " + name, rel_l2(dW, ref / 4.0), 2e-5)
    assert torch.equal(dW, dW2)
    # their bias gradients
    db = train_plain.bias_grad(nhwc16(dz), Cw, fstate, torch.empty(Cw, device=DEV))
    report("bias grad stem " + name, rel_l2(db, h(dz).double().sum(dim=(0, 2, 3)) / 4.0), 2e-5)
    db3 = train_plain.bias_grad(dzh8, 3, fstate, torch.empty(3, device=DEV))
    report("bias grad head " + name, rel_l2(db3, h(dzh).double().sum(dim=(0, 2, 3)) / 4.0), 2e-5)
    assert torch.equal(db3, train_plain.bias_grad(dzh8, 3, fstate, torch.empty(3, device=DEV)))


# ---- input gradient through the opposite-kind pack ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_dgrad_is_the_opposite_kind_on_the_same_weight(case):
    from mstg_hip.infer_plain import PackedPlainConv
    name, kind, N, H, W, Cin, Cout, _ = case
    taps = 4 if kind == 1 else 16
    w = rnd((Cin, Cout, 4, 4) if kind == 1 else (Cout, Cin, 4, 4), 21, (2.0 / (Cin * taps)) ** 0.5)
    dz = rnd((N, Cout, 2 * H, 2 * W) if kind == 1 else (N, Cout, H // 2, W // 2), 22)
    x = torch.zeros((N, Cin, H, W), requires_grad=True)
    (F.conv_transpose2d if kind == 1 else F.conv2d)(x, h(w), None, 2, 1).backward(h(dz))
    pc = PackedPlainConv(1 - kind, w.to(DEV), None, None, ACT_NONE)
    dx = pc(nhwc16(dz))
    assert tuple(dx.shape) == (N, H, W, Cin)
    report("dgrad " + name, rel_l2(dx.float().permute(0, 3, 1, 2), x.grad), 2e-3)
    assert torch.equal(dx, pc(nhwc16(dz)))


def test_dgrad_of_the_head_through_the_padded_pack():
    from mstg_hip import train_plain
    from mstg_hip.infer_plain import PackedPlainConv
    N, H, W, Cw = 2, 16, 24, 16
    w = rnd((Cw, 3, 4, 4), 23, (2.0 / (Cw * 4)) ** 0.5)
    dz = rnd((N, 3, 2 * H, 2 * W), 24, 0.5)
    x = torch.zeros((N, Cw, H, W), requires_grad=True)
    F.conv_transpose2d(x, h(w), None, 2, 1).backward(h(dz))
    wpad = torch.zeros((Cw, 8, 4, 4))
    wpad[:, :3] = w
    dx = PackedPlainConv(0, wpad.to(DEV), None, None, ACT_NONE)(train_plain.image_nhwc8(dz.to(DEV)))
    report("dgrad head (3 channels padded to 8)", rel_l2(dx.float().permute(0, 3, 1, 2), x.grad), 2e-3)


# ---- BatchNorm in training mode ----------------------------------------------------------------------------------------------------
BN_CASES = [
    # name, N, H, W, C, act, wide
    ("8 ch leaky", 2, 16, 16, 8, ACT_LEAKY02, False),
    ("64 ch relu", 4, 8, 8, 64, ACT_RELU, False),
    ("24 ch leaky (other multiples of 8)", 3, 6, 10, 24, ACT_LEAKY02, False),
    ("512 ch relu, 8 values per channel", 2, 2, 2, 512, ACT_RELU, False),
    ("64 ch leaky, 32768 pixels", 8, 64, 64, 64, ACT_LEAKY02, False),
    ("32 ch none, wide range (means to +-8, std 0.05 to 4)", 4, 32, 32, 32, ACT_NONE, True),
    ("128 ch relu, wide range", 2, 16, 16, 128, ACT_RELU, True),
]


def bn_inputs(N, H, W, C_, wide):
    z = rnd((N, C_, H, W), 31)
    if wide:
        g = torch.Generator().manual_seed(32)
        std = torch.exp(torch.empty(C_).uniform_(float(np.log(0.05)), float(np.log(4.0)), generator=g))
        mean = torch.empty(C_).uniform_(-8.0, 8.0, generator=g)
        std[0], std[1], mean[0], mean[1] = 0.05, 4.0, 8.0, -8.0
        z = z * std[None, :, None, None] + mean[None, :, None, None]
    else:
        z = z * 1.3 + 0.2
    gamma = 1.0 + 0.3 * rnd((C_,), 33)
    beta = 0.2 * rnd((C_,), 34)
    dy = rnd((N, C_, H, W), 35)
    return h(z), gamma, beta, h(dy)


@pytest.mark.parametrize("case", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_batchnorm_training_forward_and_backward(case):
    from mstg_hip import train_plain
    name, N, H, W, C_, act, wide = case
    z, gamma, beta, dy = bn_inputs(N, H, W, C_, wide)
    bn = torch.nn.BatchNorm2d(C_).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(0.1 * rnd((C_,), 36))
        bn.running_var.copy_(0.5 + torch.rand(C_, generator=torch.Generator().manual_seed(37)))
    rm, rv = bn.running_mean.float().to(DEV), bn.running_var.float().to(DEV)
    zd = z.double().requires_grad_(True)
    y_ref = ACTS[act](bn(zd))
    y_ref.backward(dy.double())
    mean_ref = z.double().mean(dim=(0, 2, 3))
    rstd_ref = torch.rsqrt(z.double().var(dim=(0, 2, 3), unbiased=False) + 1e-5)

    z_d, dy_d, g_d, b_d = nhwc16(z), nhwc16(dy), gamma.to(DEV), beta.to(DEV)
    y, mean, rstd = train_plain.bn_fwd(z_d, g_d, b_d, rm, rv, act)
    report(f"bn {name}: y", rel_l2(y.float().permute(0, 3, 1, 2), y_ref), 2e-3)
    report(f"bn {name}: batch mean", rel_l2(mean, mean_ref), 2e-5)
    report(f"bn {name}: batch rstd", rel_l2(rstd, rstd_ref), 2e-5)
    report(f"bn {name}: running_mean after 1 call", rel_l2(rm, bn.running_mean), 2e-5)
    report(f"bn {name}: running_var after 1 call", rel_l2(rv, bn.running_var), 2e-5)
    rm2, rv2 = rm.clone(), rv.clone()
    for _ in range(2):
        bn(z.double())
        y2, mean2, rstd2 = train_plain.bn_fwd(z_d, g_d, b_d, rm, rv, act)
    report(f"bn {name}: running_mean after 3 calls", rel_l2(rm, bn.running_mean), 2e-5)
    report(f"bn {name}: running_var after 3 calls", rel_l2(rv, bn.running_var), 2e-5)
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2), "two launches differ"
    assert not torch.equal(rm, rm2) and not torch.equal(rv, rv2)

    fstate, _ = state(4.0)
    dgamma, dbeta = torch.empty(C_, device=DEV), torch.empty(C_, device=DEV)
    dz = train_plain.bn_bwd(z_d, dy_d, g_d, b_d, mean, rstd, act, fstate, dgamma, dbeta)
    report(f"bn {name}: dz", rel_l2(dz.float().permute(0, 3, 1, 2), zd.grad), 2e-3)
    report(f"bn {name}: dgamma", rel_l2(dgamma, bn.weight.grad / 4.0), 2e-5)
    report(f"bn {name}: dbeta", rel_l2(dbeta, bn.bias.grad / 4.0), 2e-5)
    dgamma2, dbeta2 = torch.empty(C_, device=DEV), torch.empty(C_, device=DEV)
    dz2 = train_plain.bn_bwd(z_d, dy_d, g_d, b_d, mean, rstd, act, fstate, dgamma2, dbeta2)
    assert torch.equal(dz, dz2) and torch.equal(dgamma, dgamma2) and torch.equal(dbeta, dbeta2), "two launches differ"


def test_head_loss_and_its_gradient():
    """loss = mean |y k - real k| in fp32 on the fp16 image; dz = scale / numel * sign * k * (1 - y^2), one rounding to fp16."""
    from mstg_hip import train_plain
    N, H, W = 3, 32, 48
    y = h(torch.tanh(rnd((N, 3, H, W), 41)))
    real = rnd((N, 3, H, W), 42).clamp(-1, 1)
    m = (torch.rand((N, 1, H // 8, W // 8), generator=torch.Generator().manual_seed(43)) < 0.4).float()
    m = m.repeat_interleave(8, 2).repeat_interleave(8, 3).expand(N, 3, H, W).contiguous()
    scale = 65536.0
    fstate, _ = state(scale)
    loss, dz = train_plain.head_loss_bwd(y.half().to(DEV), real.to(DEV), m.to(DEV), fstate)
    k = (1 - m).double()
    d = y.double() * k - real.double() * k
    report("masked L1 loss", abs(float(loss) - float(d.abs().mean())) / float(d.abs().mean()), 2e-5)
    ref = scale / y.numel() * torch.sign(d) * k * (1 - y.double() ** 2)
    report("gradient at the head's pre-activation", rel_l2(dz[..., :3].float().permute(0, 3, 1, 2), ref), 2e-3)
    assert float(dz[..., 3:].abs().max()) == 0.0
    loss2, dz2 = train_plain.head_loss_bwd(y.half().to(DEV), real.to(DEV), m.to(DEV), fstate)
    assert torch.equal(loss, loss2) and torch.equal(dz, dz2)


def test_stem_activation_backward():
    from mstg_hip import train_plain
    a = h(F.leaky_relu(rnd((2, 16, 16, 8), 44), 0.2))
    da = h(rnd((2, 16, 16, 8), 45))
    dz = train_plain.act_bwd(a.half().to(DEV), da.half().to(DEV), ACT_LEAKY02)
    report("LeakyReLU backward from the output", rel_l2(dz.float(), da * torch.where(a > 0, 1.0, 0.2)), 2e-3)


# ---- whole step ----------------------------------------------------------------------------------------------------------------------
def make_step(sd, amp, loss_scale="auto", max_norm=1e9, channels=8):
    """A Generator with ``sd`` in training mode on the GPU and its PretrainStep.  max_norm = 1e9: clip_grad_norm_ multiplies by
    exactly 1, so the flat gradient buffer still holds the un-clipped gradient after the step."""
    import plain_generator
    import pretrain
    gen = plain_generator.Generator(channels)
    gen.load_state_dict(sd)
    gen.to(DEV).train()
    kw = {"amp": True, "loss_scale": loss_scale} if amp else {}
    return gen, pretrain.PretrainStep(gen, max_norm=max_norm, **kw)


def grads_of(gen):
    return {k: p.grad.detach().double().cpu() for k, p in gen.named_parameters()}


GOLDEN_DISTANCES = {}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_step_against_the_reference(seed):
    """Measured on the MI355X, loss_scale="auto" (whole-gradient distance from fp64 / the reference's own under autocast on the
    same draw / ratio; worst parameter tensor; |loss - fp64 loss|):
      seed 1: 0.0323 / 0.0329 / 0.98; encoder.0.bias 0.0929; 3.0e-06
      seed 2: 0.0444 / 0.0364 / 1.22; encoder.6.bias 0.0742; 2.5e-06
      seed 3: 0.0484 / 0.0558 / 0.87; encoder.0.bias 0.1312; 2.8e-06"""
    import emulate_plain_f16_train as E
    z = np.load(os.path.join(GOLD, "pretrain_amp_c8_64x64.npz"))
    C_, (N, _, S, _) = int(z["C"]), z["shape"]
    sd, x, real, m = E.pretrain_draw(C_, int(N), int(S), seed)
    assert np.array_equal(m.numpy().astype(np.uint8), z[f"s{seed}_mask"])
    gen, step = make_step(sd, True)
    loss = step(x.to(DEV), real.to(DEV), m.to(DEV))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    assert step.loss_scale == 65536.0 and step.skipped_steps == 0 and step.optimizer.step_count == 1
    g = grads_of(gen)
    names = list(g)
    ref = {k: torch.from_numpy(z[f"s{seed}_g64_{k}"]).double() for k in names}
    l64 = float(z[f"s{seed}_loss64"])
    print(f"  seed {seed}: loss {float(loss):.8f}  fp64 {l64:.8f}  |difference| {abs(float(loss) - l64):.2e} (bound 2^-11 = {2.0 ** -11:.2e}); "
          f"reference under autocast {float(z[f's{seed}_loss_amp']) - l64:+.2e}")
    assert abs(float(loss) - l64) <= 2.0 ** -11
    whole, amp = E.distance(g, ref, names), float(z[f"s{seed}_amp_dist"])
    print(f"  seed {seed}: whole gradient distance from fp64 {whole:.4f}; reference under autocast {amp:.4f}; ratio {whole / amp:.2f} (bar 2)")
    worst = ("", 0.0)
    for k in names:
        if k in E.DEAD_BIASES:
            assert float(g[k].abs().max()) == 0.0, f"{k}: a bias in front of a BatchNorm must get an exactly zero gradient"
            continue
        dk = float((g[k] - ref[k]).norm() / ref[k].norm())
        print(f"    {k:20s} distance {dk:.4f} (cap 0.3; reference under autocast {float(z[f's{seed}_amp_dist_{k}']):.4f})")
        worst = max(worst, (k, dk), key=lambda t: t[1])
        assert dk <= 0.3, f"{k}: {dk:.3f} > 0.3"
    print(f"  seed {seed}: worst tensor {worst[0]} {worst[1]:.4f}")
    assert whole <= 2.0 * amp, f"seed {seed}: {whole:.4f} > 2 x {amp:.4f}"


def test_loss_scaling_earns_its_place():
    """16 x 3 x 256 x 256, channels 8, seed 7 (tools/emulate_plain_f16_train.py::LOSS_SCALE_DRAW).  Yardstick: this build's fp32
    PretrainStep gradient on the same weights and batch.  The CPU emulation of the design gives, against fp64 on this draw,
    5.9027e-03 with loss_scale="auto" and 3.3632e-02 with loss_scale=1 (python tools/emulate_plain_f16_train.py), so the bar for
    "auto" is 2 x 5.9027e-03 = 1.18e-02; loss_scale=1 must be at least 3 x worse than "auto".  Measured on the MI355X: "auto"
    5.9733e-03, loss_scale=1 3.2079e-02 (5.4 x)."""
    import emulate_plain_f16_train as E
    EMULATED_AUTO = 5.9027e-03
    C_, N, S, seed = E.LOSS_SCALE_DRAW
    sd, x, real, m = E.pretrain_draw(C_, N, S, seed)
    xd, rd, md = x.to(DEV), real.to(DEV), m.to(DEV)
    gen32, step32 = make_step(sd, False)
    step32(xd, rd, md)
    ref = grads_of(gen32)
    names = list(ref)
    dist = {}
    for tag, scale in (("auto", "auto"), ("1", 1.0)):
        gen, step = make_step(sd, True, scale)
        step(xd, rd, md)
        assert step.skipped_steps == 0
        dist[tag] = E.distance(grads_of(gen), ref, names)
        if tag == "auto":
            assert step.loss_scale == 2.0 ** 22
    print(f"  distance from the fp32 step's gradient: loss_scale='auto' {dist['auto']:.4e} (bar 2 x emulation {EMULATED_AUTO:.4e} = "
          f"{2 * EMULATED_AUTO:.4e}); loss_scale=1 {dist['1']:.4e} = {dist['1'] / dist['auto']:.1f} x auto (bar >= 3 x)")
    assert dist["auto"] <= 2 * EMULATED_AUTO
    assert dist["1"] >= 3 * dist["auto"]


def test_non_finite_gradient_skips_the_step_and_halves_the_scale():
    """loss_scale = 2^40 overflows fp16 to inf -- arithmetic, not a fault: the step must leave parameters and Adam state alone."""
    import emulate_plain_f16_train as E
    sd, x, real, m = E.pretrain_draw(8, 2, 32, 5)
    gen, step = make_step(sd, True, 2.0 ** 40, max_norm=1.0)
    before = {k: v.detach().clone() for k, v in gen.state_dict().items() if "running" not in k and "num_batches" not in k}
    loss = step(x.to(DEV), real.to(DEV), m.to(DEV))
    assert np.isfinite(float(loss)) and not np.isfinite(float(step.last_grad_norm))
    for k, v in before.items():
        assert torch.equal(v, gen.state_dict()[k]), k
    assert float(step.optimizer.exp_avg.abs().max()) == 0.0 and float(step.optimizer.exp_avg_sq.abs().max()) == 0.0
    assert step.optimizer.step_count == 0 and step.skipped_steps == 1 and step.loss_scale == 2.0 ** 39
    step.loss_scale = 4096.0
    step(x.to(DEV), real.to(DEV), m.to(DEV))
    assert np.isfinite(float(step.last_grad_norm)) and step.optimizer.step_count == 1 and step.skipped_steps == 1 and step.loss_scale == 4096.0
    changed = [k for k, v in before.items() if not torch.equal(v, gen.state_dict()[k])]
    assert "encoder.0.weight" in changed and "decoder.9.weight" in changed and "encoder.6.weight" in changed
    assert float(step.optimizer.exp_avg.abs().max()) > 0.0


def run_three_steps(amp):
    import emulate_plain_f16_train as E
    sd, _, _, _ = E.pretrain_draw(8, 2, 64, 9)
    gen, step = make_step(sd, amp, max_norm=1.0)
    losses, grads = [], []
    for k in range(3):
        _, x, real, m = E.pretrain_draw(8, 2, 64, 20 + k)
        losses.append(step(x.to(DEV), real.to(DEV), m.to(DEV)).clone())
        grads.append(step.optimizer.grad.clone())
    return gen, step, losses, grads


def test_three_amp_steps_are_bit_reproducible():
    g1, s1, l1, gr1 = run_three_steps(True)
    g2, s2, l2, gr2 = run_three_steps(True)
    assert s1.optimizer.step_count == 3 and s1.skipped_steps == 0
    for a, b in zip(l1 + gr1, l2 + gr2):
        assert torch.equal(a, b)
    for (k, a), (_, b) in zip(g1.state_dict().items(), g2.state_dict().items()):
        assert torch.equal(a, b), k
    assert int(g1.state_dict()["encoder.3.num_batches_tracked"]) == 3
    assert all(np.isfinite(float(v)) for v in l1)


def test_fp32_step_is_untouched_and_inference_plans_survive_training():
    import emulate_plain_f16_train as E
    import plain_generator
    from mstg_hip import ops
    from mstg_hip.optim import FlatAdam
    gen, step, losses, _ = run_three_steps(False)
    sd, _, _, _ = E.pretrain_draw(8, 2, 64, 9)
    hand = plain_generator.Generator(8)
    hand.load_state_dict(sd)
    hand.to(DEV).train()
    opt = FlatAdam(hand.parameters(), lr=2e-4, betas=(0.5, 0.999))
    for k in range(3):
        _, x, real, m = E.pretrain_draw(8, 2, 64, 20 + k)
        opt.zero_grad()
        with ops.direct_param_grads():
            loss = ops.masked_l1_loss(hand(x.to(DEV)), real.to(DEV), m.to(DEV))
            loss.backward()
        ops.clip_grad_norm_flat_(opt.grad, 1.0)
        opt.step()
        assert torch.equal(loss.detach(), losses[k])
    for (k, a), (_, b) in zip(gen.state_dict().items(), hand.state_dict().items()):
        assert torch.equal(a, b), k
    assert step.optimizer.step_count == 3 and opt.step_count == 3

    trained, _, _, _ = run_three_steps(True)
    _, x, _, _ = E.pretrain_draw(8, 2, 64, 30)
    trained.eval().half_inference()
    fresh = plain_generator.Generator(8)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in trained.state_dict().items()})
    fresh.to(DEV).eval().half_inference()
    with torch.no_grad():
        y1, y2 = trained(x.to(DEV)), fresh(x.to(DEV))
        assert y1.dtype == torch.float16 and torch.equal(y1, y2)
        trained.graph_inference()
        fresh.graph_inference()
        assert torch.equal(trained(x.to(DEV)), y1) and torch.equal(fresh(x.to(DEV)), y1)


def _img(hh, ww, seed):
    rs = np.random.RandomState(seed)
    base = rs.randint(0, 256, size=(hh // 4 + 2, ww // 4 + 2, 3)).astype(np.uint8)
    img = np.kron(base, np.ones((4, 4, 1), dtype=np.uint8))[:hh, :ww]
    return np.ascontiguousarray((img.astype(np.int32) + rs.randint(-20, 21, size=img.shape)).clip(0, 255).astype(np.uint8))


def test_amp_training_loop_runs_and_checkpoints_move_between_precisions(tmp_path):
    import plain_generator
    import pretrain
    arrays_a = [_img(270 + 3 * i, 300 + 5 * i, 20 + i) for i in range(4)]
    arrays_b = [_img(300 + 2 * i, 260 + 7 * i, 40 + i) for i in range(4)]

    def datasets():
        return (pretrain.MonetPhotoDataset(arrays=arrays_a, device=DEV, img_size=64), pretrain.MonetPhotoDataset(arrays=arrays_b, device=DEV, img_size=64))

    gen, hist = pretrain.train(None, tmp_path / "amp", num_epochs=50, batch_size=2, channels=8, datasets=datasets(), log_every=1000, amp=True)
    first, last = np.mean([v[2] for v in hist[:4]]), np.mean([v[2] for v in hist[-4:]])
    print(f"  amp loop: mean loss of the first four {first:.4f}, of the last four {last:.4f}; skipped steps {gen.pretrain_step.skipped_steps}")
    assert all(np.isfinite(v[2]) for v in hist) and last < first, (first, last)
    assert gen.pretrain_step.skipped_steps == 0 and gen.pretrain_step.optimizer.step_count == 200
    path = tmp_path / "amp" / "generator_pretrain_epoch_50.pth"
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "loss"} and ck["epoch"] == 49
    g2 = plain_generator.Generator(channels=8)
    g2.load_state_dict(ck["model_state_dict"])
    for (k, v), (_, v2) in zip(gen.state_dict().items(), g2.state_dict().items()):
        assert torch.equal(v.cpu(), v2), k
    # resume the amp checkpoint in fp32, and an fp32 checkpoint under amp
    gen32, hist32 = pretrain.train(None, tmp_path / "fp32", num_epochs=52, batch_size=2, channels=8, datasets=datasets(), log_every=1000,
                                   resume_path=str(path), continue_epochs=True, save_every=52)
    assert len(hist32) == 4 and all(np.isfinite(v[2]) for v in hist32) and gen32.pretrain_step.optimizer.step_count == 208
    path32 = tmp_path / "fp32" / "generator_pretrain_epoch_52.pth"
    gen16, hist16 = pretrain.train(None, tmp_path / "back", num_epochs=54, batch_size=2, channels=8, datasets=datasets(), log_every=1000,
                                   resume_path=str(path32), continue_epochs=True, save_every=54, amp=True)
    assert len(hist16) == 4 and all(np.isfinite(v[2]) for v in hist16)
    assert gen16.pretrain_step.optimizer.step_count == 216 and gen16.pretrain_step.skipped_steps == 0
    assert np.mean([v[2] for v in hist16]) < first


@pytest.mark.parametrize("shape", [(64, 3, 256, 256), (1, 3, 1024, 1024)], ids=["64x256x256", "1x1024x1024"])
def test_amp_step_at_size(shape):
    """Generator(64) at the largest batch and the largest image the step is meant for: finite loss and gradient norm."""
    import plain_generator
    import pretrain
    torch.manual_seed(3)
    gen = plain_generator.Generator(64).to(DEV).train()
    step = pretrain.PretrainStep(gen, amp=True)
    g = torch.Generator().manual_seed(4)
    x, real = torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1
    m = (torch.rand((shape[0], 1, 8, 8), generator=g) < 0.4).float().repeat_interleave(shape[2] // 8, 2).repeat_interleave(shape[3] // 8, 3)
    m = m.expand(shape).contiguous()
    loss = step((x * (1 - m)).to(DEV), real.to(DEV), m.to(DEV))
    print(f"  {shape}: loss {float(loss):.5f}, gradient norm {float(step.last_grad_norm):.4e}, loss scale {step.loss_scale:.0f}")
    assert np.isfinite(float(loss)) and 0.0 < float(loss) < 2.0
    assert np.isfinite(float(step.last_grad_norm)) and float(step.last_grad_norm) > 0.0
    assert step.skipped_steps == 0 and step.optimizer.step_count == 1
