"""Train step with the mixed-precision multi-style loss (enhanced_train.attach_style_loss(..., precision="mixed")).

EnhancedCycleGAN at channels 8, (2,3,32,32), width_div=4: one step with precision="mixed" and one with "fp32" from identical state
and inputs.  The five non-style losses are bit-equal; style_loss is within the whole-loss bar (2 x the distance the CPU emulation
has from the float64 yardstick, tests/style_f16_ref.py) on this step's fake_A; the flat generator gradient is finite and within 0.3
relative L2 of the fp32 path's -- a cap that separates error classes (a lost, doubled or sign-flipped style gradient), not a
precision claim: lambda_style is chosen from the fp32 path alone so that the style term is at least half of the gradient's norm."""
import math

import pytest
import torch

import style_f16_ref as E
from conftest import rel_l2
from f16_helpers import DEV, _lib_loaded  # noqa: F401

pytestmark = pytest.mark.gpu

C_, SHAPE, DIV = 8, (2, 3, 32, 32), 4
NON_STYLE = ("d_loss", "g_loss", "cycle_loss", "identity_loss", "structure_loss")


def styles():
    return E.loss_inputs()[2]


def build(precision, lam, attach=True):
    """a fresh model on seeded weights; its optimizers capture the gradient and do not step"""
    import enhanced_train
    R = E.R
    sds = [R.make_state_dict(R.generator_spec(C_), 81), R.make_state_dict(R.generator_spec(C_), 82),
           R.make_state_dict(R.discriminator_spec(C_), 83), R.make_state_dict(R.discriminator_spec(C_), 84)]
    model = enhanced_train.EnhancedCycleGAN(channels=C_, num_transformer_blocks=0, device=torch.device(DEV))
    for m, sd in zip((model.G_AB, model.G_BA, model.D_A, model.D_B), sds):
        m.load_state_dict(sd)
    if attach:
        model.attach_style_loss(styles(), E.WEIGHTS3, lambda_style=lam, width_div=DIV, precision=precision)
    return model


def step(model):
    R = E.R
    a, b = R.make_input(SHAPE, 90), R.make_input(SHAPE, 91)
    captured = {}
    model.g_optimizer.step = lambda: captured.__setitem__("g", model.g_optimizer.grad.clone())
    model.d_optimizer.step = lambda: None
    losses = model.train_step(a.to(DEV), b.to(DEV))
    return losses, captured["g"].double().cpu()


_RUNS = {}


def runs():
    """the three steps, taken once: without the style loss, with it in fp32 (the parent's code) and mixed"""
    if not _RUNS:
        _, g_plain = step(build(None, 0.0, attach=False))
        # the style gradient is linear in lambda_style: measure it on the fp32 path at a probe value, then take the power of ten at
        # which it is at least as long as the rest of the gradient (its share of the whole is then at least one half)
        probe = 1e4
        _, g_probe = step(build("fp32", probe))
        per_unit = float((g_probe - g_plain).norm()) / probe
        lam = 10.0 ** math.ceil(math.log10(float(g_plain.norm()) / per_unit))
        l32, g32 = step(build("fp32", lam))
        lmx, gmx = step(build("mixed", lam))
        _RUNS.update(lam=lam, g_plain=g_plain, l32=l32, g32=g32, lmx=lmx, gmx=gmx)
    return _RUNS


def test_step_mixed_against_fp32():
    r = runs()
    lam, l32, lmx, g32, gmx = r["lam"], r["l32"], r["lmx"], r["g32"], r["gmx"]
    share = float((g32 - r["g_plain"]).norm() / g32.norm())
    print(f"  lambda_style {lam:g}: the style term is {share:.2f} of the generator gradient's norm on the fp32 path (needs >= 0.5)")
    assert share >= 0.5
    for k in NON_STYLE:
        assert l32[k] == lmx[k], (k, l32[k], lmx[k])
    # the whole-loss bar on this step's own fake_A and feature weights
    model = build("fp32", lam)
    with torch.no_grad():
        fake_A = model.G_BA(E.R.make_input(SHAPE, 91).to(DEV)).float().cpu()
    sd = {k: v.detach().cpu().clone() for k, v in model.style_loss.features.state_dict().items()}
    yard = float(E.yardstick(E.rounded_weights(sd), fake_A, styles(), E.WEIGHTS3)["loss"])
    emu = float(E.emulate(sd, fake_A, styles(), E.WEIGHTS3, with_grad=False)["loss"])
    bar = 2 * abs(emu - yard) / yard
    err = abs(lmx["style_loss"] / lam - yard) / yard
    print(f"  style_loss / lambda: mixed {lmx['style_loss'] / lam:.9e}  fp32 path {l32['style_loss'] / lam:.9e}  float64 {yard:.9e}  "
          f"emulation {emu:.9e}")
    print(f"  [step] style_loss: device {err:.3e}  emulation {abs(emu - yard) / yard:.3e}  bar {bar:.3e}")
    assert err <= bar
    assert bool(torch.isfinite(gmx).all())
    d = rel_l2(gmx, g32)
    print(f"  [step] flat generator gradient: relative L2 distance from the fp32 path's {d:.4f} (cap 0.3); "
          f"of the style part alone {float((gmx - g32).norm() / (g32 - r['g_plain']).norm()):.4f}")
    assert d < 0.3


def test_environment_selects_the_path(monkeypatch):
    r = runs()
    monkeypatch.setenv("MSTG_STYLE_PRECISION", "mixed")
    model = build(None, r["lam"])
    assert model.style_loss.precision == "mixed" and model.style_loss.features.precision == "mixed"
    losses, g = step(model)
    assert losses == r["lmx"] and torch.equal(g, r["gmx"])
    monkeypatch.delenv("MSTG_STYLE_PRECISION")
    assert build(None, 1.0).style_loss.precision == "fp32"
    assert build("fp32", 1.0).style_loss.precision == "fp32"


def test_unknown_precision_raises(monkeypatch):
    with pytest.raises(ValueError, match="precision"):
        build("fp16", 1.0)
    monkeypatch.setenv("MSTG_STYLE_PRECISION", "half")
    with pytest.raises(ValueError, match="precision"):
        build(None, 1.0)
