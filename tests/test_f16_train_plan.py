"""CPU side of the mixed-precision pre-training step (mstg_hip/train_plain.py, pretrain.PretrainStep(amp=True)): the loss-scale
rules, the width check (before anything touches a device), host-side validation of the new entry points, and the fixture's own
consistency.  No kernel is launched here."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLD, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_auto_loss_scale_is_next_power_of_two():
    from mstg_hip.train_plain import auto_loss_scale
    for shape in ((4, 3, 64, 64), (16, 3, 256, 256), (1, 3, 16, 16), (48, 3, 128, 128), (2, 3, 48, 80), (1, 3, 1024, 1024), (3, 3, 16, 48)):
        numel = int(np.prod(shape))
        want = 2.0 ** int(np.ceil(np.log2(numel)))
        got = auto_loss_scale(numel)
        print(f"  numel {numel}: auto loss scale {got:.0f} (2**ceil(log2) = {want:.0f})")
        assert got == want and got >= numel > got / 2


def test_loss_scale_must_be_a_power_of_two():
    import plain_generator
    import pretrain
    from mstg_hip.train_plain import check_loss_scale
    for ok in (1.0, 2.0, 65536.0, 2.0 ** 40, 0.5, 1):
        assert check_loss_scale(ok) == float(ok)
    for bad in (3.0, 1000.0, 0.0, -2.0, float("inf"), float("nan"), 65535.0):
        with pytest.raises(ValueError, match="power of two"):
            check_loss_scale(bad)
    with pytest.raises(ValueError, match="power of two"):
        pretrain.PretrainStep(plain_generator.Generator(8), amp=True, loss_scale=1000.0)


@pytest.mark.parametrize("channels", [12, 72])
def test_unsupported_width_raises_without_a_gpu(channels):
    import plain_generator
    import pretrain
    with pytest.raises(RuntimeError, match=f"channels={channels}"):
        pretrain.PretrainStep(plain_generator.Generator(channels), amp=True)


def test_eval_mode_raises():
    import plain_generator
    import pretrain
    with pytest.raises(RuntimeError, match="training mode"):
        pretrain.PretrainStep(plain_generator.Generator(8).eval(), amp=True)


def test_plan_bytes_entry_points_validate(lib):
    assert lib.mstg_f16_train_wgrad_workspace_bytes(2, 8, 8, 64, 32, 32) > 0
    assert lib.mstg_f16_train_wgrad_workspace_bytes(2, 8, 8, 64, 8, 3) > 0
    assert lib.mstg_f16_train_wgrad_workspace_bytes(2, 8, 8, 12, 32, 32) == 0
    assert b"Cs" in lib.mstg_last_error()
    assert lib.mstg_f16_train_wgrad_workspace_bytes(2, 8, 8, 64, 520, 520) == 0
    assert b"Cb" in lib.mstg_last_error()
    assert lib.mstg_f16_train_wgrad_workspace_bytes(2, 8, 8, 64, 32, 40) == 0
    assert b"CbOut" in lib.mstg_last_error()
    assert lib.mstg_f16_train_wgrad_workspace_bytes(0, 8, 8, 64, 32, 32) == 0
    assert b"positive" in lib.mstg_last_error()
    assert lib.mstg_f16_train_bn_workspace_bytes(1024, 64) > 0
    assert lib.mstg_f16_train_bn_workspace_bytes(1024, 12) == 0
    assert b"multiple of 8" in lib.mstg_last_error()
    assert lib.mstg_f16_train_bn_workspace_bytes(1024, 1024) == 0
    assert b"512" in lib.mstg_last_error()
    assert lib.mstg_f16_train_loss_workspace_bytes(2, 64, 64) > 0
    assert lib.mstg_f16_train_loss_workspace_bytes(2, 0, 64) == 0
    assert b"positive" in lib.mstg_last_error()
    assert lib.mstg_f16_train_wgrad(None, None, 2, 8, 8, 64, 32, 32, None, None, None, 0, None) == -1  # null pointers
    assert lib.mstg_f16_train_bn_fwd(1, 1, 1, 1, 64, 0, 1e-5, 0.1, None, None, 1, 1, 1, 1, 1 << 30, None) == -1  # one value per channel
    assert lib.mstg_f16_train_adam(1, 1, 1, 1, 4, 1e-3, 0.5, 0.999, 1e-8, -1, 1, None) == -1


def test_flat_adam_step_count_without_device_state_is_a_plain_integer():
    from mstg_hip import optim
    assert isinstance(optim.FlatAdam.step_count, property)


def test_fixture_is_self_consistent():
    """The stored fp64 loss is reproduced (1e-9 relative; the slack is for another BLAS summing in another order) by the oracle's
    restated forward on weights / inputs regenerated from the seed: guards the seed recipe the GPU tests rebuild the draw from."""
    import emulate_plain_f16_train as E
    from oracle import restatement as R
    z = np.load(os.path.join(GOLD, "pretrain_amp_c8_64x64.npz"))
    C, (N, _, S, _) = int(z["C"]), z["shape"]
    assert os.path.getsize(os.path.join(GOLD, "pretrain_amp_c8_64x64.npz")) < 1500000
    for s in z["seeds"]:
        sd, x, real, m = E.pretrain_draw(C, int(N), int(S), int(s))
        assert np.array_equal(m.numpy().astype(np.uint8), z[f"s{s}_mask"])
        sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
        y = R.plain_generator_forward(sd64, x.double(), train=True)
        loss = float(E.masked_l1(y, real.double(), m.double()))
        want = float(z[f"s{s}_loss64"])
        print(f"  seed {s}: restated fp64 loss {loss:.12f}, stored {want:.12f}, relative difference {abs(loss - want) / want:.1e} (tol 1e-9)")
        assert abs(loss - want) <= 1e-9 * want
        assert 0.0 < float(z[f"s{s}_amp_dist"]) <= 0.08
        for k in E.param_names(C):
            assert tuple(z[f"s{s}_g64_{k}"].shape) == tuple(sd[k].shape)
