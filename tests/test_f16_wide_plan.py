"""CPU: the fp16 inference planner accepts the layers of EnhancedGenerator(channels=32 / 64) -- stage widths up to 256 channels,
served by csrc/infer_f16_wide.hip -- and still refuses what no kernel serves.  No kernel is launched here."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


def desc(kind, Cin, Cout, K, stride, pad, N=2, H=32, W=48):
    from mstg_hip.infer import _desc
    if kind == 1:
        Ho, Wo = 2 * H, 2 * W
    elif kind == 2:
        Ho, Wo = H, W
    else:
        Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    return _desc(kind, N, H, W, Cin, Ho, Wo, Cout, K, stride, pad)


WIDE = [
    # kind, Cin, Cout, K, stride, pad: every layer the channels=32 / 64 generators add
    (0, 64, 128, 4, 2, 1),    # down1 at channels=64, down2 at channels=32
    (0, 128, 256, 4, 2, 1),   # down2 at channels=64
    (1, 256, 128, 4, 2, 1),   # up1 at channels=64
    (1, 128, 64, 4, 2, 1),    # up1 at channels=32, up2 at channels=64
    (2, 128, 128, 3, 1, 4),   # MultiScaleBlock branches
    (2, 256, 256, 3, 1, 4),
    (0, 128, 128, 1, 1, 0),   # fusion 1x1
    (0, 256, 256, 1, 1, 0),
]


@pytest.mark.parametrize("geom", WIDE, ids=[f"k{g[0]} {g[1]}->{g[2]} k{g[3]} s{g[4]}" for g in WIDE])
def test_wide_conv_geometries_have_a_plan(lib, geom):
    d = desc(*geom)
    assert lib.mstg_f16_conv_plan_bytes(C.byref(d)) > 0, lib.mstg_last_error().decode()
    assert lib.mstg_f16_conv_partial_bytes(C.byref(d)) >= d.N * 2 * d.Cout * 4


def test_narrow_stem_and_head_at_64_channels_have_a_plan(lib):
    from mstg_hip._lib import ACT_TANH
    from mstg_hip.infer import _desc
    stem = _desc(0, 1, 32, 32, 3, 32, 32, 64, 7, 1, 3, 1, 1)
    head = _desc(0, 1, 32, 32, 64, 32, 32, 3, 7, 1, 3, 1, 0, 1, ACT_TANH)
    assert lib.mstg_f16_conv_plan_bytes(C.byref(stem)) > 0
    assert lib.mstg_f16_conv_plan_bytes(C.byref(head)) > 0


def test_wide_attention_has_a_plan(lib):
    for c in (16, 32, 64, 128, 256):
        assert lib.mstg_f16_attn_plan_bytes(c) == 4 * c * 4 + 4 * c * c * 2


@pytest.mark.parametrize("geom,what", [((0, 48, 128, 4, 2, 1), b"multiple of 32"),
                                       ((0, 128, 512, 1, 1, 0), b"256"),
                                       ((0, 512, 128, 1, 1, 0), b"256"),
                                       ((2, 192, 192, 3, 1, 4), b"msblock")])
def test_unsupported_geometries_still_refused(lib, geom, what):
    d = desc(*geom)
    assert lib.mstg_f16_conv_plan_bytes(C.byref(d)) == 0
    assert what in lib.mstg_last_error()


def test_unsupported_attention_width_refused(lib):
    assert lib.mstg_f16_attn_plan_bytes(512) == 0
    assert b"256" in lib.mstg_last_error()
    assert lib.mstg_f16_attn_plan_bytes(48) == 0


def test_norm_residual_widths(lib):
    # host-side checks only: C = 128 / 256 pass validation (null pointers then fail), other widths are refused
    assert lib.mstg_f16_norm_residual(None, None, None, None, 1, 16, 128, None) == -1
    assert lib.mstg_f16_norm_residual(1, None, 1, 1, 1, 16, 96, None) != 0
    assert b"C must be" in lib.mstg_last_error()
