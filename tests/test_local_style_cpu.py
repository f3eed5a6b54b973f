"""CPU: the device weight map of process_local_style's 'enhanced' mode (csrc/local_style.hip, mstg_hip.image.enhanced_weight_map)
up to the launch.  The numpy restatement the GPU tests compare with (tests/local_style_ref.py) is pinned with closed forms, the
integer formulations the kernels evaluate are checked against it, the tap order of the kernel's Gaussian is shown to reproduce
scipy's bits, and the C-ABI entry points validate on the host.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch

import local_style_ref as LR
from conftest import PKG, ROOT

NEW_SYMBOLS = ["mstg_local_style_workspace_bytes", "mstg_local_style_prepare", "mstg_local_style_hysteresis", "mstg_local_style_weights",
               "mstg_local_style_weight_map"]


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _rgb(g):
    return np.ascontiguousarray(np.repeat(np.asarray(g, dtype=np.uint8)[..., None], 3, axis=-1))


# ---- the restatement, pinned with closed forms ------------------------------------------------------------------------------------
def test_gray_of_primaries_and_white():
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]], dtype=np.uint8)
    # (255 * 4899 + 8192) >> 14 = 76, (255 * 9617 + 8192) >> 14 = 150, (255 * 1868 + 8192) >> 14 = 29; the weights sum to 2^14
    assert LR.gray_u8(px).tolist() == [76, 150, 29, 255, 0]
    g = np.arange(256, dtype=np.uint8)
    assert np.array_equal(LR.gray_u8(_rgb(g)), g)


def test_saturation_and_value_by_hand():
    px = np.array([[0, 0, 0], [255, 0, 0], [200, 100, 50], [50, 100, 200], [255, 150, 150], [255, 160, 160], [7, 7, 7], [151, 151, 151]],
                  dtype=np.uint8)
    s, v = LR.sat_val(px)
    # sdiv[255] = 4096: s = diff; sdiv[200] = round(5222.4) = 5222: (150 * 5222 + 2048) >> 12 = 191; v = 0 has sdiv 0
    assert v.tolist() == [0, 255, 200, 200, 255, 255, 7, 151]
    assert s.tolist() == [0, 255, 191, 191, 105, 95, 0, 0]
    assert LR.sky_mask(px).tolist() == [False, False, False, False, False, True, False, True]
    assert not LR.sky_mask(np.array([[150, 150, 150]], dtype=np.uint8))[0]  # v > 150 is strict


def test_sdiv_table_in_integers():
    """the kernel builds the table without floating point: quotient, remainder, round half to even"""
    t = LR.sdiv_table()
    assert t[0] == 0 and t[255] == 4096 and t[1] == 1044480
    for i in range(1, 256):
        q, r = divmod(1044480, i)
        assert q + (1 if (2 * r > i or (2 * r == i and q & 1)) else 0) == t[i], i


def test_step_edge_gives_one_line_in_the_column_the_rule_selects():
    g = np.zeros((20, 24), dtype=np.uint8)
    g[:, 10:] = 200  # columns 9 and 10 both have |dx| = 800; m > m[left] && m >= m[right] keeps column 9 only
    dx, dy = LR.sobel(g)
    assert (dx[:, 9] == 800).all() and (dx[:, 10] == 800).all() and not dy.any()
    state = LR.state_map(g)
    want = np.ones_like(g)
    want[:, 9] = 2
    assert np.array_equal(state, want)
    edge = LR.canny(g)
    assert edge[:, 9].all() and edge.sum() == 20
    assert np.array_equal(LR.canny(g.T.copy()), edge.T)  # a horizontal step: row 9 by the same rule, m > m[up] && m >= m[down]
    assert LR.canny(g[:, ::-1].copy())[:, 13].all() and LR.canny(g[:, ::-1].copy()).sum() == 20  # mirrored: still the left one of 13, 14


def test_step_below_low_gives_no_edge():
    """A step of h grey levels has the Sobel magnitude 4 h.  Magnitude 40 (h = 10) is below ``low`` = 50: nothing survives.  (A step
    of 40 grey levels has magnitude 160, above ``high``, and is an edge; one of 20 has magnitude 80, a candidate without a seed.)"""
    for h, edges, states in ((10, 0, {1}), (12, 0, {1}), (20, 0, {0, 1}), (40, 20, {1, 2})):
        g = np.full((20, 24), 100, dtype=np.uint8)
        g[:, 10:] += h
        assert int(LR.canny(g).sum()) == edges, h
        assert set(np.unique(LR.state_map(g)).tolist()) == states, h


def test_ramp_between_the_thresholds_has_no_seed():
    g = np.tile((15 * np.arange(16)).astype(np.uint8), (12, 1))  # |dx| = 120 inside, 60 in the two border columns
    dx, dy = LR.sobel(g)
    m = np.abs(dx) + np.abs(dy)
    assert m.min() == 60 and m.max() == 120
    state = LR.state_map(g)
    assert (state == 0).any() and not (state == 2).any()  # column 1 beats column 0 and ties with column 2: candidates only
    assert (state[:, 1] == 0).all() and (state == 0).sum() == 12
    assert not LR.canny(g).any()


def test_hysteresis_restatement_by_hand():
    st = np.array([[2, 1, 0, 1, 1],
                   [1, 0, 1, 1, 0],
                   [1, 1, 1, 1, 0],
                   [0, 1, 1, 1, 1]], dtype=np.uint8)
    want = np.array([[1, 0, 1, 0, 0],
                     [0, 1, 0, 0, 0],
                     [0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0]], dtype=bool)  # the chain along the diagonals is reached, the two other groups are not
    assert np.array_equal(LR.hysteresis(st), want)
    sp = LR.spiral_state(48, 64)
    assert (sp == 2).sum() == 1 and LR.hysteresis(sp).sum() == (sp != 1).sum() > 48 * 64 // 3
    assert not LR.hysteresis(LR.spiral_state(48, 64, strong=False)).any()


def test_gaussian_tap_order_reproduces_scipy():
    """csrc/local_style.hip sums centre tap first, then the symmetric pairs from the outermost inwards, along axis 0 and then axis 1,
    with the 'reflect' index of any distance: in numpy float64 that order gives scipy.ndimage.gaussian_filter's bits, and the taps
    in the kernel source are exp(-x^2 / 8) / sum as numpy evaluates them."""
    x = np.arange(-8, 9)
    k = np.exp(-0.5 / 4.0 * x ** 2)
    k = (k / k.sum())[8:]
    src = open(os.path.join(PKG, "mstg_hip", "csrc", "local_style.hip")).read()
    taps = [float.fromhex(h) for h in re.findall(r"0x1\.[0-9a-f]+p-\d+", src.split("LC_K[LC_R + 1]")[1].split("};")[0])]
    assert taps == k.tolist()

    def refl(i, n):
        i = i % (2 * n)
        return np.where(i < n, i, 2 * n - 1 - i)

    def axis_pass(a, axis):
        a = np.moveaxis(a, axis, 0)
        idx = np.arange(a.shape[0])
        t = a * k[0]
        for j in range(8, 0, -1):
            t = t + (a[refl(idx - j, a.shape[0])] + a[refl(idx + j, a.shape[0])]) * k[j]
        return np.moveaxis(t, 0, axis)
    rs = np.random.RandomState(0)
    for shape in ((67, 93), (5, 3), (1, 1), (1, 40), (96, 80)):
        e = (rs.rand(*shape) < 0.1).astype(float)
        assert np.array_equal(axis_pass(axis_pass(e, 0), 1), LR.gaussian(e)), shape


def test_weight_levels_and_assignment_order():
    from mstg_hip import image as dimg
    assert dimg.local_style_weights(0.8, 0.7) == (0.8, 1.0, 0.8 - 0.3 * 0.7) == LR.weights(0.8, 0.7)
    assert dimg.local_style_weights(0.1, 0.7, 0.4) == (0.1, 0.1 + 0.2, 0.0)
    assert dimg.local_style_weights(0.65, 1.0, 0.4) == (0.65, 0.65 + 0.2, 0.65 - 0.4 * 1.0)
    r = LR.enhanced_weight_map(LR.bright_low_saturation(256, 256, 1))
    assert r["has_sky"] and set(np.unique(r["weight"]).tolist()) == {0.8 - 0.3 * 0.7, 0.8, 1.0}
    assert (r["weight"][r["detail"]] == 0.8 - 0.3 * 0.7).all() and (r["detail"] & r["sky"]).any()  # detail overrides sky
    for n_sky, flag in ((6999, False), (7000, False), (7001, True)):
        r = LR.enhanced_weight_map(LR.sky_threshold_canvas(100, 100, n_sky, 5))
        assert r["has_sky"] is flag and int(r["sky"].sum()) == n_sky and not r["edge"].any()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_and_bound(lib):
    from mstg_hip import _lib
    header = open(os.path.join(ROOT, "include", "mstg_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define MSTG_LOCAL_STYLE_MAX_PIXELS %d" % _lib.LOCAL_STYLE_MAX_PIXELS in header


def test_host_side_validation(lib):
    P = 4096  # any non-null, 8-byte aligned address: every call below is refused before a launch
    assert lib.mstg_local_style_workspace_bytes(1, 384, 384) >= 3 * 384 * 384 + 4
    assert lib.mstg_local_style_workspace_bytes(64, 256, 256) >= 3 * 64 * 65536 + 256
    assert lib.mstg_local_style_workspace_bytes(1, 385, 384) == 0 and b"385 x 384" in lib.mstg_last_error()
    assert lib.mstg_local_style_workspace_bytes(0, 16, 16) == 0
    # over the LDS limit: UNSUPPORTED, naming the size
    assert lib.mstg_local_style_hysteresis(P, 1, 385, 384, P, None) == -5
    assert b"385 x 384" in lib.mstg_last_error() and b"147456" in lib.mstg_last_error()
    assert lib.mstg_local_style_weight_map(P, 2, 1, 147457, 0.8, 1.0, 0.59, P, P, 1 << 30, None) == -5
    assert b"1 x 147457" in lib.mstg_last_error()
    # null pointers
    assert lib.mstg_local_style_prepare(None, 1, 16, 16, P, P, P, None, None) == -1
    assert lib.mstg_local_style_prepare(P, 1, 16, 16, None, P, P, None, None) == -1
    assert lib.mstg_local_style_prepare(P, 1, 16, 16, P, None, P, None, None) == -1
    assert lib.mstg_local_style_prepare(P, 1, 16, 16, P, P, None, None, None) == -1
    assert lib.mstg_local_style_hysteresis(None, 1, 16, 16, P, None) == -1
    assert lib.mstg_local_style_hysteresis(P, 1, 16, 16, None, None) == -1
    assert lib.mstg_local_style_weights(None, P, P, 1, 16, 16, 0.8, 1.0, 0.59, P, None, None) == -1
    assert lib.mstg_local_style_weights(P, None, P, 1, 16, 16, 0.8, 1.0, 0.59, P, None, None) == -1
    assert lib.mstg_local_style_weights(P, P, None, 1, 16, 16, 0.8, 1.0, 0.59, P, None, None) == -1
    assert lib.mstg_local_style_weights(P, P, P, 1, 16, 16, 0.8, 1.0, 0.59, None, None, None) == -1
    assert lib.mstg_local_style_weight_map(None, 1, 16, 16, 0.8, 1.0, 0.59, P, P, 1 << 20, None) == -1
    assert lib.mstg_local_style_weight_map(P, 1, 16, 16, 0.8, 1.0, 0.59, None, P, 1 << 20, None) == -1
    # N = 0 and empty images
    assert lib.mstg_local_style_prepare(P, 0, 16, 16, P, P, P, None, None) == -1 and b"N = 0" in lib.mstg_last_error()
    assert lib.mstg_local_style_hysteresis(P, 0, 16, 16, P, None) == -1
    assert lib.mstg_local_style_weights(P, P, P, 0, 16, 16, 0.8, 1.0, 0.59, P, None, None) == -1
    assert lib.mstg_local_style_weight_map(P, 0, 16, 16, 0.8, 1.0, 0.59, P, P, 1 << 20, None) == -1
    assert lib.mstg_local_style_prepare(P, 1, 0, 16, P, P, P, None, None) == -1
    assert lib.mstg_local_style_hysteresis(P, 1, 16, 0, P, None) == -1
    # workspace and alignment
    assert lib.mstg_local_style_weight_map(P, 1, 16, 16, 0.8, 1.0, 0.59, P, None, 0, None) == -4
    need = lib.mstg_local_style_workspace_bytes(1, 16, 16)
    assert lib.mstg_local_style_weight_map(P, 1, 16, 16, 0.8, 1.0, 0.59, P, P, need - 1, None) == -4
    assert lib.mstg_local_style_weight_map(P, 1, 16, 16, 0.8, 1.0, 0.59, P + 4, P, need, None) == -2
    assert lib.mstg_local_style_weight_map(P, 1, 16, 16, 0.8, 1.0, 0.59, P, P + 8, need, None) == -2
    assert lib.mstg_local_style_weights(P, P, P, 1, 16, 16, 0.8, 1.0, 0.59, P + 4, None, None) == -2
    assert lib.mstg_local_style_prepare(P, 1, 16, 16, P, P, P + 2, None, None) == -2


def test_python_boundary_rejects_what_is_not_a_device_canvas():
    from mstg_hip import image as dimg
    with pytest.raises(RuntimeError, match="canvas on the GPU"):
        dimg.enhanced_weight_map(torch.zeros(8, 8, 3, dtype=torch.uint8))
