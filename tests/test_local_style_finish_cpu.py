"""CPU: the finish of process_local_style's 'enhanced' mode (csrc/local_style.hip local_style_finish_kernel,
mstg_hip.image.local_style_finish) up to the launch.  The numpy restatement the GPU tests compare with
(tests/local_style_finish_ref.py: cv2.convertScaleAbs on the float64 blend, smooth_transitions) is pinned with closed forms, the
share of bytes on which other evaluations of the colour step would differ from the definition is measured (and bounded by one
grey level), and the new C-ABI entry points validate on the host.  The restatement has not been compared with an OpenCV binary.
No kernel is launched here."""
import numpy as np
import pytest

import local_style_finish_ref as FR
import local_style_ref as LR

NEW_SYMBOLS = ["mstg_local_style_finish", "mstg_local_style_enhanced_workspace_bytes", "mstg_local_style_enhanced"]


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


# ---- the colour step ----------------------------------------------------------------------------------------------------------------
def test_enhance_closed_forms():
    # 0 * 1.1 + 5 = 5; 100 * 1.1f + 5 = 115.0000024 -> 115; 227.5 * 1.1f + 5 = 255.25 -> 255; 255 * 1.1f + 5 = 285.5 -> saturates
    assert FR.enhance_u8(np.array([0.0, 100.0, 227.5, 255.0])).tolist() == [5, 115, 255, 255]
    assert FR.enhance_u8(np.array([-100.0])).tolist() == [105]  # the absolute value: |-110 + 5|
    # no float32 x makes x * 1.1f + 5 an exact tie, so the tie rule is pinned on the rounding step the restatement uses
    assert np.rint(np.float32([114.5, 115.5])).tolist() == [114.0, 116.0]


def test_enhance_is_one_rounding():
    """the float64 emulation is the fused operation: product and sum are exact there (checked with exact rationals on a sample)"""
    from fractions import Fraction
    rs = np.random.RandomState(0)
    xs = np.concatenate([rs.rand(500) * 255, np.arange(0, 256, 17).astype(np.float64), [0.0625, 0.07, 1e-3 + 0.0625]])
    got = (xs.astype(np.float32).astype(np.float64) * np.float64(FR.ALPHA32) + 5.0)
    for x, g in zip(xs, got):
        exact = Fraction(float(np.float32(x))) * Fraction(float(FR.ALPHA32)) + 5
        assert Fraction(float(g)) == exact, x


def _pairs(w):
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return FR.blend_f64(a[..., None], b[..., None], np.full((256, 256), w))


def test_all_byte_pairs_within_one_level_of_float64():
    x = _pairs(0.8)
    e = FR.enhance_u8(x).astype(np.int32)
    d = np.abs(e - FR.enhance_u8_float64(x).astype(np.int32))
    assert d.max() <= 1
    assert np.abs(e - FR.enhance_u8_unfused(x).astype(np.int32)).max() <= 1


def test_measured_share_of_other_evaluations(capsys):
    """float64 and unfused float32 against the definition, on blends of this repository's generators with their own maps; the
    shares are printed (DESIGN.md 3d quotes them), the assertion is 'never more than one grey level'"""
    rows = []
    for name, gen in (("landscape", LR.landscape), ("blocky", LR.blocky), ("gradient_rects", LR.gradient_rects),
                      ("bright_low_saturation", LR.bright_low_saturation), ("noise", LR.noise)):
        canvas = gen(256, 256, 100)
        styled = np.ascontiguousarray(255 - canvas[:, ::-1])
        x = FR.blend_f64(canvas, styled, LR.enhanced_weight_map(canvas)["weight"])
        e = FR.enhance_u8(x).astype(np.int32)
        d64 = np.abs(e - FR.enhance_u8_float64(x).astype(np.int32))
        d32 = np.abs(e - FR.enhance_u8_unfused(x).astype(np.int32))
        rows.append((name, float((d64 != 0).mean()), int(d64.max()), float((d32 != 0).mean()), int(d32.max())))
    x = _pairs(0.8)
    e = FR.enhance_u8(x).astype(np.int32)
    d64, d32 = np.abs(e - FR.enhance_u8_float64(x).astype(np.int32)), np.abs(e - FR.enhance_u8_unfused(x).astype(np.int32))
    rows.append(("byte pairs, w = 0.8", float((d64 != 0).mean()), int(d64.max()), float((d32 != 0).mean()), int(d32.max())))
    with capsys.disabled():
        print()
        for name, s64, m64, s32, m32 in rows:
            print(f"  {name:24s} float64 differs on {100 * s64:.3f} % (max {m64})   unfused float32 on {100 * s32:.3f} % (max {m32})")
    assert all(m64 <= 1 and m32 <= 1 for _, _, m64, _, m32 in rows)


# ---- the blur -----------------------------------------------------------------------------------------------------------------------
def test_taps_and_constant_images():
    assert int(FR.TAPS.sum()) == 256 and FR.TAPS.tolist() == FR.TAPS[::-1].tolist()
    for shape in ((9, 11), (1, 1), (2, 3)):
        for v in range(256):
            assert (FR.blur7(np.full(shape, v, dtype=np.uint8)) == v).all(), (shape, v)


def test_single_bright_pixel_spreads_as_the_tap_products():
    for v in (255, 200, 1):
        img = np.zeros((15, 17), dtype=np.uint8)
        img[7, 8] = v
        want = np.zeros((15, 17), dtype=np.int64)
        want[4:11, 5:12] = (np.outer(FR.TAPS, FR.TAPS) * v + 32768) >> 16
        assert np.array_equal(FR.blur7(img), want)
    assert ((72 * 72 * 255 + 32768) >> 16) == 20


def _blur_row_by_hand(row):
    """one row through both passes: index p outside [0, n) mirrored without repeating the edge pixel, repeatedly; n == 1 gives 0.
    A one-row image is constant along y, so the vertical pass multiplies by 256."""
    n = len(row)

    def at(p):
        if n == 1:
            return 0
        period = 2 * n - 2
        p %= period
        return p if p < n else period - p
    h = [sum(int(FR.TAPS[k]) * int(row[at(x - 3 + k)]) for k in range(7)) for x in range(n)]
    return [(256 * s + 32768) >> 16 for s in h]


@pytest.mark.parametrize("row", [[37], [10, 200], [10, 200, 30, 90], [0, 255, 0, 255, 7]])
def test_narrow_images_follow_the_mirror_rule(row):
    got = FR.blur7(np.array([row], dtype=np.uint8))
    assert got[0].tolist() == _blur_row_by_hand(row)
    assert FR.blur7(np.array([row], dtype=np.uint8).T)[:, 0].tolist() == _blur_row_by_hand(row)  # and along y
    if row == [10, 200]:  # d c b | a b | a b a: the taps at -3..3 read b a b a b a b
        assert got[0].tolist() == [((8 + 56 + 56 + 8) * 200 + (28 + 72 + 28) * 10 + 128) >> 8, ((8 + 56 + 56 + 8) * 10 + (28 + 72 + 28) * 200 + 128) >> 8]
    if row == [10, 200, 30, 90]:  # x = 0 reads indices 3 2 1 0 1 2 3
        assert got[0][0] == ((8 * 90 + 28 * 30 + 56 * 200 + 72 * 10 + 56 * 200 + 28 * 30 + 8 * 90) * 256 + 32768) >> 16


# ---- the boundary -------------------------------------------------------------------------------------------------------------------
def test_boundary_squares():
    d = np.zeros((32, 32), dtype=np.uint8)
    d[15, 16] = 1
    want = np.zeros((32, 32), dtype=bool)
    want[11:20, 12:21] = True
    assert np.array_equal(FR.boundary(d), want) and want.sum() == 81
    for y, x, ys, xs in ((0, 0, slice(0, 5), slice(0, 5)), (31, 0, slice(27, 32), slice(0, 5)), (0, 31, slice(0, 5), slice(27, 32)),
                         (31, 31, slice(27, 32), slice(27, 32))):
        d = np.zeros((32, 32), dtype=np.uint8)
        d[y, x] = 1
        want = np.zeros((32, 32), dtype=bool)
        want[ys, xs] = True
        assert np.array_equal(FR.boundary(d), want) and want.sum() == 25
    assert not FR.boundary(np.ones((32, 32), dtype=np.uint8)).any()   # the border is neutral: no boundary along it
    assert not FR.boundary(np.zeros((32, 32), dtype=np.uint8)).any()
    assert not FR.boundary(np.ones((1, 1), dtype=bool)).any() and not FR.boundary(np.ones((3, 2), dtype=bool)).any()
    hole = np.ones((32, 32), dtype=bool)  # one clear pixel in a set mask: the same square
    hole[15, 16] = False
    assert FR.boundary(hole).sum() == 81


def test_boundary_is_two_iterations_of_a_5x5_box():
    rs = np.random.RandomState(3)
    d = (rs.rand(40, 37) < 0.02).astype(np.uint8)
    dil = maximum5(maximum5(d, 0), 0)
    ero = minimum5(minimum5(d, 1), 1)
    assert np.array_equal(FR.boundary(d), dil != ero)


def maximum5(a, cval):
    from scipy.ndimage import maximum_filter
    return maximum_filter(a, size=5, mode="constant", cval=cval)


def minimum5(a, cval):
    from scipy.ndimage import minimum_filter
    return minimum_filter(a, size=5, mode="constant", cval=cval)


# ---- finish -------------------------------------------------------------------------------------------------------------------------
def test_finish_composition():
    from oracle import image_ref as IR
    canvas = LR.gradient_rects(40, 50, 3)
    styled = np.ascontiguousarray(255 - canvas[:, ::-1])
    m = LR.enhanced_weight_map(canvas)
    plain = FR.finish(canvas, styled, m["weight"], m["detail"], enhance=False, smooth=False)
    assert np.array_equal(plain, IR.blend_weight_map(canvas, styled, m["weight"]))
    e = FR.finish(canvas, styled, m["weight"], None, enhance=True, smooth=False)
    out = FR.finish(canvas, styled, m["weight"], m["detail"])
    b = FR.boundary(m["detail"])
    assert 0.05 < b.mean() < 0.95
    assert np.array_equal(out[~b], e[~b]) and (out[b] != e[b]).any()
    # the reference's statement: a float64 0.5 * a + 0.5 * b assigned into a uint8 array truncates
    res = e.copy()
    res[np.where(b)] = e[np.where(b)] * 0.5 + FR.blur7(e)[np.where(b)] * 0.5
    assert np.array_equal(out, res)
    with pytest.raises(NotImplementedError):
        FR.finish(canvas, styled, m["weight"], m["detail"], enhance=False, smooth=True)


# ---- the C ABI, host side -----------------------------------------------------------------------------------------------------------
def test_entry_points_validate_on_the_host(lib):
    from mstg_hip import _lib
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.mstg_local_style_finish(None, None, None, None, 1, 8, 8, 1, 1, None, None) == -1
    assert lib.mstg_local_style_finish(4096, 8192, 12288, 16384, 1, 8, 8, 0, 1, 20480, None) == -5  # smooth without enhance_colors
    msg = lib.mstg_last_error()
    assert b"smooth without enhance_colors" in msg and b"float64" in msg
    assert lib.mstg_local_style_finish(4096, 8192, 12288, None, 1, 8, 8, 1, 1, 20480, None) == -1 and b"detail" in lib.mstg_last_error()
    assert lib.mstg_local_style_finish(4096, 8192, 12288, 16384, 1, 8, 8, 1, 1, 4096 + 100, None) == -1 and b"overlaps" in lib.mstg_last_error()
    assert lib.mstg_local_style_finish(4096, 8192, 12288 + 4, 16384, 1, 8, 8, 1, 1, 20480, None) == -2
    assert lib.mstg_local_style_finish(4096, 8192, 12288, 16384, 0, 8, 8, 1, 1, 20480, None) == -1
    need = lib.mstg_local_style_enhanced_workspace_bytes(3, 256, 256)
    assert need >= 3 * 256 * 256 * (8 + 1) + lib.mstg_local_style_workspace_bytes(3, 256, 256)
    assert lib.mstg_local_style_enhanced_workspace_bytes(1, 385, 384) == 0 and b"385 x 384" in lib.mstg_last_error()
    assert lib.mstg_local_style_enhanced(4096, 8192, 1, 385, 384, 0.8, 1.0, 0.59, 1, 1, 1 << 30, 1 << 28, 1 << 27, None) == -5
    assert b"385 x 384" in lib.mstg_last_error()
    assert lib.mstg_local_style_enhanced(4096, 8192, 1, 8, 8, 0.8, 1.0, 0.59, 0, 1, 1 << 30, 1 << 28, 1 << 20, None) == -5
    assert b"smooth without enhance_colors" in lib.mstg_last_error()
    assert lib.mstg_local_style_enhanced(4096, 8192, 1, 8, 8, 0.8, 1.0, 0.59, 1, 1, 1 << 30, 1 << 28, 16, None) == -4


def test_python_surface_has_the_keywords():
    import inspect
    from mstg_hip import image as dimg
    for fn in (dimg.process_local_style, dimg.process_local_style_batch):
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ["enhance_colors", "smooth"]
        p = inspect.signature(fn).parameters
        assert p["enhance_colors"].default is True and p["smooth"].default is True
    assert list(inspect.signature(dimg.local_style_finish).parameters) == ["canvas_u8", "styled_u8", "weight_map", "detail_mask", "enhance_colors",
                                                                           "smooth"]
