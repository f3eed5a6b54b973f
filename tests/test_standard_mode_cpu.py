"""CPU: the finish of the application's standard mode (csrc/standard_mode.hip, mstg_hip.image.standard_finish) up to the launch.
The numpy restatement the GPU tests compare with (tests/standard_mode_ref.py) is pinned against scipy's median, the blur of
tests/local_style_finish_ref.py and closed forms; the host-built tables of the library are compared bit for bit with math.exp and
the numpy expressions; the share of bytes on which other evaluations of the floating-point steps would differ from the definition
is measured and printed (DESIGN.md 3d quotes it; asserted is 'never more than one grey level'); and the new C-ABI entry points
validate on the host.  The restatement has not been compared with an OpenCV binary.  No kernel is launched here."""
import math
from fractions import Fraction

import numpy as np
import pytest

import local_style_finish_ref as FR
import standard_mode_ref as SR

NEW_SYMBOLS = ["mstg_bilateral_tables", "mstg_standard_color_lut", "mstg_median3_u8", "mstg_bilateral_u8", "mstg_lut_u8",
               "mstg_gaussian_u8", "mstg_standard_finish_workspace_bytes", "mstg_standard_finish"]
SHAPES = [(1, 1), (1, 7), (2, 5), (7, 9), (33, 65)]


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


# ---- the integer steps --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_median_against_scipy(shape):
    from scipy.ndimage import median_filter
    for kind in SR.KINDS:
        img = SR.image(kind, *shape, seed=3)
        assert np.array_equal(SR.median3(img), median_filter(img, size=(3, 3, 1), mode="nearest")), kind


def test_median_closed_forms():
    img = np.zeros((3, 3, 3), dtype=np.uint8)
    img[..., 0] = np.arange(9).reshape(3, 3) * 10  # centre window = all nine samples: median 40
    assert SR.median3(img)[1, 1, 0] == 40
    assert SR.median3(img)[0, 0, 0] == 10  # corner: 0 0 10 0 0 10 30 30 40 sorted -> the fifth is 10
    assert np.array_equal(SR.median3(np.array([[[7, 8, 9]]], dtype=np.uint8)), [[[7, 8, 9]]])


@pytest.mark.parametrize("shape", SHAPES + [(67, 93)])
def test_blur7_against_the_existing_restatement(shape):
    for kind in SR.KINDS:
        img = SR.image(kind, *shape, seed=5)
        assert np.array_equal(SR.gaussian(img, 7), FR.blur7(img)), kind


def test_blur_taps_and_small_sizes():
    for k, taps in SR.GAUSS_TAPS.items():
        assert len(taps) == k and sum(taps) == 256 and taps == taps[::-1]
        for v in (0, 1, 128, 255):  # a constant image is a fixed point at every size, shorter than the radius included
            for shape in ((1, 1), (2, 3), (9, 11)):
                assert (SR.gaussian(np.full(shape + (3,), v, dtype=np.uint8), k) == v).all()
        img = np.zeros((15, 17, 3), dtype=np.uint8)  # a single bright pixel spreads as the tap products
        img[7, 8] = 255
        want = np.zeros((15, 17), dtype=np.int64)
        r = k // 2
        want[7 - r:8 + r, 8 - r:9 + r] = (np.outer(taps, taps) * 255 + 32768) >> 16
        assert np.array_equal(SR.gaussian(img, k)[..., 1], want)
    row = np.array([[[10] * 3, [200] * 3]], dtype=np.uint8)  # d c b | a b | a b a: the taps at -1 .. 1 read b a b
    assert SR.gaussian(row, 3)[0, :, 0].tolist() == [(128 * 10 + 128 * 200 + 128) >> 8, (128 * 200 + 128 * 10 + 128) >> 8]
    with pytest.raises(NotImplementedError, match="smooth_level 4"):
        SR.gaussian(row, 9)


def test_reflect101_iterates():
    assert SR.reflect101(np.arange(-4, 7), 3).tolist() == [0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2]
    assert SR.reflect101(np.arange(-4, 6), 2).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert SR.reflect101(np.arange(-4, 5), 1).tolist() == [0] * 9


# ---- the host-built tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [(9, 75.0, 75.0), (5, 10.0, 3.0), (3, 0.0, -1.0), (7, 25.5, 1.25)])
def test_bilateral_tables_bit_for_bit(lib, params):
    d, sc, ss = params
    table = np.full(768 + 49, -1, dtype=np.float32)
    taps = lib.mstg_bilateral_tables(d, sc, ss, table.ctypes.data)
    assert taps == {3: 5, 5: 13, 7: 29, 9: 49}[d]
    sc, ss = (sc if sc > 0 else 1), (ss if ss > 0 else 1)  # a sigma <= 0 counts as 1
    radius = max(d // 2, 1)
    color = [np.float32(math.exp(t * t * (-0.5 / (sc * sc)))) for t in range(768)]
    space = [np.float32(math.exp((i * i + j * j) * (-0.5 / (ss * ss)))) for i in range(-radius, radius + 1)
             for j in range(-radius, radius + 1) if math.sqrt(i * i + j * j) <= radius]
    assert len(space) == taps
    assert table[:768].view(np.uint32).tolist() == np.array(color, dtype=np.float32).view(np.uint32).tolist()
    assert table[768:768 + taps].view(np.uint32).tolist() == np.array(space, dtype=np.float32).view(np.uint32).tolist()
    assert (table[768 + taps:] == 0).all()
    _, rs, rc = SR.bilateral_tables(d, *params[1:])  # and the restatement's own tables
    assert np.array_equal(rs.view(np.uint32), table[768:768 + taps].view(np.uint32)) and np.array_equal(rc.view(np.uint32), table[:768].view(np.uint32))
    if d == 9:
        assert table[768 + 24] == 1.0 and table[0] == 1.0  # the centre tap and a zero colour distance weigh 1
        assert 0 < table[765] < 1e-22  # exp(-52.02): the smallest colour weight the filter can meet, still a normal float


def test_color_lut_against_numpy(lib):
    v = np.arange(256)
    lut = np.zeros(768, dtype=np.uint8)
    assert lib.mstg_standard_color_lut(0, lut.ctypes.data) == 0
    assert np.array_equal(lut[:256], np.clip(v * 1.1, 0, 255).astype(np.uint8))
    assert np.array_equal(lut[256:512], np.clip(v * 1.05, 0, 255).astype(np.uint8))
    assert np.array_equal(lut[512:], v)
    assert np.array_equal(lut.reshape(3, 256), SR.color_lut("photo_to_monet"))
    assert lut[100] == 110 and lut[256 + 100] == 105 and lut[232] == 255 and lut[231] == 254
    assert lib.mstg_standard_color_lut(1, lut.ctypes.data) == 0
    want = np.clip(np.rint(np.abs((v.astype(np.float32).astype(np.float64) * np.float64(np.float32(1.1)) + 5.0).astype(np.float32))), 0, 255)
    for c in range(3):
        assert np.array_equal(lut[256 * c:256 * (c + 1)], want.astype(np.uint8))
    assert np.array_equal(lut.reshape(3, 256), SR.color_lut("monet_to_photo"))
    assert lut[0] == 5 and lut[100] == 115 and lut[255] == 255
    for x in v:  # the float64 emulation is the fused operation: exact with rationals
        exact = Fraction(float(np.float32(x))) * Fraction(float(np.float32(1.1))) + 5
        assert Fraction(float(np.float64(np.float32(x)) * np.float64(np.float32(1.1)) + 5.0)) == exact


def test_color_lut_other_evaluations_measured(capsys):
    v = np.arange(256)
    e = SR.scale_abs_u8(v).astype(int)
    du, d64 = np.abs(e - SR.scale_abs_u8_unfused(v).astype(int)), np.abs(e - SR.scale_abs_u8_float64(v).astype(int))
    with capsys.disabled():
        print(f"\n  convertScaleAbs table: unfused float32 changes {int((du != 0).sum())} of 256 entries (max {du.max()}), "
              f"float64 changes {int((d64 != 0).sum())} (max {d64.max()})")
    assert du.max() <= 1 and d64.max() <= 1


# ---- the bilateral restatement ------------------------------------------------------------------------------------------------------
def test_fma_emulation_is_one_rounding():
    rs = np.random.RandomState(0)
    a = rs.randint(0, 256, size=400).astype(np.float32)
    b = (rs.rand(400) * 2.0 ** rs.randint(-80, 1, size=400)).astype(np.float32)
    c = (rs.rand(400) * 2.0 ** rs.randint(-20, 14, size=400)).astype(np.float32)
    got = SR.fma_f32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        assert abs(Fraction(float(g)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)), (x, y, z)
    # a sum whose float64 rounding lands exactly on a float32 tie although the exact value lies below it: (1 + 2^-23) * 2^-24 *
    # (1 - 2^-23) + (1 + 2^-23) = 1 + 2^-23 + 2^-24 - 2^-70.  Rounded twice it would go to the even neighbour 1 + 2^-22.
    one = np.float32(1) + np.float32(2.0 ** -23)
    stats = {}
    r = SR.fma_f32(np.array([one]), np.array([np.float32(2.0 ** -24) * (np.float32(1) - np.float32(2.0 ** -23))]), np.array([one]), stats)
    assert r[0] == one and stats == {"fma": 1, "inexact": 1, "fired": 1}
    naive = (np.float64(one) * np.float64(np.float32(2.0 ** -24) * (np.float32(1) - np.float32(2.0 ** -23))) + np.float64(one)).astype(np.float32)
    assert naive == np.float32(1) + np.float32(2.0 ** -22)


def test_bilateral_closed_forms():
    for shape in ((1, 1), (3, 5), (12, 9)):  # a constant image is a fixed point, sides below the radius included
        img = np.full(shape + (3,), 77, dtype=np.uint8)
        img[..., 1] = 200
        assert np.array_equal(SR.bilateral(img), img) and np.array_equal(SR.bilateral(img, 5, 10, 3), img)
    # one bright pixel on black, sigma_color tiny: the colour weight of every other sample is 0, so nothing moves
    img = np.zeros((11, 11, 3), dtype=np.uint8)
    img[5, 5] = 255
    assert np.array_equal(SR.bilateral(img, 9, 1, 75), img)
    # a huge sigma_color makes it the plain spatial mean over the 49 taps: out = rint(255 * w_centre / sum(space))
    _, space, _ = SR.bilateral_tables(9, 1e9, 75)
    got = SR.bilateral(img, 9, 1e9, 75)
    assert abs(int(got[5, 5, 0]) - round(255 * float(space[24]) / float(space.astype(np.float64).sum()))) <= 1
    assert got[5, 5, 0] == got[5, 1, 0] == got[1, 5, 0] and got[1, 1, 0] == 0  # inside the disc of radius 4, outside it


@pytest.mark.parametrize("kind", SR.KINDS)
def test_bilateral_other_evaluations_measured(kind, capsys):
    """the definition against an unfused float32 sum, a division by wsum and plain float64, at 256 x 256, d = 9, (75, 75): shares
    printed, 'never more than one grey level' asserted (also for d = 5, (10, 3) at 64 x 64)"""
    for (d, sc, ss), size in (((9, 75, 75), 256), ((5, 10, 3), 64)):
        stats = {}
        out = SR.bilateral_all(SR.image(kind, size, size, seed=100), d, sc, ss, stats)
        e = out["definition"].astype(np.int32)
        row = {}
        for name in ("unfused", "divide", "float64"):
            diff = np.abs(e - out[name].astype(np.int32))
            row[name] = (float((diff != 0).mean()), int(diff.max()))
        with capsys.disabled():
            print(f"\n  {kind:9s} d={d} ({sc}, {ss}) {size}x{size}: " + "  ".join(f"{n} differs on {100 * s:.4f} % (max {m})" for n, (s, m) in row.items()) +
                  f"  | fma: {stats['inexact']} of {stats['fma']} float64 sums inexact, correction changed {stats['fired']}")
        assert all(m <= 1 for _, m in row.values()), row


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
def test_chain_composition_and_switches():
    canvas, styled = SR.image("gradient", 20, 27, 1), SR.image("blocky", 20, 27, 2)
    full = SR.standard_finish(canvas, styled, "photo_to_monet")
    x = np.clip(styled * (1 - 0.3) + canvas * 0.3, 0, 255).astype(np.uint8)
    x = SR.apply_lut(SR.bilateral(SR.median3(x)), SR.color_lut("photo_to_monet"))
    assert np.array_equal(full, SR.gaussian(x, 7))
    assert np.array_equal(SR.standard_finish(canvas, styled, "monet_to_photo", blend_ratio=0, fix_blocks=False, enhance_colors=False,
                                             smooth_level=0), styled)
    assert np.array_equal(SR.standard_finish(canvas, styled, "monet_to_photo", adaptive_smooth=False),
                          SR.standard_finish(canvas, styled, "monet_to_photo", smooth_level=0))
    with pytest.raises(ValueError):
        SR.standard_finish(canvas, styled, "monet")
    with pytest.raises(NotImplementedError, match="smooth_level 4"):
        SR.standard_finish(canvas, styled, "photo_to_monet", smooth_level=4)


# ---- the C ABI, host side -----------------------------------------------------------------------------------------------------------
def test_entry_points_validate_on_the_host(lib):
    from mstg_hip import _lib
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    IN, OUT, TAB, LUT, WS = 4096, 1 << 20, 1 << 24, 1 << 25, 1 << 26  # never dereferenced: every call below is refused on the host
    table = np.zeros(768 + 49, dtype=np.float32)
    # d outside 3, 5, 7, 9: by name, before anything else
    for d in (11, 0, -1, 4, 1):
        assert lib.mstg_bilateral_tables(d, 75.0, 75.0, table.ctypes.data) == -5 and f"d = {d} ".encode() in lib.mstg_last_error()
        assert lib.mstg_bilateral_u8(IN, 1, 8, 8, d, TAB, OUT, None) == -5 and f"d = {d} ".encode() in lib.mstg_last_error()
    assert lib.mstg_standard_finish(IN, IN + 4096, 1, 8, 8, 0.7, 0.3, 1, 11, TAB, LUT, 3, OUT, WS, 1 << 20, None) == -5
    assert b"d = 11 " in lib.mstg_last_error()
    assert lib.mstg_bilateral_tables(9, 75.0, 75.0, None) == -1
    # blur levels above 3: by name, never approximated
    assert lib.mstg_gaussian_u8(IN, 1, 8, 8, 9, OUT, None) == -5
    assert b"smooth_level = 4" in lib.mstg_last_error() and b"ksize 9" in lib.mstg_last_error()
    assert lib.mstg_standard_finish(IN, IN + 4096, 1, 8, 8, 0.7, 0.3, 1, 9, TAB, LUT, 4, OUT, WS, 1 << 20, None) == -5
    assert b"smooth_level = 4" in lib.mstg_last_error()
    assert lib.mstg_gaussian_u8(IN, 1, 8, 8, 15, OUT, None) == -5 and b"smooth_level = 7" in lib.mstg_last_error()
    for k in (4, 1, 0, -3):
        assert lib.mstg_gaussian_u8(IN, 1, 8, 8, k, OUT, None) == -1
    assert lib.mstg_standard_finish(IN, IN + 4096, 1, 8, 8, 0.7, 0.3, 1, 9, TAB, LUT, -1, OUT, WS, 1 << 20, None) == -1
    # null pointers
    assert lib.mstg_median3_u8(None, 1, 8, 8, OUT, None) == -1 and lib.mstg_median3_u8(IN, 1, 8, 8, None, None) == -1
    assert lib.mstg_bilateral_u8(IN, 1, 8, 8, 9, None, OUT, None) == -1 and lib.mstg_bilateral_u8(None, 1, 8, 8, 9, TAB, OUT, None) == -1
    assert lib.mstg_lut_u8(IN, 1, 8, 8, None, OUT, None) == -1 and lib.mstg_gaussian_u8(None, 1, 8, 8, 7, OUT, None) == -1
    assert lib.mstg_standard_color_lut(0, None) == -1
    assert lib.mstg_standard_finish(None, IN, 1, 8, 8, 0.7, 0.3, 1, 9, TAB, LUT, 3, OUT, WS, 1 << 20, None) == -1  # a blend needs the canvas
    assert lib.mstg_standard_finish(IN, None, 1, 8, 8, 0.7, 0.3, 1, 9, TAB, LUT, 3, OUT, WS, 1 << 20, None) == -1
    assert lib.mstg_standard_finish(IN, IN + 4096, 1, 8, 8, 0.7, 0.3, 1, 9, None, LUT, 3, OUT, WS, 1 << 20, None) == -1
    assert b"bilateral table" in lib.mstg_last_error()
    # aliasing: out must not overlap an input of a neighbourhood stage
    nb = 2 * 8 * 8 * 3
    for off in (0, nb - 1, -(nb - 1)):
        assert lib.mstg_median3_u8(IN, 2, 8, 8, IN + off, None) == -1 and b"overlaps" in lib.mstg_last_error()
        assert lib.mstg_bilateral_u8(IN, 2, 8, 8, 9, TAB, IN + off, None) == -1 and b"overlaps" in lib.mstg_last_error()
        assert lib.mstg_gaussian_u8(IN, 2, 8, 8, 7, IN + off, None) == -1 and b"overlaps" in lib.mstg_last_error()
        assert lib.mstg_lut_u8(IN, 2, 8, 8, LUT, IN + off, None) == -1
    assert lib.mstg_standard_finish(IN, IN + 4096, 2, 8, 8, 0.7, 0.3, 1, 9, TAB, LUT, 3, IN + 8, WS, 1 << 20, None) == -1
    assert b"overlaps" in lib.mstg_last_error()
    assert lib.mstg_standard_finish(IN, IN + 4096, 2, 8, 8, 0.7, 0.3, 1, 9, TAB, LUT, 3, WS + 16, WS, 1 << 20, None) == -1
    # shapes, workspace, alignment, model type
    assert lib.mstg_median3_u8(IN, 0, 8, 8, OUT, None) == -1 and lib.mstg_bilateral_u8(IN, 1, 0, 8, 9, TAB, OUT, None) == -1
    need = lib.mstg_standard_finish_workspace_bytes(3, 67, 93)
    assert need >= 2 * 3 * 67 * 93 * 3 and need % 16 == 0
    assert lib.mstg_standard_finish_workspace_bytes(0, 8, 8) == 0
    assert lib.mstg_standard_finish(IN, IN + 4096, 1, 8, 8, 0.7, 0.3, 1, 9, TAB, LUT, 3, OUT, WS, 16, None) == -4
    assert lib.mstg_standard_finish(IN, IN + 4096, 1, 8, 8, 0.7, 0.3, 1, 9, TAB, LUT, 3, OUT, None, 1 << 20, None) == -4
    assert lib.mstg_standard_finish(IN, IN + 4096, 1, 8, 8, 0.7, 0.3, 1, 9, TAB, LUT, 3, OUT, WS + 4, 1 << 20, None) == -2
    assert lib.mstg_bilateral_u8(IN, 1, 8, 8, 9, TAB + 2, OUT, None) == -2
    lut = np.zeros(768, dtype=np.uint8)
    assert lib.mstg_standard_color_lut(2, lut.ctypes.data) == -1 and b"model_type = 2" in lib.mstg_last_error()


def test_python_surface():
    import inspect
    from mstg_hip import image as dimg
    sig = inspect.signature
    assert list(sig(dimg.median3_u8).parameters) == ["img"]
    assert [(n, p.default) for n, p in list(sig(dimg.bilateral_u8).parameters.items())[1:]] == [("d", 9), ("sigma_color", 75), ("sigma_space", 75)]
    assert list(sig(dimg.gaussian_u8).parameters) == ["img", "ksize"]
    options = [("blend_ratio", 0.3), ("fix_blocks", True), ("enhance_colors", True), ("smooth_level", 3), ("adaptive_smooth", True)]
    assert [(n, p.default) for n, p in list(sig(dimg.standard_finish).parameters.items())[3:]] == options
    assert list(sig(dimg.standard_finish).parameters)[:3] == ["canvas_u8", "styled_u8", "model_type"]
    assert [(n, p.default) for n, p in list(sig(dimg.process_standard).parameters.items())[3:]] == options + [("target", 256)]
    assert [(n, p.default) for n, p in list(sig(dimg.process_standard_batch).parameters.items())[3:]] == options + [("target", 256), ("batch_size", 64)]
    for fn in (dimg.standard_finish, dimg.process_standard, dimg.process_standard_batch):
        assert "strength" not in sig(fn).parameters  # the reference never reads it
    # a bad model_type is a ValueError before anything touches a device
    with pytest.raises(ValueError, match="model_type 'monet'"):
        dimg.standard_finish(None, None, "monet")
    with pytest.raises(ValueError, match="model_type"):
        dimg.process_standard(None, None, "photo2monet")
    with pytest.raises(ValueError, match="model_type"):
        dimg.process_standard_batch(None, [], None)
