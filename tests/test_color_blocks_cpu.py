"""CPU: the colour-block repair (csrc/color_blocks.hip, mstg_hip.image.fix_color_blocks, improved_smooth.py) up to the launch.  The
host-built tables of the library are compared bit for bit with the numpy restatement the GPU tests use (tests/color_blocks_ref.py);
the restatement's Lab path is pinned with the constants of include/mstg_hip.h and against CIE Lab in float64 over all 2^24 colours;
its pixel-subset bilateral filter equals its full one; the share of bytes on which other evaluations of the floating-point steps
would differ from the definition at radius 90 is measured and printed (DESIGN.md 3d quotes it); the new C-ABI entry points refuse
by name on the host; and the drop-in module imports without OpenCV.  The restatement has not been compared with an OpenCV binary.
No kernel is launched here."""
import inspect
import math
import sys

import numpy as np
import pytest

import color_blocks_ref as CR
import standard_mode_ref as SR


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


# ---- tables and constants -----------------------------------------------------------------------------------------------------------
def test_lab_tables_equal_the_restatement(lib):
    from mstg_hip import _lib
    t = np.full(_lib.LAB_TABLE_U16, 0xffff, dtype=np.uint16)
    assert lib.mstg_lab_tables(t.ctypes.data) == 0
    gamma, cbrt, C = CR.lab_tables()
    assert np.array_equal(t[:256], gamma) and np.array_equal(t[256:3328], cbrt) and np.array_equal(t[3328:3337].reshape(3, 3), C)
    assert (t[3337:] == 0).all()
    assert lib.mstg_lab_tables(None) == -1


def test_lab_constants():
    gamma, cbrt, C = CR.lab_tables()
    assert C.tolist() == [[1777, 1541, 778], [871, 2929, 296], [73, 448, 3575]] and (C.sum(axis=1) == 4096).all()
    assert gamma.max() == 2040 and cbrt.max() == 37555 and gamma[0] == 0
    assert (2040 * 4096 + 2048) >> 12 < 3072  # the largest index into cbrt
    want = {(255, 255, 255): (128, 128), (0, 0, 0): (128, 128), (255, 0, 0): (208, 195), (0, 255, 0): (42, 211), (0, 0, 255): (207, 20)}
    for rgb, ab in want.items():
        a, b = CR.lab_ab(np.array(rgb, dtype=np.uint8))
        assert (int(a), int(b)) == ab, rgb


def test_lab_ab_against_cie_lab_all_colours(capsys):
    """the reference here is CIE Lab in float64, not the code under test: the integer path stays within 3 levels (a) and 2 (b)"""
    tables = CR.lab_tables()
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    worst = [0.0, 0.0]
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], axis=-1)
        ia, ib = CR.lab_ab(rgb, tables)
        fa, fb = CR.lab_ab_float64(rgb)
        worst = [max(worst[0], float(np.abs(ia - fa).max())), max(worst[1], float(np.abs(ib - fb).max()))]
    with capsys.disabled():
        print(f"\n  8-bit Lab against float64 CIE Lab over 2^24 colours: a within {worst[0]:.2f}, b within {worst[1]:.2f}")
    assert worst[0] <= 3 and worst[1] <= 2


def test_lab_table_entries_are_far_from_ties(capsys):
    """one ulp of a double pow / cbrt result moves an entry of magnitude 2^15 by 7e-12: with every unrounded value more than 1e-9
    from a tie the C library's and numpy's last bit cannot change an entry.  A float32 evaluation (OpenCV 4 builds the tables in
    32-bit soft-float) is measured: include/mstg_hip.h records the counts."""
    gu, cu = CR.lab_tables_unrounded()
    margin = min(float(np.abs(np.abs(v - np.floor(v)) - 0.5).min()) for v in (gu, cu))
    g, c, _ = CR.lab_tables()
    g32, c32, _ = CR.lab_tables(np.float32)
    dg, dc = np.abs(g32 - g), np.abs(c32 - c)
    with capsys.disabled():
        print(f"\n  Lab tables: smallest distance from a tie {margin:.3g}; a float32 evaluation changes {int((dg != 0).sum())} of 256 gamma "
              f"entries and {int((dc != 0).sum())} of 3072 cbrt entries (max {int(max(dg.max(), dc.max()))})")
    assert margin > 1e-9
    assert (int((dg != 0).sum()), int((dc != 0).sum())) == (0, 2) and max(dg.max(), dc.max()) <= 1  # the counts the header records


def test_radius_taps_and_sizes(lib):
    from mstg_hip import _lib
    assert len(CR.bilateral_taps(90)) == 25445
    assert CR.bilateral_radius(0, 60) == 90 and CR.bilateral_radius(0, 61) == 92 and CR.bilateral_radius(9, 60) == 4
    assert CR.bilateral_radius(0, 0.1) == 1 and CR.bilateral_radius(1, 5) == 1
    assert 0.4 * 255 == 102.0
    assert CR.detail_ksize(3) == 25 and CR.detail_ksize(4) == 33
    from mstg_hip import image as dimg
    assert dimg._detail_ksize(3) == 25 and dimg._detail_ksize(3.0) == 25 and dimg._detail_ksize(4) == 33
    table = np.zeros(_lib.BILATERAL_WIDE_TABLE_FLOATS, dtype=np.float32)
    assert lib.mstg_bilateral_wide_tables(0, 102.0, 60.0, table.ctypes.data) == 90
    gc, gs = -0.5 / (102.0 * 102.0), -0.5 / (60.0 * 60.0)
    assert np.array_equal(table[:768], np.array([math.exp(t * t * gc) for t in range(768)]).astype(np.float32))
    assert np.array_equal(table[768:], np.array([math.exp(q * gs) for q in range(8101)]).astype(np.float32))
    for d in (3, 5, 7, 9):  # the same weights as the existing tables, tap by tap
        old = np.zeros(_lib.BILATERAL_COLOR_WEIGHTS + _lib.BILATERAL_MAX_TAPS, dtype=np.float32)
        n = lib.mstg_bilateral_tables(d, 75.0, 75.0, old.ctypes.data)
        assert lib.mstg_bilateral_wide_tables(d, 75.0, 75.0, table.ctypes.data) == d // 2
        taps = CR.bilateral_taps(d // 2)
        assert n == len(taps) and np.array_equal(old[:768], table[:768])
        assert np.array_equal(old[768:768 + n], np.array([table[768 + i * i + j * j] for i, j in taps]))
        assert (table[768 + (d // 2) ** 2 + 1:] == 0).all()


def test_refusals_by_name_on_the_host(lib):
    from mstg_hip import _lib
    table = np.zeros(_lib.BILATERAL_WIDE_TABLE_FLOATS, dtype=np.float32)
    assert lib.mstg_bilateral_wide_tables(0, 102.0, 61.0, table.ctypes.data) == -5 and b"radius = 92 " in lib.mstg_last_error()
    assert lib.mstg_bilateral_wide_tables(183, 102.0, 60.0, table.ctypes.data) == -5 and b"radius = 91 " in lib.mstg_last_error()
    assert lib.mstg_bilateral_wide_u8(1, 1, 8, 8, 91, 1, 1, None) == -5 and b"radius = 91 " in lib.mstg_last_error()
    assert lib.mstg_color_block_mask(1, 1, 8, 8, 1, 30.0, 10, 1, 1, 64, None) == -5 and b"kernel_size = 10 " in lib.mstg_last_error()
    assert lib.mstg_color_block_mask(1, 1, 8, 8, 1, 30.0, 33, 1, 1, 64, None) == -5 and b"kernel_size = 33 " in lib.mstg_last_error()
    assert lib.mstg_detail_blend_u8(1, 1, 1, 8, 8, 1, 33, 0.9, 0.1, 0.5, 1, 1, 0, None) == -5 and b"ksize = 33 " in lib.mstg_last_error()
    assert lib.mstg_detail_blend_u8(1, 1, 1, 8, 8, 1, 24, 0.9, 0.1, 0.5, 1, 1, 0, None) == -5 and b"ksize = 24 " in lib.mstg_last_error()
    assert lib.mstg_color_correct_u8(1, 1, 1, 5000, 5000, 50, 1, 1, 0, None) == -5 and b"H * W * 255" in lib.mstg_last_error()
    assert lib.mstg_color_block_fix(1, None, 1, 8, 8, 1, 30.0, 11, 50, 91, 1, None, 25, 0.9, 0.1, 0.5, 1, 1, 0, None) == -5
    assert b"radius = 91 " in lib.mstg_last_error()
    assert lib.mstg_color_block_fix_workspace_bytes(1, 0, 8, 0) == 0
    small, large = lib.mstg_color_block_fix_workspace_bytes(2, 67, 93, 0), lib.mstg_color_block_fix_workspace_bytes(2, 67, 93, 1)
    assert 2 * 67 * 93 * (1 + 1 + 12 + 3) <= small < large
    # out must not overlap an input: the same pointer for in and out
    assert lib.mstg_bilateral_wide_u8(4096, 1, 8, 8, 90, 8192, 4096, None) == -1 and b"overlaps" in lib.mstg_last_error()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_pixel_subset_bilateral_equals_the_full_one():
    imgs = np.stack([SR.image(kind, 40, 33, seed=3 + i) for i, kind in enumerate(("noise", "blocky", "gradient"))])
    full = CR.bilateral_wide(imgs, 0, 102.0, 8)  # radius 12: mirrored more than once along neither side, taps outside on all four
    assert full.shape == imgs.shape and CR.bilateral_radius(0, 8) == 12
    coords = [(0, 0), (0, 32), (39, 0), (39, 32), (20, 16), (11, 12), (12, 13), (13, 11), (28, 20)]
    sub = CR.bilateral_wide(imgs, 0, 102.0, 8, coords)
    assert sub.shape == (3, len(coords), 3)
    for k, (y, x) in enumerate(coords):
        assert np.array_equal(sub[:, k], full[:, y, x]), (y, x)
    for d, sc, ss in ((9, 75, 75), (5, 10, 3)):  # and the full one equals the existing restatement where both are defined
        assert np.array_equal(CR.bilateral_wide(imgs[:1], d, sc, ss)[0], SR.bilateral(imgs[0], d, sc, ss))


def test_bilateral_other_evaluations_measured_at_radius_90(capsys):
    """the definition against an unfused float32 sum, a division by wsum and plain float64 at radius 90, on 192 pixels of three 96 x
    128 images: shares printed.  Asserted is 'never more than one grey level': a float32 sum of 25 445 non-negative terms is off by
    at most 25 445 * 2^-24 = 0.0016 of its value, 0.39 levels, in either evaluation."""
    imgs = np.stack([SR.image(kind, 96, 128, seed=21 + i) for i, kind in enumerate(("noise", "blocky", "gradient"))])
    rs = np.random.RandomState(5)
    coords = [(int(y), int(x)) for y, x in zip(rs.randint(0, 96, 64), rs.randint(0, 128, 64))]
    out = CR.bilateral_wide_all(imgs, 0, 0.4 * 255, 60, coords, others=True)
    e = out["definition"].astype(np.int32)
    row = {}
    for name in ("unfused", "divide", "float64"):
        diff = np.abs(e - out[name].astype(np.int32))
        row[name] = (float((diff != 0).mean()), int(diff.max()))
        assert diff.max() <= 1, name
    with capsys.disabled():
        print("\n  bilateral radius 90, bytes that differ from the definition: " +
              ", ".join(f"{k} {100 * v[0]:.2f} % (max {v[1]})" for k, v in row.items()))


def test_mask_branches_and_correction_closed_forms():
    const = SR.image("constant", 20, 30, seed=1)
    assert not CR.block_mask(const).any()
    assert CR.block_mask(SR.image("noise", 20, 30, seed=2)).all()
    share = CR.block_mask(CR.blocks(67, 93, 3)).mean()
    assert 0.05 < share < 0.95
    # one edge pixel dilates to the box clipped to the image
    e = np.zeros((9, 12), dtype=bool)
    e[0, 11] = True
    d = CR.dilate_box(e, 5)
    assert d.sum() == 9 and d[:3, 9:].all()
    # correction: a constant image stays; a flagged pixel of a two-level image moves halfway to the window mean, truncated
    m = np.ones((20, 30), dtype=bool)
    assert np.array_equal(CR.correct(const, m), const)
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    img[:, 2:] = 101
    out = CR.correct(img, np.ones((4, 4), dtype=bool), radius=50)  # every window is the whole image: mean 50.5
    assert (out[:, :2] == 25).all() and (out[:, 2:] == 75).all()  # 25.25 and 75.75 truncated
    none = CR.correct(img, np.zeros((4, 4), dtype=bool))
    assert np.array_equal(none, img)


def test_detail_blend_closed_forms():
    const = SR.image("constant", 9, 11, seed=4)
    other = SR.image("noise", 9, 11, seed=5)
    # the blur of a constant plane is the constant up to rounding: the detail is tiny and the blend lands next to the byte
    out = CR.detail_blend(const, const, alpha=0.1, beta=0.5).astype(int)
    assert np.abs(out - const.astype(int)).max() <= 1
    # beta = 0 and alpha = 0: the image itself
    assert np.array_equal(CR.detail_blend(other, const, alpha=0.0, beta=0.0), other)


# ---- the drop-in module -------------------------------------------------------------------------------------------------------------
def test_improved_smooth_imports_without_cv2():
    import improved_smooth as IS
    assert "cv2" not in sys.modules
    want = {"adaptive_color_correction": ["img", "blocks_detected", "radius"], "detect_color_blocks": ["img", "threshold", "kernel_size"],
            "edge_preserving_smoothing": ["img", "sigma_s", "sigma_r"], "detail_enhancing_blend": ["img", "original", "alpha", "beta"],
            "fix_color_blocks_improved": ["input_img_path", "original_img_path", "output_img_path"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(IS, name)).parameters) == params, name
    d = {k: v.default for k, v in inspect.signature(IS.detail_enhancing_blend).parameters.items()}
    assert (d["alpha"], d["beta"]) == (0.3, 1.5)
    d = {k: v.default for k, v in inspect.signature(IS.edge_preserving_smoothing).parameters.items()}
    assert (d["sigma_s"], d["sigma_r"]) == (60, 0.4)
    assert inspect.signature(IS.detect_color_blocks).parameters["threshold"].default == 30
    assert inspect.signature(IS.adaptive_color_correction).parameters["radius"].default == 50
