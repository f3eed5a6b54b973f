"""CPU: the mixed-size comparison (csrc/compare.hip, mstg_hip.metrics.pair_metrics, the three three-way drop-ins) up to the launch.
The numpy restatement of the 8-bit cv2.resize (tests/cv_resize_ref.py, written from include/mstg_hip.h) is pinned with closed
forms, the host-only coefficient entry is held to it entry by entry, descriptor validation and the workspace query refuse by
name, and the drop-ins list and match file names the way the reference does.  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest

import cv_resize_ref as CV

EXTRA = [(300, 7), (7, 300), (1000, 999), (999, 1000), (4096, 1)]
PAIRS = [(s, d) for s in range(1, 41) for d in range(1, 41)] + EXTRA


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _entry(lib, s, d, horizontal):
    index, weights = np.full(d, -99, np.int32), np.full((d, 2), -99, np.int16)
    assert lib.mstg_cv_resize_coeffs(s, d, horizontal, index.ctypes.data, weights.ctypes.data) == 0, lib.mstg_last_error()
    return index, weights


# ---- the coefficient table ---------------------------------------------------------------------------------------------------------
def test_host_coefficients_equal_the_restatement_and_weights_sum_to_2048(lib):
    for s, d in PAIRS:
        for horizontal in (0, 1):
            index, weights = _entry(lib, s, d, horizontal)
            ref_i, ref_w = CV.coeffs(s, d, bool(horizontal))
            assert np.array_equal(index, ref_i) and np.array_equal(weights, ref_w), (s, d, horizontal)
            assert np.all(weights.astype(np.int32).sum(axis=1) == 2048), (s, d, horizontal)
            assert weights.min() >= 0
            if horizontal:
                assert index.min() >= 0 and index.max() <= s - 1
            else:
                assert index.min() >= -1 and index.max() <= s - 1  # the vertical index is not clamped; the rows are, when read


def test_coefficient_entry_refuses_bad_extents_by_name(lib):
    buf = np.zeros(8, np.int32)
    for s, d in [(0, 4), (4, 0), (-1, 4)]:
        assert lib.mstg_cv_resize_coeffs(s, d, 0, buf.ctypes.data, buf.ctypes.data) == -1
        assert f"{s} -> {d}".encode() in lib.mstg_last_error()
    assert lib.mstg_cv_resize_coeffs(4, 4, 0, None, buf.ctypes.data) == -1


# ---- the restatement, pinned with closed forms ------------------------------------------------------------------------------------
def test_resized_noise_stays_in_byte_range_before_the_cast():
    rs = np.random.RandomState(0)
    for s, d in [(1, 7), (2, 9), (7, 7), (22, 11), (23, 40), (129, 8), (64, 63), (64, 65), (300, 7), (7, 300), (40, 1)]:
        for img in (rs.randint(0, 256, size=(s, 37, 3)).astype(np.uint8), (rs.randint(0, 2, size=(s, 37, 3)) * 255).astype(np.uint8)):
            for size, src in (((53, d), img), ((d, 53), np.ascontiguousarray(img.transpose(1, 0, 2)))):
                wide = CV.resize_wide(src, size)
                assert wide.min() >= 0 and wide.max() <= 255, (s, d, size)
                assert wide.shape == (size[1], size[0], 3)


@pytest.mark.parametrize("shape", [(1, 1), (7, 7), (23, 37), (64, 5)])
def test_identity_at_equal_size(shape):
    img = np.random.RandomState(1).randint(0, 256, size=shape + (3,)).astype(np.uint8)
    assert np.array_equal(CV.resize(img, (shape[1], shape[0])), img)


@pytest.mark.parametrize("shape", [(2, 2), (22, 36), (8, 130)])
def test_exact_2x_reduction_is_the_rounded_mean_of_four(shape):
    img = np.random.RandomState(2).randint(0, 256, size=shape + (3,)).astype(np.uint8)
    v = img.astype(np.int64)
    want = (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2
    assert np.array_equal(CV.resize(img, (shape[1] // 2, shape[0] // 2)), want.astype(np.uint8))


@pytest.mark.parametrize("value", [0, 1, 127, 254, 255])
def test_a_constant_image_stays_constant(value):
    img = np.full((13, 29, 3), value, np.uint8)
    for size in [(7, 7), (64, 40), (29, 5), (3, 13), (58, 26)]:
        assert np.all(CV.resize(img, size) == value), (value, size)


# ---- C ABI: descriptors, validation, workspace; no launch ------------------------------------------------------------------------
def _descs(shapes, ptr=4096):
    """PairDesc array for [(ha, wa, hb, wb)], pointers never dereferenced"""
    from mstg_hip._lib import PairDesc
    arr = (PairDesc * len(shapes))()
    for d, (ha, wa, hb, wb) in zip(arr, shapes):
        d.a, d.b, d.ha, d.wa, d.hb, d.wb = ptr, ptr, ha, wa, hb, wb
    return arr


def test_pair_desc_layout_and_launch_constant():
    import re

    from conftest import ROOT
    from mstg_hip import _lib, metrics
    assert C.sizeof(_lib.PairDesc) == 56 == metrics._PAIR.itemsize
    assert [n for n, _ in _lib.PairDesc._fields_] == list(metrics._PAIR.names)
    text = open(os.path.join(ROOT, "include", "mstg_hip.h")).read()
    assert int(re.search(r"#define MSTG_PAIR_METRICS_LAUNCHES (\d+)", text).group(1)) == _lib.PAIR_METRICS_LAUNCHES == 2


def test_tiles_and_workspace_follow_the_image_metrics_decomposition(lib):
    from mstg_hip import metrics
    th, tw = metrics.TILE_H, metrics.TILE_W
    shapes = [(7, 7, 1, 1), (th + 7, tw + 7, 50, 300), (70, 130, 35, 65), (40, 7, 7, 40), (23, 37, 23, 37)]
    arr = _descs(shapes)
    n = lib.mstg_pair_metrics_tiles(arr, len(shapes), None, 0)
    per_pair = [lib.mstg_image_metrics_workspace_bytes(1, s[0], s[1]) // 32 for s in shapes]
    assert n == sum(per_pair) and per_pair == [1, 4, 8, 3, 2]
    assert [d.ntiles for d in arr] == per_pair and [d.tile0 for d in arr] == list(np.cumsum([0] + per_pair[:-1]))
    assert lib.mstg_pair_metrics_workspace_bytes(arr, len(shapes)) == 32 * n
    tiles = np.full((n, 4), -7, np.int32)
    assert lib.mstg_pair_metrics_tiles(arr, len(shapes), tiles.ctypes.data, n) == n
    assert lib.mstg_pair_metrics_tiles(arr, len(shapes), tiles.ctypes.data, n - 1) == -4
    want = []
    for i, s in enumerate(shapes):
        tx, ty = -(-(s[1] - 6) // tw), -(-(s[0] - 6) // th)
        want += [(i, y, x, 0) for y in range(ty) for x in range(tx)]  # row-major per pair, pair after pair
    assert tiles.tolist() == [list(t) for t in want]
    assert lib.mstg_pair_metrics_validate(arr, len(shapes), None, 0) == -1 and b"pair 0" in lib.mstg_last_error()  # no table for a resized pair
    table_len = 2 * max(max(s[0], s[1]) for s in shapes)
    assert lib.mstg_pair_metrics_validate(arr, len(shapes), None, table_len) == 0, lib.mstg_last_error()


REFUSALS = [
    ((0, 30, 8, 8), -1, b"below 1", b"0 x 30"),
    ((30, 30, 8, 0), -1, b"below 1", b"8 x 0"),
    ((30, 30, -2, 8), -1, b"below 1", b"-2 x 8"),
    ((6, 30, 8, 8), -1, b"7x7", b"6 x 30"),
    ((30, 6, 8, 8), -1, b"7x7", b"30 x 6"),
    ((26758, 26755, 8, 8), -5, b"image a", str(26758 * 26755 * 3).encode()),
    ((30, 30, 26758, 26755), -5, b"image b", str(26758 * 26755 * 3).encode()),
]


@pytest.mark.parametrize("shape,code,what,value", REFUSALS, ids=[str(r[0]) for r in REFUSALS])
def test_validation_names_the_pair_index_and_the_workspace_query_returns_zero(lib, shape, code, what, value):
    good = (30, 40, 20, 20)
    for position in (0, 2):
        shapes = [good, good, good]
        shapes[position] = shape
        arr = _descs(shapes)
        assert lib.mstg_pair_metrics_tiles(arr, 3, None, 0) == code
        msg = lib.mstg_last_error()
        assert f"pair {position}:".encode() in msg and what in msg and value in msg, msg
        assert lib.mstg_pair_metrics_validate(arr, 3, None, 1 << 20) == code and f"pair {position}:".encode() in lib.mstg_last_error()
        assert lib.mstg_pair_metrics_workspace_bytes(arr, 3) == 0
        assert lib.mstg_pair_metrics_u8(arr, 3, None, 0, 4096, 4096, 1, 4096, 4096, 4096, 1 << 30, None) == code  # before any launch


def test_total_tile_count_is_refused_by_name(lib):
    big = (26000, 26000, 8, 8)  # 407 x 1625 tiles
    per = 407 * 1625
    count = (1 << 24) // per + 1
    arr = _descs([big] * count)
    assert lib.mstg_pair_metrics_tiles(arr, count, None, 0) == -5
    msg = lib.mstg_last_error()
    assert f"pair {count - 1}:".encode() in msg and str(per * count).encode() in msg and b"tile count" in msg, msg
    assert lib.mstg_pair_metrics_workspace_bytes(arr, count) == 0
    assert lib.mstg_pair_metrics_tiles(arr, count - 1, None, 0) == per * (count - 1)
    huge = _descs([big] * 3400)  # 2.2e9 tiles: past int32 as well
    assert lib.mstg_pair_metrics_tiles(huge, 3400, None, 0) == -5 and lib.mstg_pair_metrics_workspace_bytes(huge, 3400) == 0


def test_validation_of_tile_fields_tables_and_arguments(lib):
    shapes = [(30, 40, 20, 20), (30, 40, 30, 40)]
    arr = _descs(shapes)
    assert lib.mstg_pair_metrics_validate(None, 2, None, 0) == -1 and lib.mstg_pair_metrics_validate(arr, 0, None, 0) == -1
    assert lib.mstg_pair_metrics_workspace_bytes(None, 2) == 0 and lib.mstg_pair_metrics_workspace_bytes(arr, 0) == 0
    assert lib.mstg_pair_metrics_validate(arr, 2, None, 1000) == -1 and b"pair 0" in lib.mstg_last_error() and b"tile0" in lib.mstg_last_error()
    assert lib.mstg_pair_metrics_tiles(arr, 2, None, 0) == 4  # two tiles each
    assert lib.mstg_pair_metrics_validate(arr, 2, None, 1000) == 0
    arr[1].tile0 = 0
    assert lib.mstg_pair_metrics_validate(arr, 2, None, 1000) == -1 and b"pair 1" in lib.mstg_last_error()
    arr[1].tile0 = 2
    arr[1].a = None
    assert lib.mstg_pair_metrics_validate(arr, 2, None, 1000) == -1 and b"pair 1: null" in lib.mstg_last_error()
    arr[1].a = 4096
    # table offsets: pair 0 needs 2 * 30 words at table_v and 2 * 40 at table_h
    arr[0].table_v, arr[0].table_h = 0, 60
    assert lib.mstg_pair_metrics_validate(arr, 2, None, 140) == 0
    assert lib.mstg_pair_metrics_validate(arr, 2, None, 139) == -1 and b"pair 0" in lib.mstg_last_error() and b"139" in lib.mstg_last_error()
    arr[0].table_v = -1
    assert lib.mstg_pair_metrics_validate(arr, 2, None, 140) == -1
    arr[0].table_v = 0
    # table contents: every index inside b
    iv, wv = _entry(lib, 20, 30, 0)
    ih, wh = _entry(lib, 20, 40, 1)
    table = np.concatenate([iv, wv.view(np.int32).ravel(), ih, wh.view(np.int32).ravel()])
    assert table.size == 140 and lib.mstg_pair_metrics_validate(arr, 2, table.ctypes.data, 140) == 0, lib.mstg_last_error()
    bad = table.copy()
    bad[60 + 5] = 20
    assert lib.mstg_pair_metrics_validate(arr, 2, bad.ctypes.data, 140) == -1
    assert b"pair 0" in lib.mstg_last_error() and b"horizontal index 20 at column 5" in lib.mstg_last_error()
    bad = table.copy()
    bad[7] = -2
    assert lib.mstg_pair_metrics_validate(arr, 2, bad.ctypes.data, 140) == -1 and b"vertical index -2 at row 7" in lib.mstg_last_error()
    # the launch entry: nulls, tile count, workspace, alignment -- all before a launch
    f = lib.mstg_pair_metrics_u8
    p = 4096
    assert f(arr, 2, table.ctypes.data, 140, None, p, 4, p, p, p, 128, None) == -1
    assert f(arr, 2, table.ctypes.data, 140, p, p, 3, p, p, p, 128, None) == -1
    assert f(arr, 2, table.ctypes.data, 140, p, p, 4, None, p, p, 128, None) == -1  # a resized pair and no device table
    assert f(arr, 2, table.ctypes.data, 140, p, p, 4, p, p, p, 127, None) == -4
    assert f(arr, 2, table.ctypes.data, 140, p, p, 4, p, p, None, 128, None) == -4
    assert f(arr, 2, table.ctypes.data, 140, p, p + 8, 4, p, p, p, 128, None) == -2
    assert f(arr, 2, table.ctypes.data, 140, p, p, 4, p, p + 4, p, 128, None) == -2


def test_resize_entry_validates_on_the_host(lib):
    f, p = lib.mstg_cv_resize_linear_u8, 1 << 20
    assert f(None, 1, 8, 8, 4, 4, p, p, p + 4096, None) == -1
    assert f(p, 1, 8, 8, 4, 4, p, p, None, None) == -1
    assert f(p, 1, 8, 8, 4, 4, None, p, p + 4096, None) == -1
    for bad in [(0, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, 8, 4, 0)]:
        assert f(p, *bad, p, p, p + 4096, None) == -1 and b"at least 1" in lib.mstg_last_error()
    assert f(p, 1, 26758, 26755, 4, 4, p, p, p + (1 << 40), None) == -5 and str(26758 * 26755 * 3).encode() in lib.mstg_last_error()
    assert f(p, 70000, 8, 8, 4, 4, p, p, p + (1 << 40), None) == -5
    assert f(p, 1, 8, 8, 4, 4, p + 2, p, p + 4096, None) == -2
    for dst in (p, p + 8 * 8 * 3 - 1, p - 4 * 4 * 3 + 1):  # the output overlaps the input
        assert f(p, 1, 8, 8, 4, 4, p, p, dst, None) == -1 and b"overlaps" in lib.mstg_last_error()


# ---- Python surface up to the launch ---------------------------------------------------------------------------------------------
def test_python_surface_rejects_before_the_launch():
    import torch

    from mstg_hip import image, metrics
    a = torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.pair_metrics([a], [a])
    with pytest.raises(ValueError, match="1 images against 2"):
        metrics.pair_metrics([a], [a, a])
    with pytest.raises(ValueError, match="at least one pair"):
        metrics.pair_metrics([], [])
    with pytest.raises(RuntimeError, match="GPU"):
        image.cv_resize_u8(a, (4, 4))
    assert metrics.evaluate_pairs_resized([]) == ([], None)
    assert metrics.compare_three_way([], [], []) == ([], None, None)
    with pytest.raises(ValueError, match="2 originals, 1 CycleGAN"):
        metrics.compare_three_way([a, a], [a], [a, a])
    tie = {"mse": 0.5, "psnr": 3.0, "ssim": 0.25}
    assert metrics.better_labels(tie, dict(tie)) == {"mse_better": "CycleGAN", "psnr_better": "CycleGAN", "ssim_better": "CycleGAN"}
    better = {"mse": 0.4, "psnr": 3.5, "ssim": 0.3}
    assert metrics.better_labels(tie, better) == {"mse_better": "LocalStyle", "psnr_better": "LocalStyle", "ssim_better": "LocalStyle"}
    assert metrics.better_labels(better, tie) == {"mse_better": "CycleGAN", "psnr_better": "CycleGAN", "ssim_better": "CycleGAN"}


def test_three_way_rows_come_from_one_pair_metrics_call(monkeypatch):
    """2 P comparisons, one call: the launch is stubbed with a function of the shapes"""
    import torch

    from mstg_hip import metrics
    calls = []

    def fake(images_a, images_b):
        calls.append(([tuple(t.shape) for t in images_a], [tuple(t.shape) for t in images_b]))
        v = torch.tensor([[b.shape[0] / 100.0, b.shape[1], 1.0 / b.shape[0]] for b in images_b], dtype=torch.float64)
        return {"mse": v[:, 0], "psnr": v[:, 1], "ssim": v[:, 2], "ssim_channels": v}

    monkeypatch.setattr(metrics, "pair_metrics", fake)
    monkeypatch.setattr(metrics, "_as_cuda_u8", lambda img, name: torch.from_numpy(img) if isinstance(img, np.ndarray) else img)
    z = lambda h, w: np.zeros((h, w, 3), np.uint8)  # noqa: E731
    rows, avg_cy, avg_ls = metrics.compare_three_way([z(10, 10), z(12, 9)], [z(10, 10), z(20, 30)], [z(5, 10), z(20, 30)])
    assert calls == [([(10, 10, 3), (12, 9, 3)] * 2, [(10, 10, 3), (20, 30, 3), (5, 10, 3), (20, 30, 3)])]
    assert [r["cyclegan"]["resized"] for r in rows] == [False, True] and [r["local_style"]["resized"] for r in rows] == [True, True]
    assert rows[0]["comparison"] == {"mse_better": "LocalStyle", "psnr_better": "CycleGAN", "ssim_better": "LocalStyle"}
    assert rows[1]["comparison"] == {"mse_better": "CycleGAN", "psnr_better": "CycleGAN", "ssim_better": "CycleGAN"}  # a tie in all three
    assert avg_cy == {"mse": (0.1 + 0.2) / 2, "psnr": 20.0, "ssim": (0.1 + 0.05) / 2} and avg_ls["psnr"] == 20.0


# ---- the drop-ins: listing and matching on temporary folders ---------------------------------------------------------------------
def _touch(folder, names):
    folder.mkdir()
    for n in names:
        (folder / n).write_bytes(b"")
    return str(folder)


def test_compare_image_quality_matches_exact_names(tmp_path):
    import compare_image_quality as ciq
    test = _touch(tmp_path / "test", ["a.jpg", "b.png", "c.jpeg", "d.bmp", "E.PNG", "only.jpg"])
    ls = _touch(tmp_path / "ls", ["a.jpg", "b.png", "c.jpeg", "d.bmp", "E.PNG", "x_only.jpg"])
    cy = _touch(tmp_path / "cy", ["a.jpg", "b.png", "cyclegan_c.jpeg", "d.bmp", "E.PNG"])
    assert sorted(ciq.list_names(test)) == ["a.jpg", "b.png", "c.jpeg", "only.jpg"]  # .bmp and upper-case extensions are not listed
    assert sorted(ciq.match_test_images(ls, cy, test)) == ["a.jpg", "b.png"]  # the exact name, in all three folders
    assert ciq.find_matching_images(test, ls) == {"a.jpg", "b.png", "c.jpeg"}
    assert ciq.compare_with_test_images(ls, cy, str(tmp_path / "none")) is None  # nothing listed: nothing decoded or launched
    assert ciq.compare_image_folders(str(tmp_path / "none"), [ls]) == []
    assert ciq.compare_image_folders(test, [test, str(tmp_path / "none")]) == []  # itself: skipped; no common names: skipped
    for call in (lambda: ciq.compare_with_test_images(ls, cy, test, output_file="r.xlsx"),
                 lambda: ciq.compare_image_folders(test, [ls], output_file="r.xlsx")):
        with pytest.raises(ValueError, match=r"\.xlsx"):
            call()
    with pytest.raises(ValueError, match="only .csv"):
        ciq.compare_image_folders(test, [ls], output_file="chart.png")


def test_compare_image_quality_float_images_map_back_to_bytes():
    import compare_image_quality as ciq
    img = np.random.RandomState(3).randint(0, 256, size=(9, 11, 3)).astype(np.uint8)
    assert ciq._as_u8(img, "img1") is img
    assert np.array_equal(ciq._as_u8(img.astype(float) / 255.0, "img1"), img)
    off = img.astype(float) / 255.0
    off[2, 3, 1] += 1e-6
    with pytest.raises(ValueError, match="off the byte grid by"):
        ciq._as_u8(off, "img1")
    with pytest.raises(ValueError, match="byte grid|8-bit"):
        ciq._as_u8(np.full((4, 4, 3), 256 / 255.0), "img2")
    with pytest.raises(ValueError, match="int32"):
        ciq._as_u8(img.astype(np.int32), "img1")


def test_complete_comparison_matches_orig_in_other(tmp_path):
    import complete_comparison as cc
    orig = _touch(tmp_path / "orig", ["001.jpg", "sky.png", "tree.bmp", "alone.jpg", "UP.PNG", "long_name.jpg"])
    cy = _touch(tmp_path / "cy", ["cyclegan_001.jpg", "sky.png", "tree.bmp", "alone.jpg", "name.jpg"])
    ls = _touch(tmp_path / "ls", ["local_style_001.jpg", "x_sky.png", "sky.png", "tree.bmp", "name.jpg"])
    files = [cc.list_images(f) for f in (orig, cy, ls)]
    assert sorted(os.path.basename(f) for f in files[0]) == ["001.jpg", "alone.jpg", "long_name.jpg", "sky.png", "tree.bmp"]
    got = {tuple(os.path.basename(p) for p in s) for s in cc.match_sets(*files)}
    # 'orig in other' only: long_name.jpg does not match name.jpg (the other way round); alone.jpg has no local-style file
    assert {s for s in got if s[0] != "sky.png"} == {("001.jpg", "cyclegan_001.jpg", "local_style_001.jpg"), ("tree.bmp", "tree.bmp", "tree.bmp")}
    assert [s for s in got if s[0] == "sky.png"][0][2] in ("x_sky.png", "sky.png") and len(got) == 3
    # the first match in listing order wins
    assert cc.match_sets(["/o/a.png"], ["/c/zz_a.png", "/c/a.png"], ["/l/a.png", "/l/zz_a.png"]) == [("/o/a.png", "/c/zz_a.png", "/l/a.png")]
    assert cc.compare_with_original(orig, str(tmp_path / "none"), ls) is None
    with pytest.raises(ValueError, match=r"\.xlsx"):
        cc.compare_with_original(orig, cy, ls, output="detailed_metrics_comparison.xlsx")
    assert cc.COLUMNS == ("Image Name", "CycleGAN MSE", "LocalStyle MSE", "MSE Better", "CycleGAN PSNR", "LocalStyle PSNR", "PSNR Better",
                          "CycleGAN SSIM", "LocalStyle SSIM", "SSIM Better")


def test_improved_image_compare_matches_stems_either_way_sorted(tmp_path):
    import improved_image_compare as iic
    orig = _touch(tmp_path / "orig", ["b_long_name.jpg", "a1.png", "zz.jpg", "alone.jpg"])
    cy = _touch(tmp_path / "cy", ["cyclegan_a1.jpg", "name.png", "zz.png"])
    ls = _touch(tmp_path / "ls", ["a1_local.bmp", "long_name.jpg", "zz.jpeg", "alone.jpg"])
    files = [iic.list_images(f) for f in (orig, cy, ls)]
    got = [tuple(os.path.basename(p) for p in s) for s in iic.match_sets(*files)]
    # stems, either direction: b_long_name contains name (CycleGAN) and long_name (local style); extensions do not matter; sorted
    assert got == [("a1.png", "cyclegan_a1.jpg", "a1_local.bmp"), ("b_long_name.jpg", "name.png", "long_name.jpg"), ("zz.jpg", "zz.png", "zz.jpeg")]
    assert iic.get_file_ext("/x/Y.JPG") == ".jpg"
    assert iic.compare_folders_with_original(orig, str(tmp_path / "none"), ls) is None
    with pytest.raises(ValueError, match=r"\.xlsx"):
        iic.compare_folders_with_original(orig, cy, ls, output="out.xlsx")
