"""CPU: the SLIC segmentation's host side (mstg_slic_grid, mstg_slic_workspace_bytes, the refusals by name, null pointers) against the
numpy restatement of tests/slic_ref.py, the properties the header claims of the definition checked on that restatement (every pixel
has a candidate in round 1, the final labels are connected and numbered 1 .. count, the count stays below the host's bound), and
the drop-in's --segmentation option.  The restatement has not been compared with a scikit-image binary (see its docstring)."""
import numpy as np
import pytest
from scipy import ndimage

import slic_ref as SR

SWEEP = [(256, 256, 100), (96, 80, 30), (37, 53, 12), (40, 70, 15), (64, 48, 100), (64, 64, 1), (7, 9, 2), (1024, 1024, 100), (1024, 1024, 4096),
         (100, 100, 16), (100, 100, 44), (300, 17, 20), (17, 300, 20), (2, 2, 3), (50, 50, 8), (31, 31, 6), (640, 480, 250), (33, 47, 1000)]
REFUSED = [((256, 256, 0), "n_segments = 0"), ((256, 256, -3), "n_segments = -3"), ((10, 10, 100), "n_segments = 100"),
           ((10, 10, 500), "n_segments = 500"), ((5, 200, 10), "step = 10"), ((200, 5, 10), "step = 10"), ((1024, 1025, 100), "H * W = 1049600"),
           ((1024, 1024, 6000), "K = "), ((0, 5, 1), "H = 0, W = 5")]


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _grid(lib, H, W, n):
    out = np.full(3, -1, dtype=np.int32)
    at = out.ctypes.data
    return lib.mstg_slic_grid(H, W, n, at, at + 4, at + 8), tuple(int(v) for v in out)


def test_grid_equals_the_restatement(lib):
    assert _grid(lib, 256, 256, 100) == (0, (26, 10, 10))
    for H, W, n in SWEEP:
        step, ny, nx, start = SR.grid(H, W, n)
        assert _grid(lib, H, W, n) == (0, (step, ny, nx)), (H, W, n)
        assert start + (ny - 1) * step < H <= start + ny * step and start + (nx - 1) * step < W <= start + nx * step
        assert lib.mstg_slic_workspace_bytes(1, H, W, n) > 0 and lib.mstg_slic_workspace_bytes(3, H, W, n) > lib.mstg_slic_workspace_bytes(1, H, W, n)
    # step = rint(s) rounds ties to even: 25 x 25 pixels in 100 segments has s = 2.5 exactly
    assert SR.grid(25, 25, 100)[0] == 2 and _grid(lib, 25, 25, 100)[1][0] == 2
    assert SR.grid(35, 35, 100)[0] == 4 and _grid(lib, 35, 35, 100)[1][0] == 4  # s = 3.5


def test_every_refusal_names_its_value(lib):
    from mstg_hip import _lib
    for (H, W, n), words in REFUSED:
        with pytest.raises(SR.Refused):
            SR.grid(H, W, n)
        rc, out = _grid(lib, H, W, n)
        msg = lib.mstg_last_error().decode()
        assert rc in (_lib_code("UNSUPPORTED"), _lib_code("BADARG")) and out == (-1, -1, -1), (H, W, n, rc)
        assert words in msg, (H, W, n, msg)
        assert lib.mstg_slic_workspace_bytes(1, H, W, n) == 0, (H, W, n)
        assert words in lib.mstg_last_error().decode()
    assert lib.mstg_slic_workspace_bytes(0, 64, 64, 10) == 0
    assert _lib.SLIC_MAX_CENTRES == SR.MAX_CENTRES >= 1024 and _lib.SEGMENT_MAX_PIXELS == SR.MAX_PIXELS


def _lib_code(name):
    return {"BADARG": -1, "ALIGN": -2, "LAUNCH": -3, "WORKSPACE": -4, "UNSUPPORTED": -5}[name]


def test_null_pointers_and_bad_parameters_are_refused_before_any_launch(lib):
    out = np.zeros(3, dtype=np.int32)
    at = out.ctypes.data
    for args in ((None, at, at), (at, None, at), (at, at, None)):
        assert lib.mstg_slic_grid(64, 64, 10, *args) == _lib_code("BADARG")
    buf = np.zeros(1 << 16, dtype=np.uint8)  # host memory: every call below must return before it launches anything
    p = buf.ctypes.data
    need = lib.mstg_slic_workspace_bytes(1, 16, 16, 4)
    assert 0 < need
    for entry in (lib.mstg_slic_u8, lib.mstg_slic_assign_u8):
        for hole in range(4):
            ptrs = [p, p + 1024, p + 8192, p + 16384]
            ptrs[hole] = None
            assert entry(ptrs[0], 1, 16, 16, 4, 10.0, ptrs[1], ptrs[2], ptrs[3], p + 32768, need, None) == _lib_code("BADARG")
        assert entry(p, 1, 16, 16, 4, 10.0, p + 1024, p + 8192, p + 16384, None, need, None) == _lib_code("WORKSPACE")
        assert entry(p, 1, 16, 16, 4, 10.0, p + 1024, p + 8192, p + 16384, p + 32768, 16, None) == _lib_code("WORKSPACE")
        for bad in (0.0, -2.0, float("nan")):
            assert entry(p, 1, 16, 16, 4, bad, p + 1024, p + 8192, p + 16384, p + 32768, need, None) == _lib_code("UNSUPPORTED")
            assert "compactness = " in lib.mstg_last_error().decode()
        assert entry(p, 1, 5, 200, 10, 10.0, p + 1024, p + 8192, p + 16384, p + 32768, need, None) == _lib_code("UNSUPPORTED")
        assert "step = 10" in lib.mstg_last_error().decode()
    need = lib.mstg_connect_labels_workspace_bytes(1, 8, 8)
    assert need > 0 and lib.mstg_connect_labels_workspace_bytes(1, 1024, 1025) == 0 and lib.mstg_connect_labels_workspace_bytes(1, 0, 8) == 0
    assert lib.mstg_connect_labels(None, 1, 8, 8, 2, p + 1024, p + 2048, p + 4096, need, None) == _lib_code("BADARG")
    assert lib.mstg_connect_labels(p, 1, 8, 8, 2, None, p + 2048, p + 4096, need, None) == _lib_code("BADARG")
    assert lib.mstg_connect_labels(p, 1, 8, 8, 2, p + 1024, None, p + 4096, need, None) == _lib_code("BADARG")
    assert lib.mstg_connect_labels(p, 1, 8, 8, 2, p + 1024, p + 2048, None, need, None) == _lib_code("WORKSPACE")
    assert lib.mstg_connect_labels(p, 1, 8, 8, 2, p + 128, p + 2048, p + 4096, need, None) == _lib_code("BADARG")  # out overlaps in
    assert "overlaps" in lib.mstg_last_error().decode()
    assert lib.mstg_connect_labels(p, 1, 1024, 1025, 2, p + 1024, p + 2048, p + 4096, need, None) == _lib_code("UNSUPPORTED")


def test_python_bound_and_grid_follow_the_restatement(lib):
    from mstg_hip import image as dimg
    assert dimg.slic_grid(256, 256, 100) == (26, 10, 10) and dimg.slic_segment_bound(256, 256, 100) == 201
    for H, W, n in SWEEP:
        assert dimg.slic_segment_bound(H, W, n) == SR.segment_bound(H, W, n)
    with pytest.raises(RuntimeError, match="step = 10"):
        dimg.slic_segment_bound(5, 200, 10)
    with pytest.raises(ValueError, match="quickshift"):
        dimg.process_enhanced_local_style(None, None, segmentation="quickshift")


def test_round_one_leaves_no_pixel_without_a_candidate():
    """with the centres still on their grid every pixel lies within step of a grid row and a grid column"""
    for H, W, n in SWEEP:
        if H * W > 1 << 16:
            continue
        rs = np.random.RandomState(H + W + n)
        stats = {}
        SR.assign(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8), n, 10.0, rounds=1, stats=stats)
        assert stats["orphans"] == [0], (H, W, n)


@pytest.mark.parametrize("name", SR.CASES)
def test_properties_of_the_restatement(name):
    r = SR.reference(name)
    H, W = r["img"].shape[:2]
    labels, count, raw = r["labels"], r["count"], r["raw"]
    assert r["stats"]["orphans"][0] == 0
    assert raw.min() >= 0 and raw.max() < len(r["centres"])
    assert np.array_equal(np.unique(labels), np.arange(1, count + 1))  # exactly 1 .. count
    for v in range(1, count + 1):  # every final label is one 4-connected set
        assert ndimage.label(labels == v)[1] == 1, (name, v)
    assert count <= SR.segment_bound(H, W, r["n_segments"])
    first = [int(np.flatnonzero(labels.ravel() == v)[0]) for v in range(1, count + 1)]
    assert first == sorted(first)  # numbered in raster order of the first pixels


def test_the_cases_are_the_ones_their_names_promise():
    big = SR.reference("blocks256")
    assert (big["stats"]["components"], big["stats"]["small"], big["count"]) == (100, 16, 84)
    noise = SR.reference("noise")
    assert noise["count"] == 1 and noise["stats"]["small"] == noise["stats"]["components"] - 1 and noise["stats"]["deepest"] > 40
    flat = SR.reference("flat")
    assert flat["stats"]["small"] == 0 and flat["count"] == flat["stats"]["components"]
    st = {}
    labels, count = SR.connect(SR.checkerboard(32, 64), 2, st)
    assert count == 1 and st["components"] == 32 * 64 and st["deepest"] == 63 + 31  # along the row, then up the first column
    assert SR.connect(SR.checkerboard(32, 64), 1)[1] == 32 * 64
    st = {}
    labels, count = SR.connect(SR.serpentine(33, 47), 50, st)
    assert st["components"] == 17 and st["small"] == 16 and count == 1


def test_drop_in_command_line_takes_the_segmentation():
    import enhanced_local_style as E
    parser = E.build_parser()
    base = ["--image", "a.png", "--model", "m.pth"]
    assert parser.parse_args(base).segmentation == "felzenszwalb"
    assert parser.parse_args(base + ["--segmentation", "slic"]).segmentation == "slic"
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--segmentation", "quickshift"])
    with pytest.raises(SystemExit):
        E.main(base + ["--segmentation", "watershed"])
    with pytest.raises(NotImplementedError, match="slic"):  # the reference's own entry keeps refusing it by name
        E.get_segmentation_mask(np.zeros((8, 8, 3), dtype=np.uint8), method="slic")
