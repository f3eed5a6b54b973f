"""CPU: the quickshift segmentation's host side (mstg_quickshift_workspace_bytes, every refusal by name, null pointers, overlaps)
and the properties the header claims of the definition, checked on the numpy restatement of tests/quickshift_ref.py: flat images
and ratio 0 are one segment, the labels are 0 .. count - 1 numbered by ascending root, the reduced search square changes no
parent, and the density gaps of the three cases on which the GPU test demands plain end-to-end equality exceed twice the window's
tap count (two float64 exp move a density by at most the tap count).  Also the drop-in's --device-segmentation option.  The
restatement has not been compared with a scikit-image binary (see its docstring)."""
import os
import re

import numpy as np
import pytest
import torch

import quickshift_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {"BADARG": -1, "ALIGN": -2, "LAUNCH": -3, "WORKSPACE": -4, "UNSUPPORTED": -5}


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


# ---- properties of the restatement ------------------------------------------------------------------------------------------------
def test_flat_images_and_ratio_zero_are_one_segment():
    for name in ("flat", "flat_small", "one"):
        r = QR.reference(name)
        assert r["count"] == 1 and not r["labels"].any(), name
    r = QR.reference("smooth_noise48", (0.0, 3, 6))  # ratio 0: the colours do not count, the image is as good as flat
    assert r["count"] == 1 and not r["labels"].any()
    flat = QR.reference("flat")
    assert flat["stats"]["depth"] > 64, flat["stats"]  # a chain that a walk of 64 hops does not finish
    assert flat["stats"]["ties"] > 100000  # the interior densities tie exactly: the raster index decides
    interior = flat["density"][9:-9, 9:-9]
    assert (interior == interior[0, 0]).all()


def test_noise_leaves_most_pixels_as_roots():
    r = QR.reference("noise")
    H, W = r["img"].shape[:2]
    assert r["stats"]["roots"] == r["count"] and 2 * r["count"] > H * W, (r["count"], H * W)


@pytest.mark.parametrize("run", QR.RUNS, ids=lambda run: f"{run[0]}-{run[1]}")
def test_labels_are_numbered_by_ascending_root(run):
    name, params = run
    r = QR.reference(name, params)
    labels, parent, count = r["labels"], r["parent"], r["count"]
    H, W = labels.shape
    assert np.array_equal(np.unique(labels), np.arange(count))  # exactly 0 .. count - 1
    roots = np.flatnonzero(parent.ravel() == np.arange(H * W))
    assert len(roots) == count and np.array_equal(labels.ravel()[roots], np.arange(count))  # ascending root index
    assert np.array_equal(labels.ravel()[parent.ravel()], labels.ravel())  # a pixel has its parent's label
    first = [int(np.flatnonzero(labels.ravel() == v)[0]) for v in range(count)]
    # np.unique(root of every pixel, return_inverse=True) numbers the same way
    root_of = roots[labels.ravel()]
    assert np.array_equal(np.unique(root_of, return_inverse=True)[1].reshape(H, W), labels)
    assert all(f <= r0 for f, r0 in zip(first, roots))
    # the density is what the header bounds it by
    w, _ = QR.check(H, W, *params)
    assert r["density"].min() >= 1 << 32 and (r["density"] <= QR.taps(H, W, w) << 32).all()


@pytest.mark.parametrize("run", QR.RUNS, ids=lambda run: f"{run[0]}-{run[1]}")
def test_the_reduced_search_square_changes_no_parent(run):
    name, params = run
    r = QR.reference(name, params)
    H, W = r["img"].shape[:2]
    w, reach = QR.check(H, W, *params)
    assert reach == min(w, int(params[2]))
    assert np.array_equal(QR.parents(r["img"], r["density"], *params, reach=reach), r["parent"])


def test_density_gaps_allow_plain_equality_on_three_cases():
    """A device exp that differs from numpy's by a few ulp moves a term by at most one unit, a density by at most its tap count and
    a difference of two densities by at most twice that: where the smallest non-zero difference among compared pairs is larger,
    no comparison can come out differently (exact ties hold the same terms and stay ties)."""
    bound = 2 * (2 * QR.window(3) + 1) ** 2
    assert bound == 722
    for name in QR.EXACT_CASES:
        gap = QR.reference(name)["stats"]["gap"]
        assert gap is not None and gap > bound, (name, gap)
    assert QR.reference("smooth")["stats"]["gap"] <= bound  # the others do not promise it: the GPU test does not demand it there
    assert set(QR.EXACT_CASES) == {"flat", "flat_small", "blocks96"}


def test_a_given_density_drives_the_later_stages():
    r = QR.reference("smooth")
    other = np.array(r["density"])
    other[5, 7] += 1 << 36  # a new peak
    out = QR.quickshift(r["img"], *r["params"], density=other)
    assert out["parent"][5, 7] == 5 * 53 + 7 and not np.array_equal(out["parent"], r["parent"])
    same = QR.quickshift(r["img"], *r["params"], density=r["density"])
    assert np.array_equal(same["labels"], r["labels"]) and same["count"] == r["count"]


# ---- header and refusals -----------------------------------------------------------------------------------------------------------
def test_header_constants_equal_the_restatements():
    from mstg_hip import _lib
    text = open(os.path.join(ROOT, "include", "mstg_hip.h")).read()
    assert int(re.search(r"#define MSTG_QUICKSHIFT_MAX_RADIUS (\d+)", text).group(1)) == QR.MAX_RADIUS == _lib.QUICKSHIFT_MAX_RADIUS
    assert int(re.search(r"#define MSTG_SEGMENT_MAX_PIXELS (\d+)", text).group(1)) == QR.MAX_PIXELS == _lib.SEGMENT_MAX_PIXELS
    assert "RESTATED AS RECALLED, NOT COMPARED WITH A SCIKIT-IMAGE BINARY" in text


# (H, W, ratio, kernel_size, max_dist) -> the words the refusal must hold
REFUSED = [((16, 16, 0.5, 0.5, 6.0), "kernel_size = 0.5"), ((16, 16, 0.5, float("nan"), 6.0), "kernel_size = "),
           ((16, 16, 0.5, float("inf"), 6.0), "kernel_size = inf"), ((16, 16, 0.5, 5.5, 6.0), "w = 17"), ((16, 16, 0.5, 3.0, 0.0), "max_dist = 0"),
           ((16, 16, 0.5, 3.0, -1.0), "max_dist = -1"), ((16, 16, 0.5, 3.0, float("inf")), "max_dist = inf"),
           ((16, 16, 0.5, 3.0, float("nan")), "max_dist = "), ((16, 16, 1.5, 3.0, 6.0), "ratio = 1.5"), ((16, 16, -0.1, 3.0, 6.0), "ratio = -0.1"),
           ((16, 16, float("nan"), 3.0, 6.0), "ratio = "), ((1024, 1025, 0.5, 3.0, 6.0), "H * W = 1049600"), ((0, 5, 0.5, 3.0, 6.0), "H = 0, W = 5"),
           ((5, 0, 0.5, 3.0, 6.0), "H = 5, W = 0")]


def test_every_refusal_names_its_value_and_returns_before_a_launch(lib):
    buf = np.zeros(1 << 16, dtype=np.uint8)  # host memory: every call below must return before it launches anything
    p = buf.ctypes.data
    img, table, out, count, ws = p, p + 1024, p + 16384, p + 32768, p + 40960
    for (H, W, ratio, ks, md), words in REFUSED:
        with pytest.raises(QR.Refused):
            QR.check(H, W, ratio, ks, md)
        shape_or_kernel = not (words.startswith("max_dist") or words.startswith("ratio"))
        calls = [("u8", lambda: lib.mstg_quickshift_u8(img, 1, H, W, ratio, ks, md, table, out, count, ws, 1 << 14, None)),
                 ("parents", lambda: lib.mstg_quickshift_parents_u8(img, ws, 1, H, W, ratio, ks, md, table, out, None))]
        if not words.startswith("max_dist"):
            calls.append(("density", lambda: lib.mstg_quickshift_density_u8(img, 1, H, W, ratio, ks, table, ws, None)))
        for what, call in calls:
            rc = call()
            msg = lib.mstg_last_error().decode()
            assert rc in (CODE["UNSUPPORTED"], CODE["BADARG"]), (what, words, rc)
            assert words in msg, (what, words, msg)
        if shape_or_kernel:
            assert lib.mstg_quickshift_workspace_bytes(1, H, W, ks) == 0
            assert words in lib.mstg_last_error().decode()
    assert lib.mstg_quickshift_workspace_bytes(0, 16, 16, 3.0) == 0
    assert 0 < lib.mstg_quickshift_workspace_bytes(1, 16, 16, 3.0) < lib.mstg_quickshift_workspace_bytes(3, 16, 16, 3.0)
    assert lib.mstg_quickshift_workspace_bytes(1, 16, 16, 5.0) > 0  # w = 15: the largest window that is built
    assert lib.mstg_quickshift_workspace_bytes(1, 1024, 1024, 3.0) > 0


def test_null_pointers_workspace_and_overlaps_are_refused_before_any_launch(lib):
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    need = lib.mstg_quickshift_workspace_bytes(1, 16, 16, 3.0)
    assert 0 < need <= 1 << 14
    good = dict(img=p, table=p + 1024, labels=p + 16384, count=p + 32768, ws=p + 40960)

    def whole(**kw):
        a = dict(good, **kw)
        return lib.mstg_quickshift_u8(a["img"], 1, 16, 16, 0.5, 3.0, 6.0, a["table"], a["labels"], a["count"], a["ws"], kw.get("bytes", need), None)

    for hole in ("img", "table", "labels", "count"):
        assert whole(**{hole: None}) == CODE["BADARG"], hole
    assert whole(ws=None) == CODE["WORKSPACE"]
    assert whole(bytes=need - 1) == CODE["WORKSPACE"] and "workspace too small" in lib.mstg_last_error().decode()
    assert whole(labels=p + 256) == CODE["BADARG"] and "overlaps" in lib.mstg_last_error().decode()  # labels on the image
    assert whole(ws=p + 512) == CODE["BADARG"] and "overlaps" in lib.mstg_last_error().decode()  # workspace on image and table
    assert whole(count=p + 16384 + 512) == CODE["BADARG"] and "overlaps" in lib.mstg_last_error().decode()  # count inside labels
    assert whole(labels=p + 16384 + 2) == CODE["ALIGN"]
    assert whole(ws=p + 40960 + 8) == CODE["ALIGN"]

    dens = p + 40960
    assert lib.mstg_quickshift_density_u8(None, 1, 16, 16, 0.5, 3.0, p + 1024, dens, None) == CODE["BADARG"]
    assert lib.mstg_quickshift_density_u8(p, 1, 16, 16, 0.5, 3.0, None, dens, None) == CODE["BADARG"]
    assert lib.mstg_quickshift_density_u8(p, 1, 16, 16, 0.5, 3.0, p + 1024, None, None) == CODE["BADARG"]
    assert lib.mstg_quickshift_density_u8(p, 1, 16, 16, 0.5, 3.0, p + 1024, p + 512, None) == CODE["BADARG"]  # density on the image
    assert "overlaps" in lib.mstg_last_error().decode()
    assert lib.mstg_quickshift_density_u8(p, 1, 16, 16, 0.5, 3.0, p + 1024, dens + 4, None) == CODE["ALIGN"]
    par = p + 16384
    assert lib.mstg_quickshift_parents_u8(p, None, 1, 16, 16, 0.5, 3.0, 6.0, p + 1024, par, None) == CODE["BADARG"]
    assert lib.mstg_quickshift_parents_u8(p, dens, 1, 16, 16, 0.5, 3.0, 6.0, p + 1024, None, None) == CODE["BADARG"]
    assert lib.mstg_quickshift_parents_u8(p, dens, 1, 16, 16, 0.5, 3.0, 6.0, p + 1024, dens + 64, None) == CODE["BADARG"]  # parent on the density
    assert "overlaps" in lib.mstg_last_error().decode()


def test_python_refusals():
    from mstg_hip import image as dimg
    host = torch.zeros((8, 8, 3), dtype=torch.uint8)
    for fn in (dimg.quickshift_labels, dimg.quickshift_density, lambda x: dimg.quickshift_parents(x, np.zeros((8, 8), dtype=np.int64))):
        with pytest.raises(RuntimeError, match="on the GPU"):
            fn(host)
    with pytest.raises(RuntimeError, match="on the GPU"):
        dimg.quickshift_segmenter()(host)
    assert callable(dimg.quickshift_segmenter()) and callable(dimg.slic_segmenter())
    assert dimg.SEGMENTATIONS == ("felzenszwalb", "slic")  # quickshift enters through segments=, not through the keyword
    with pytest.raises(ValueError, match="quickshift"):
        dimg.process_enhanced_local_style(None, None, segmentation="quickshift")
    with pytest.raises(ValueError, match="quickshift"):
        dimg.process_enhanced_local_style(None, None, segments=dimg.quickshift_segmenter(), segmentation="quickshift")


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def test_drop_in_command_line_takes_the_device_segmentation():
    import enhanced_local_style as E
    from mstg_hip import image as dimg
    parser = E.build_parser()
    base = ["--image", "a.png", "--model", "m.pth"]
    args = parser.parse_args(base)
    assert args.device_segmentation is None and args.segmentation == "felzenszwalb"
    args = parser.parse_args(base + ["--device-segmentation", "quickshift"])
    assert args.device_segmentation == "quickshift" and args.segmentation == "felzenszwalb"
    assert parser.parse_args(base + ["--device-segmentation", "slic"]).device_segmentation == "slic"
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--device-segmentation", "felzenszwalb"])
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--segmentation", "quickshift"])  # stays refused there
    assert E.DEVICE_SEGMENTERS == {"slic": dimg.slic_segmenter, "quickshift": dimg.quickshift_segmenter}
    with pytest.raises(NotImplementedError, match="quickshift"):  # the reference's own entry keeps refusing it by name
        E.get_segmentation_mask(np.zeros((8, 8, 3), dtype=np.uint8), method="quickshift")
    assert "device-segmentation" in E.__doc__
