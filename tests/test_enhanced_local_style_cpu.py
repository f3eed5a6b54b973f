"""CPU: the numpy restatement of the segmentation-driven local style (tests/enhanced_local_style_ref.py) against what can be checked
without OpenCV and scikit-image: the reference's literal numpy evaluation of the ratios, scipy's own gaussian_filter bit for bit,
closed forms of CLAHE and of the 8-bit HSV -> RGB conversion, the measured shares the header states, the host segmentation
(mstg_felzenszwalb_u8) against the Python restatement label for label, the host-side refusals by name, and the drop-in's imports."""
import os
import subprocess
import sys

import numpy as np
import pytest

import enhanced_local_style_ref as ER
from app_local_style_ref import hsv_u8
from conftest import PKG

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


# ---- 1. the ratios ------------------------------------------------------------------------------------------------------------------
CASES = [((64, 64), 1), ((64, 64), 2), ((48, 80), 3), ((48, 80), 4), ((37, 53), 5), ((37, 53), 6)]


def test_ratio_equals_the_literal_numpy_evaluation():
    """The header's evaluation (exact integer sums, a 2^32 fixed-point edge sum, a fixed float64 order) against the reference's own
    numpy expressions (np.mean, np.std, a pairwise float64 mean of the magnitudes): 0 differing float32 map entries.  The inputs
    are chosen so that the literal evaluation is itself stable: no label's literal ratio changes when every masked reduction
    runs over the pixels in reversed order (_literal_reversed: the same sums, another summation order), so none sits on a float32
    rounding tie and every map entry is compared."""
    entries = differing = labels_total = unstable = 0
    for (h, w), seed in CASES:
        canvas = ER.smooth_noise(h, w, seed)
        labels, S = ER.grid_labels(h, w, seed)
        assert 25 <= len(np.unique(labels)) <= 48 or (h, w) == (64, 64)
        _, ratio = ER.segment_ratios(canvas, labels, S)
        lit = ER.literal_ratios(canvas, labels)
        lit2 = _literal_reversed(canvas, labels)
        for s in np.unique(labels):
            labels_total += 1
            if lit[int(s)] != lit2[int(s)]:
                unstable += 1
                continue
            n = int((labels == s).sum())
            entries += n
            if ratio[s] != lit[int(s)]:
                differing += n
    print(f"ratios: {entries} map entries compared, {differing} differ; {unstable} of {labels_total} labels unstable under reordering")
    assert unstable == 0 and entries == sum(h * w for (h, w), _ in CASES)
    assert differing == 0


def _literal_reversed(canvas, labels):
    """the literal ratios with every masked reduction taken in REVERSED pixel order: np.std / np.mean over ``a[mask][::-1]``"""
    H, W = labels.shape
    gray = ER.gray_u8(canvas)
    hsv = np.stack(hsv_u8(canvas), axis=-1).astype(np.uint8)
    center_y, center_x = H // 2, W // 2
    max_dist = np.sqrt(center_x ** 2 + center_y ** 2)
    out = {}
    for segment_id in np.unique(labels):
        mask = labels == segment_id
        region_rgb, region_hsv = canvas[mask][::-1], hsv[mask][::-1]
        avg_hsv = np.mean(region_hsv, axis=0)
        std_color = np.std(region_rgb, axis=0)
        gx, gy = ER.sobel101(np.where(mask, gray, 0))
        mag = np.sqrt(gx.astype(F64) ** 2 + gy.astype(F64) ** 2)
        edge_density = np.mean(mag[::-1, ::-1])
        size = np.sum(mask)
        pos_y, pos_x = np.mean(np.argwhere(mask)[::-1], axis=0)
        adjustment = (0.3 * (edge_density / 30) + 0.2 * (np.mean(std_color) / 50)
                      - 0.1 * (np.sqrt((pos_y - center_y) ** 2 + (pos_x - center_x) ** 2) / max_dist)
                      + -0.1 * (size / (H * W / 100)) + 0.2 * (avg_hsv[1] / 255))
        out[int(segment_id)] = F32(max(0.3, min(0.9, 0.7 + adjustment)))
    return out


def test_sums_closed_form():
    """one segment covering a constant image: every sum is known, the masked grey has no gradient (reflect-101 of a constant)"""
    canvas = np.full((6, 10, 3), (200, 100, 50), dtype=np.uint8)
    labels = np.zeros((6, 10), dtype=np.int32)
    sums, ratio = ER.segment_ratios(canvas, labels, 3)
    s = hsv_u8(canvas[:1, :1])[1][0, 0]
    assert list(sums[0]) == [60, 200 * 60, 100 * 60, 50 * 60, 200 * 200 * 60, 100 * 100 * 60, 50 * 50 * 60, int(s) * 60, 10 * 15, 6 * 45, 0]
    assert list(sums[1]) == [0] * 11 and ratio[1] == 0 and ratio[2] == 0
    # two halves: the masked grey steps from g to 0 at the boundary: |gx| = 4 g on both sides of it, for each of the two labels
    labels[:, 5:] = 2
    sums, _ = ER.segment_ratios(canvas, labels, 3)
    g = int(ER.gray_u8(canvas[:1, :1])[0, 0])
    assert sums[0][10] == sums[2][10] == 2 * 6 * 4 * g << 32
    # a label outside [0, S) contributes to nothing and maps to 0
    labels[0, 0] = -7
    labels[1, 1] = 3
    sums, ratio = ER.segment_ratios(canvas, labels, 3)
    assert sums[0][0] == 28 and ER.map_of(labels, ratio)[0, 0] == 0 and ER.map_of(labels, ratio)[1, 1] == 0


# ---- 2. the Gaussian ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 64), (37, 53), (5, 3), (1, 30), (13, 1)])
def test_gaussian_equals_scipy_bit_for_bit(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(shape[0])
    for plane in (rs.rand(*shape).astype(F32), (0.3 + 0.6 * (rs.rand(*shape) < 0.3)).astype(F32)):
        want = ndimage.gaussian_filter(plane, sigma=3)
        got = ER.gaussian_reflect(plane)
        assert want.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_gaussian_weights_are_the_kernels_constants():
    _filters = pytest.importorskip("scipy.ndimage._filters")
    src = open(os.path.join(PKG, "mstg_hip", "csrc", "segment_style.hip")).read()
    for sigma, radius in ((3, 12), (0.5, 2)):
        w = _filters._gaussian_kernel1d(sigma, 0, radius)[radius:]
        assert np.array_equal(w, ER.gaussian_weights(sigma, radius))
        for x in w:
            assert float(x).hex() in src, (sigma, float(x).hex())


# ---- 4. CLAHE and HSV -> RGB --------------------------------------------------------------------------------------------------------
def test_saturation_scale_float32_equals_float64():
    s = np.arange(256)
    a, b = ER.sat_scale(s, F32), ER.sat_scale(s, F64)
    assert np.array_equal(a, b) and a[0] == 0 and a[100] == 120 and a[213] == 255 and a[212] == 254
    frac = (s * 12 % 10) / 10.0  # the fractions are multiples of 0.2: never near a tie
    assert set(np.unique(frac)) <= {0.0, 0.2, 0.4, 0.6, 0.8}


def test_clahe_closed_forms():
    # a constant plane: one bin holds the tile, clip = 32 at a 64 x 64 tile, the excess is spread evenly
    v = np.full((512, 512), 77, dtype=np.uint8)
    luts = ER.clahe_luts(v)
    area, clip = 64 * 64, 32
    excess = area - clip
    batch, residual = divmod(excess, 256)
    assert (batch, residual) == (15, 224)
    hist = np.full(256, batch)
    hist[77] += clip
    hist[np.arange(0, 224)] += 1  # step = max(256 // 224, 1) = 1: the first 224 bins
    want = np.clip(np.rint(np.cumsum(hist).astype(F32) * (F32(255) / F32(area))), 0, 255)
    assert np.array_equal(luts[3, 4], want) and np.array_equal(luts[0, 0], luts[7, 7])
    out = ER.clahe(v)
    assert (out == want[77]).all()  # all tables equal: the interpolation returns the entry
    # two grey levels in a tile of 8 x 8 (clip = max(int(0.5), 1) = 1): both bins are cut to 1, excess 62 = batch 0, residual 62,
    # step 4: bins 0, 4, .., 244 get one each
    v = np.zeros((64, 64), dtype=np.uint8)
    v[:, ::2] = 200
    luts = ER.clahe_luts(v)
    hist = np.zeros(256, dtype=np.int64)
    hist[[0, 200]] = 1
    hist[np.arange(0, 62) * 4] += 1
    want = np.clip(np.rint(np.cumsum(hist).astype(F32) * (F32(255) / F32(64))), 0, 255)
    assert np.array_equal(luts[2, 5], want)
    with pytest.raises(NotImplementedError, match="H = 60"):
        ER.clahe_luts(np.zeros((60, 64), dtype=np.uint8))


def test_clahe_interpolation_is_exact_for_power_of_two_tiles():
    """tile sides 8, 32 and 64: every product and sum of the interpolation is exact in float32, so float64 gives the same bytes;
    at tile 5 x 9 the float32 path is inexact and only has to stay within one level of float64"""
    rs = np.random.RandomState(3)
    for side in (64, 256, 512):
        v = rs.randint(0, 256, size=(side, side)).astype(np.uint8)
        assert np.array_equal(ER.clahe(v, F32), ER.clahe(v, F64)), side
    v = rs.randint(0, 256, size=(40, 72)).astype(np.uint8)
    assert np.abs(ER.clahe(v, F32).astype(int) - ER.clahe(v, F64).astype(int)).max() <= 1


def test_hsv2rgb_closed_forms():
    for v in (0, 1, 128, 255):  # greys
        assert list(ER.hsv2rgb_u8(np.array([37]), np.array([0]), np.array([v]))[0]) == [v, v, v]
    pure = {0: (255, 0, 0), 30: (255, 255, 0), 60: (0, 255, 0), 90: (0, 255, 255), 120: (0, 0, 255), 150: (255, 0, 255)}
    for h, rgb in pure.items():
        assert tuple(ER.hsv2rgb_u8(np.array([h]), np.array([255]), np.array([255]))[0]) == rgb, h
    # h = 179: sector 5, the last one; red with a little blue
    r, g, b = ER.hsv2rgb_u8(np.array([179]), np.array([255]), np.array([255]))[0]
    assert (r, g) == (255, 0) and 0 < b <= 9
    # a hue outside [0, 180) counts as sector 0 with hf = 0
    assert tuple(ER.hsv2rgb_u8(np.array([200]), np.array([255]), np.array([255]))[0]) == (255, 0, 0)
    # the round trip of the 8-bit RGB -> HSV -> RGB stays within the hue's quantisation
    rs = np.random.RandomState(0)
    rgb = rs.randint(0, 256, size=(500, 3)).astype(np.uint8)
    back = ER.hsv2rgb_u8(*hsv_u8(rgb))
    assert np.abs(back.astype(int) - rgb.astype(int)).max() <= 4


def test_hsv2rgb_measured_shares():
    """over all h in [0, 180), s, v in [0, 256): the bytes a fused and a float64 evaluation change; the header states the shares"""
    h, s, v = np.meshgrid(np.arange(180), np.arange(256), np.arange(256), indexing="ij")
    base = ER.hsv2rgb_u8(h, s, v).astype(np.int16)
    shares = {}
    for how in ("fused", "float64"):
        d = np.abs(ER.hsv2rgb_u8(h, s, v, how).astype(np.int16) - base)
        shares[how] = float((d != 0).mean())
        print(f"hsv2rgb {how}: {100 * shares[how]:.3f} % of the bytes change, by at most {int(d.max())}")
        assert d.max() <= 1
    header = open(os.path.join(os.path.dirname(PKG), "include", "mstg_hip.h")).read()
    assert f"changes {100 * shares['fused']:.3f} % of the" in header and f"a float64 evaluation {100 * shares['float64']:.3f} %" in header


# ---- 5. the sharpening filter -------------------------------------------------------------------------------------------------------
def test_sharpen_closed_forms():
    img = np.full((5, 7, 3), 90, dtype=np.uint8)
    assert np.array_equal(ER.sharpen3(img), img)  # the weights sum to 1
    img[2, 3] = (100, 80, 255)
    out = ER.sharpen3(img)
    assert tuple(out[2, 3]) == (180, 0, 255) and tuple(out[2, 2]) == (80, 100, 0)
    img = np.zeros((3, 3, 3), dtype=np.uint8)
    img[0, 0] = 10  # a corner: reflect-101 never repeats it
    assert ER.sharpen3(img)[0, 0, 0] == 90 and ER.sharpen3(img)[1, 1, 0] == 0


# ---- the host segmentation ----------------------------------------------------------------------------------------------------------
def _segment(lib, img, scale=100.0, sigma=0.5, min_size=50):
    H, W = img.shape[:2]
    img = np.ascontiguousarray(img)
    labels = np.full((H, W), -1, dtype=np.int32)
    rc = lib.mstg_felzenszwalb_u8(img.ctypes.data, H, W, scale, sigma, min_size, labels.ctypes.data)
    return rc, labels


@pytest.mark.parametrize("shape", [(24, 32), (37, 53)])
def test_felzenszwalb_equals_the_restatement(lib, shape):
    h, w = shape
    halves = np.zeros((h, w, 3), dtype=np.uint8)
    halves[:, : w // 2] = (40, 90, 200)
    halves[:, w // 2:] = (220, 60, 30)  # flat halves: most costs are exactly 0, the stable order decides
    quads = np.zeros((h, w, 3), dtype=np.float64)  # four flat quadrants under noise of sigma 3: several segments, costs without ties
    quads[: h // 2, : w // 2], quads[: h // 2, w // 2:] = (200, 40, 40), (40, 200, 40)
    quads[h // 2:, : w // 2], quads[h // 2:, w // 2:] = (40, 40, 200), (220, 220, 60)
    quads = np.clip(np.rint(quads + np.random.RandomState(h).normal(0, 3, size=quads.shape)), 0, 255).astype(np.uint8)
    images = {"noise": quads, "constant": np.full((h, w, 3), 93, dtype=np.uint8), "halves": halves}
    for name, img in images.items():
        want = ER.felzenszwalb(img)
        rc, got = _segment(lib, img)
        assert rc == want.max() + 1, (name, rc)
        assert np.array_equal(got, want), name
        if name == "constant":
            assert rc == 1
        if name == "halves":
            assert rc == 2 and got[0, 0] == 0 and got[0, w - 1] == 1
        if name == "noise":
            assert rc > 1 and np.bincount(got.ravel()).min() >= 50
    rc, got = _segment(lib, images["noise"], scale=30.0, min_size=5)
    assert np.array_equal(got, ER.felzenszwalb(images["noise"], scale=30, min_size=5))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_host_side_refusals_name_the_value(lib):
    def err():
        return lib.mstg_last_error().decode()
    assert lib.mstg_segment_blend_map(1, 1, 1, 1, 64, 4, 1, 1, 1, 1, 1, 1 << 30, None) == -5 and "H = 1" in err()
    assert lib.mstg_segment_blend_map(1, 1, 1, 1025, 1024, 4, 1, 1, 1, 1, 1, 1 << 30, None) == -5 and "H * W = 1049600" in err()
    assert lib.mstg_segment_blend_map(1, 1, 1, 64, 64, 0, 1, 1, 1, 1, 1, 1 << 30, None) == -1 and "num_segments = 0" in err()
    assert lib.mstg_segment_blend_map_workspace_bytes(1, 1025, 1024, 4, 1) == 0 and "1049600" in err()
    assert lib.mstg_segment_blend_map_workspace_bytes(2, 64, 64, 4, 1) == 2 * 2 * 64 * 64 * 4
    for name, args in (("mstg_clahe_u8", (1, 1, 60, 64, 1, 1, 1 << 30, None)), ("mstg_hsv_enhance_u8", (1, 1, 64, 36, 1, 1, 1 << 30, None))):
        assert getattr(lib, name)(*args) == -5
        assert f"H = {args[2]}, W = {args[3]}" in err() and "multiples of 8" in err()
    assert lib.mstg_enhanced_style_finish(1, 1, 1, 1, 37, 53, 1, 1, 1, 1 << 30, None) == -5 and "H = 37, W = 53" in err()
    assert lib.mstg_enhanced_style_finish_workspace_bytes(1, 37, 53) == 0 and lib.mstg_clahe_workspace_bytes(3, 64, 64) == 3 * 64 * 256
    assert lib.mstg_sharpen3_u8(None, 1, 8, 8, None, None) == -1 and lib.mstg_sharpen3_u8(1, 0, 8, 8, 1, None) == -1 and "N = 0" in err()
    assert lib.mstg_gaussian_reflect_f32(1, 1, 8, 8, 1, 1, 16, None) != 0 and "workspace" in err()
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    assert _segment(lib, img, sigma=0.8)[0] == -5 and "sigma = 0.8" in err()
    assert _segment(lib, img, scale=0.0)[0] == -1 and "scale = 0" in err()
    assert lib.mstg_felzenszwalb_u8(None, 8, 8, 100.0, 0.5, 50, None) == -1


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------
def test_drop_in_imports_without_cv2_skimage_torchvision():
    code = ("import sys\n"
            "for m in ('cv2', 'skimage', 'torchvision', 'matplotlib'): sys.modules[m] = None\n"
            f"sys.path.insert(0, {PKG!r})\n"
            "import enhanced_local_style as E\n"
            "for n in ('load_model', 'preprocess_image', 'standard_postprocess', 'get_segmentation_mask', 'analyze_segments',\n"
            "          'determine_blend_ratios', 'enhanced_local_style_transfer', 'main'):\n"
            "    assert callable(getattr(E, n)), n\n"
            "import numpy as np\n"
            "for m in ('slic', 'quickshift'):\n"
            "    try:\n"
            "        E.get_segmentation_mask(np.zeros((8, 8, 3), np.uint8), method=m)\n"
            "    except NotImplementedError as e:\n"
            "        assert m in str(e)\n"
            "    else:\n"
            "        raise SystemExit('no refusal for ' + m)\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
