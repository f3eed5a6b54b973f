"""CPU: the advanced transform (csrc/advanced_transform.hip, mstg_hip.image.process_advanced, advanced_transform.py) up to the launch.
The host table entries against the numpy restatement (tests/advanced_transform_ref.py), the Lab round trip and the distance of the
inverse from a float64 CIE inverse over all 2^24 colours (the numbers include/mstg_hip.h states), a and b against
tests/color_blocks_ref.py, the sigma 3 taps with their tie margin, the float32 gains against float64, the K-means restatement
against scikit-learn's Lloyd iteration, the host-side refusals by name, and the drop-in's imports."""
import subprocess
import sys

import numpy as np
import pytest

import advanced_transform_ref as AR
import color_blocks_ref as CR
import enhanced_local_style_ref as ER
from app_local_style_ref import hsv_u8
from conftest import PKG

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


def err(lib):
    return lib.mstg_last_error().decode()


# ---- host tables --------------------------------------------------------------------------------------------------------------------
def test_lab_inverse_tables_equal_the_restatement(lib):
    from mstg_hip import _lib
    t = np.full(_lib.LAB_INV_TABLE_U16, 0xffff, dtype=np.uint16)
    assert lib.mstg_lab_inverse_tables(t.ctypes.data) == 0
    want = AR.lab_inverse_flat()
    assert len(want) == 3 * 256 + AR.CUBE_N + 9 + AR.ENC_N <= _lib.LAB_INV_TABLE_U16
    assert np.array_equal(t[:len(want)].astype(np.int64), want & 0xffff) and not t[len(want):].any()
    fy, da, db, cube, D, enc = AR.lab_inverse_tables()
    assert cube.max() == 36160 < 65536 and fy.max() == 32768 and enc[0] == 0 and enc[-1] == 255 and cube[0] == 0
    assert np.abs(D).max() <= 13273 and np.abs(D.sum(axis=1) - 4096).max() <= 1  # white maps to white
    margin = min(float(np.abs(np.abs(v - np.floor(v)) - 0.5).min()) for v in AR.lab_inverse_tables_unrounded())
    print(f"\n  inverse Lab tables: smallest distance from a rounding tie {margin:.3g}")
    assert margin > 1e-9  # a last-bit difference of pow cannot change an entry
    assert lib.mstg_lab_inverse_tables(None) == -1


def test_sigma_taps_equal_the_restatement(lib):
    for sigma, ksize in ((3.0, 19), (0.5, 5), (1.0, 7), (2.0, 13), (5.0, 31), (4.9, 31), (0.1, 3)):
        taps, margin = np.full(31, -1, dtype=np.int32), np.zeros(1)
        assert lib.mstg_gaussian_sigma_taps(sigma, taps.ctypes.data, margin.ctypes.data) == ksize == AR.sigma_ksize(sigma)
        want, want_margin = AR.sigma_taps(sigma)
        assert taps[:ksize].tolist() == want and not taps[ksize:].any() and sum(want) == 256 and min(want) >= 0
        assert abs(margin[0] - want_margin) < 1e-9
    taps, margin = AR.sigma_taps(3.0)
    print(f"\n  sigma 3: {taps}, smallest distance from a rounding tie {margin:.4f}")
    assert taps == [0, 1, 3, 4, 9, 14, 20, 28, 32, 34, 32, 28, 20, 14, 9, 4, 3, 1, 0]
    assert margin > 0.09  # a last-bit difference in exp cannot move a tap
    assert 255 * 256 <= 65535  # the row sums stay exact in 16 bits


# ---- Lab ----------------------------------------------------------------------------------------------------------------------------
def test_lab_round_trip_over_all_colours():
    """The numbers of include/mstg_hip.h: the distance of the integer inverse from the float64 CIE inverse of the same Lab bytes, and
    the round trip RGB -> Lab -> RGB, over all 2^24 colours; a and b are those of tests/color_blocks_ref.py."""
    tabs, inv = CR.lab_tables(), AR.lab_inverse_tables()
    g, b = np.mgrid[0:256, 0:256]
    worst = worst64 = 0
    total = total64 = above1 = 0
    dist = 0.0
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], axis=-1).astype(np.uint8)
        lab = AR.lab_u8(rgb, tabs)
        if r % 51 == 0:
            a_ref, b_ref = CR.lab_ab(rgb, tabs)
            assert np.array_equal(lab[..., 1], a_ref) and np.array_equal(lab[..., 2], b_ref)
        back = AR.lab2rgb_u8(lab, inv).astype(np.int64)
        f = AR.lab2rgb_float64(lab)
        d = np.abs(back - rgb)
        d64 = np.abs(np.rint(f) - rgb)
        worst, worst64 = max(worst, int(d.max())), max(worst64, int(d64.max()))
        total, total64, above1 = total + int(d.sum()), total64 + float(d64.sum()), above1 + int((d > 1).sum())
        dist = max(dist, float(np.abs(back - f).max()))
    n = 3 * 2 ** 24
    print(f"\n  Lab over 2^24 colours: inverse within {dist:.3f} of float64; round trip worst {worst}, mean {total / n:.4f}, "
          f"{100 * above1 / n:.2f} % above one level; the float64 inverse rounded: worst {worst64}, mean {total64 / n:.4f}")
    assert 2.06 < dist < 2.07
    assert worst == 27 and worst64 == 27
    assert abs(total / n - 0.702) < 0.001 and abs(total64 / n - 0.699) < 0.001 and abs(100 * above1 / n - 9.8) < 0.05


def test_lab_primaries_and_every_triple_defined():
    prim = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=np.uint8)
    assert AR.lab_u8(prim).tolist() == [[0, 128, 128], [255, 128, 128], [136, 208, 195], [224, 42, 211], [82, 207, 20]]
    assert AR.lab2rgb_u8(AR.lab_u8(prim[:2])).tolist() == prim[:2].tolist()
    corners = np.array([[L, a, b] for L in (0, 255) for a in (0, 255) for b in (0, 255)], dtype=np.uint8)
    out = AR.lab2rgb_u8(corners)
    assert out.dtype == np.uint8 and out.shape == (8, 3)
    assert np.abs(out.astype(F64) - AR.lab2rgb_float64(corners)).max() < 2.07


# ---- gains --------------------------------------------------------------------------------------------------------------------------
def test_gains_float32_against_float64():
    v = np.arange(256)
    assert np.array_equal(AR.gain_u8(v, 1.2, F32), AR.gain_u8(v, 1.2, F64)) and np.array_equal(AR.gain_u8(v, 1.2), ER.sat_scale(v))
    differ = v[AR.gain_u8(v, 1.1, F32) != AR.gain_u8(v, 1.1, F64)]
    assert differ.tolist() == [55, 95, 115, 175, 195, 215]
    assert np.array_equal(AR.gain_u8(v, 1.0), v)


def test_gain_with_clahe_put_back_is_hsv_enhance():
    img = AR.smooth(64, 64, 3)
    h, s, v = hsv_u8(img)
    want = ER.hsv_enhance(img)
    got = ER.hsv2rgb_u8(h, AR.gain_u8(s, 1.2), ER.clahe(v.astype(np.uint8)).astype(np.int64))
    assert np.array_equal(got, want)
    assert np.array_equal(AR.hsv_gain_u8(img, 1.2, 1.0), ER.hsv2rgb_u8(h, ER.sat_scale(s), v))


# ---- K-means ------------------------------------------------------------------------------------------------------------------------
def test_kmeans_equals_sklearn_lloyd_on_separated_blobs():
    from sklearn.cluster import KMeans
    rng = np.random.RandomState(7)
    means = np.array([[40, 60, 200], [200, 50, 40], [90, 220, 100], [230, 230, 30]])
    which = rng.randint(0, 4, size=24 * 30)
    img = (means[which] + rng.randint(-12, 13, size=(24 * 30, 3))).astype(np.uint8).reshape(24, 30, 3)
    centers0 = (means + np.array([[9, -7, 5], [-8, 6, 9], [7, 7, -9], [-6, -9, 8]])).astype(F32)
    labels, cen, comp, _ = AR.kmeans_u8(img, K=4, attempts=1, iters=10, eps=0.0, centers0=centers0)
    px = img.reshape(-1, 3)
    _, _, used = AR.km_attempt(px, centers0, 10, 0.0)
    assert used < 10  # converged inside 10 iterations: the centres stopped moving
    for c in (centers0, cen):  # no distance tie, at the first and at the last assignment
        d = np.sort(((px.astype(F64)[:, None, :] - c.astype(F64)[None]) ** 2).sum(axis=2), axis=1)
        assert (d[:, 1] - d[:, 0]).min() > 1.0
    km = KMeans(n_clusters=4, init=centers0.astype(F64), n_init=1, max_iter=10, tol=0, algorithm="lloyd").fit(px.astype(F64))
    assert np.array_equal(km.labels_, labels.reshape(-1))
    assert np.array_equal(labels.reshape(-1), which)  # the order of the initial centres, no renumbering
    assert np.abs(km.cluster_centers_ - cen).max() < 1e-4 and abs(km.inertia_ - comp) < 1e-6 * comp


def test_kmeans_attempts_ties_and_empty_clusters():
    img = AR.smooth(20, 28, 5)
    labels, cen, comp, a = AR.kmeans_u8(img, K=5, attempts=10, seed=0)
    px = img.reshape(-1, 3)
    lo, hi = px.min(axis=0).astype(F32), px.max(axis=0).astype(F32)
    starts = [lo + u * (hi - lo) for u in AR.uniforms(0, 10, 5)]
    comps = [AR.km_attempt(px, s, 10, 1.0)[1] for s in starts]
    assert a == int(np.argmin(comps)) and comp == comps[a]
    solo = AR.kmeans_u8(img, K=5, attempts=1, centers0=starts[a])
    assert np.array_equal(solo[0], labels) and np.array_equal(solo[1], cen) and solo[2] == comp
    flat = np.full((6, 7, 3), 93, dtype=np.uint8)  # lo == hi: every centre equals the colour, label 0 wins every tie
    labels, cen, comp, _ = AR.kmeans_u8(flat, K=5, attempts=2, seed=1)
    assert not labels.any() and np.array_equal(cen, np.full((5, 3), 93, dtype=F32)) and comp == 0.0
    with pytest.raises(NotImplementedError, match="K = 17"):
        AR.kmeans_u8(flat, K=17)
    with pytest.raises(NotImplementedError, match="attempts = 0"):
        AR.kmeans_u8(flat, attempts=0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_host_side_refusals_name_the_value(lib):
    big = 1 << 30
    taps = np.zeros(31, dtype=np.int32)
    assert lib.mstg_gaussian_sigma_taps(5.1, taps.ctypes.data, None) == -5 and "ksize = 33" in err(lib)
    assert lib.mstg_gaussian_sigma_taps(0.0, taps.ctypes.data, None) == -1 and "sigma = 0" in err(lib)
    assert lib.mstg_gaussian_sigma_u8(1, 1, 8, 8, taps.ctypes.data, 33, 1, 1, big, None) == -5 and "ksize = 33" in err(lib)
    assert lib.mstg_gaussian_sigma_u8(1, 1, 8, 8, taps.ctypes.data, 4, 1, 1, big, None) == -5 and "ksize = 4" in err(lib)
    assert lib.mstg_gaussian_sigma_u8(1, 1, 8, 8, taps.ctypes.data, 3, 1, 1, big, None) == -1 and "sum to 0" in err(lib)
    assert lib.mstg_kmeans_u8(1, 1, 8, 8, 0, 10, 10, 1.0, 1, None, 1, 1, 1, 1, 1, big, None) == -5 and "K = 0" in err(lib)
    assert lib.mstg_kmeans_u8(1, 1, 8, 8, 17, 10, 10, 1.0, 1, None, 1, 1, 1, 1, 1, big, None) == -5 and "K = 17" in err(lib)
    assert lib.mstg_kmeans_u8(1, 1, 8, 8, 5, 17, 10, 1.0, 1, None, 1, 1, 1, 1, 1, big, None) == -5 and "attempts = 17" in err(lib)
    assert lib.mstg_kmeans_u8(1, 1, 8, 8, 5, 0, 10, 1.0, 1, None, 1, 1, 1, 1, 1, big, None) == -5 and "attempts = 0" in err(lib)
    assert lib.mstg_kmeans_u8(1, 1, 8, 8, 5, 10, 0, 1.0, 1, None, 1, 1, 1, 1, 1, big, None) == -5 and "iters = 0" in err(lib)
    assert lib.mstg_kmeans_u8(1, 1, 8, 8, 5, 2, 10, 1.0, None, 16, 32, 48, 64, 80, 96, big, None) == -1 and "centers0" in err(lib)
    assert lib.mstg_kmeans_u8(1, 1, 8, 8, 5, 2, 10, 1.0, 16, 16, 32, 48, 64, 80, 96, big, None) == -1 and "either" in err(lib)
    assert lib.mstg_kmeans_workspace_bytes(1, 17, 1) == 0 and "K = 17" in err(lib)
    assert lib.mstg_kmeans_workspace_bytes(2, 5, 10) > 2 * 10 * 16 * (7 * 8 + 3 * 4)
    for name, args in (("mstg_contrast_enhanced_finish", (1, 1, 60, 64, 1, 1, 1.2, 1.0, 1, 1, big, None)),
                       ("mstg_contrast_enhanced_finish", (1, 1, 64, 36, 1, 1, 1.2, 1.0, 1, 1, big, None))):
        assert getattr(lib, name)(*args) == -5
        assert f"H = {args[2]}, W = {args[3]}" in err(lib) and "multiples of 8" in err(lib)
    assert lib.mstg_contrast_enhanced_finish_workspace_bytes(1, 37, 53) == 0
    assert lib.mstg_contrast_enhanced_finish_workspace_bytes(3, 64, 64) == 3 * 64 * 256
    ratios = np.array([0.8, 0.4, 0.6])
    assert lib.mstg_region_blend_u8(1, 1, 4, 1, 8, 8, ratios.ctypes.data, 0, 1, None) == -1 and "count = 0" in err(lib)
    assert lib.mstg_region_blend_u8(1, 1, 4, 1, 8, 8, ratios.ctypes.data, 17, 1, None) == -1 and "count = 17" in err(lib)
    w = np.ones(9, dtype=F32)
    assert lib.mstg_fuse_scales_u8(1, 9, 1, 8, 8, w.ctypes.data, 1.1, 1, None) == -5 and "S = 9" in err(lib)
    assert lib.mstg_hsv_gain_u8(1, 1, 8, 8, -1.0, 1.0, 1, None) == -1 and "s_gain = -1" in err(lib)
    assert lib.mstg_lab_u8(None, 1, 8, 8, None, None, None) == -1 and lib.mstg_lab2rgb_u8(1, 0, 8, 8, 2, 1, None) == -1 and "N = 0" in err(lib)
    # out overlapping the input
    assert lib.mstg_lab_u8(4096, 1, 8, 8, 2, 4096 + 64, None) == -1 and "overlaps" in err(lib)
    assert lib.mstg_hsv_gain_u8(4096, 1, 8, 8, 1.2, 1.0, 4096, None) == -1 and "overlaps" in err(lib)
    taps3 = np.array([64, 128, 64] + [0] * 28, dtype=np.int32)
    assert lib.mstg_detail_enhanced_finish(4096, 8192, 1, 8, 8, 2, 4, taps3.ctypes.data, 3, 1.2, 1.1, 8192 + 8, 1 << 20, big, None) == -1
    assert "overlaps" in err(lib)


def test_python_refusals():
    from mstg_hip import image as dimg
    with pytest.raises(RuntimeError, match="ksize = 33"):
        dimg.gaussian_sigma_taps(5.1)
    assert dimg.gaussian_sigma_taps(3.0)[0] == 19
    with pytest.raises(ValueError, match="posterize"):
        dimg.process_advanced(None, None, "posterize")


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------
def test_drop_in_imports_without_cv2_torchvision_matplotlib():
    code = ("import sys\n"
            "for m in ('cv2', 'skimage', 'torchvision', 'matplotlib'): sys.modules[m] = None\n"
            f"sys.path.insert(0, {PKG!r})\n"
            "import advanced_transform as A\n"
            "for n in ('load_model', 'generate_with_different_settings', 'standard_postprocess', 'contrast_enhanced_postprocess',\n"
            "          'multi_scale_fusion', 'detail_enhanced_postprocess', 'local_style_transfer', 'main'):\n"
            "    assert callable(getattr(A, n)), n\n"
            "try:\n"
            "    A.main(['--image'])\n"
            "except SystemExit:\n"
            "    pass\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
