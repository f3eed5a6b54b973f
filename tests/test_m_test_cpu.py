"""CPU: the Frechet distance and the display finish of the reference's m_test.py as include/mstg_hip.h defines them.  The numpy
restatement (tests/fid_ref.py) against the reference's own formula (np.cov + scipy.linalg.sqrtm), the restated Jacobi's sweep
counts against the committed bound, the C entries' refusals (host side: no kernel is launched), the restated equalizeHist, and
the drop-in's surface."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import display_finish_ref as DR
import fid_ref as FR
from conftest import PKG, ROOT

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


def err(lib):
    return lib.mstg_last_error().decode()


def special_draws():
    """(name, x1, x2): a zero-variance column, identical sets"""
    x1, x2 = FR.draw(48, 40, 13, 5, F64)
    x1[:, 4] = 0.25
    x2[:, 4] = 0.25
    y1, _ = FR.draw(24, 24, 64, 3, F64)
    return [("constant column", x1, x2), ("identical sets", y1, y1.copy())]


def all_draws():
    out = []
    for n1, n2, d in FR.CASES:
        for dt in (F32, F64):
            out.append((f"{(n1, n2, d)} {dt.__name__}",) + FR.draw(n1, n2, d, 7 + n1 + d, dt))
    return out + special_draws()


# ---- the form against the reference's formula ------------------------------------------------------------------------------------------
def sqrtm_bound(x1, x2, parts):
    """What the reference's own evaluation can be off by, from its arithmetic:
      * its float64 products and traces: 8 K eps (ssdiff + tr1 + tr2), K = max(n1, n2, d) accumulated terms;
      * sqrtm of a singular product: S1 S2 (d x d) has at least d - min(n1, n2) + 1 zero eigenvalues, which its Schur form holds to
        eps ||S1 S2||; the square root of each is then off by up to sqrt(eps ||S1|| ||S2||), and the trace adds them;
      * float32 features: its mean(0) is a float32 (pairwise) sum, relative error (1 + log2 n) eps32 in each mean, which enters
        ssdiff as 2 |mu1 - mu2| times the error of the difference."""
    n1, n2, d = x1.shape[0], x2.shape[0], x1.shape[1]
    scale = parts["ssdiff"] + parts["tr1"] + parts["tr2"]
    bound = 8 * max(n1, n2, d) * FR.EPS * scale
    nulls = max(d - (min(n1, n2) - 1), 0)
    if nulls:
        A, B = FR.factors(x1, x2)[:2]
        s1, s2 = np.linalg.norm(A, 2) ** 2, np.linalg.norm(B, 2) ** 2
        bound += nulls * math.sqrt(FR.EPS * s1 * s2)
    if x1.dtype == F32:
        eps32 = float(np.finfo(F32).eps)
        mu = np.linalg.norm(x1.astype(F64).mean(0)) + np.linalg.norm(x2.astype(F64).mean(0))
        bound += 2 * math.sqrt(parts["ssdiff"]) * (1 + math.log2(max(n1, n2))) * eps32 * mu
    return bound


@pytest.mark.parametrize("name,x1,x2", all_draws(), ids=[d[0] for d in all_draws()])
def test_restatement_equals_the_sqrtm_formula(name, x1, x2):
    parts = FR.frechet(x1, x2)
    ref = FR.reference_fid(x1, x2)
    bound = sqrtm_bound(x1, x2, parts)
    print(f"{name}: fid {parts['fid']:.12g}, sqrtm formula {ref:.12g}, |diff| {abs(parts['fid'] - ref):.3g}, bound {bound:.3g}")
    assert abs(parts["fid"] - ref) <= bound


def test_sqrtm_formula_equals_the_references_own_calculate_fid(gold_dir):
    """tests/golden/fid_cases.npz holds what the reference's m_test.calculate_fid itself returned on these draws
    (tools/make_fid_golden.py): the formula as written in tests/fid_ref.py, and the restatement, lie within the reference's own
    error of it.  The reference refuses one feature (np.cov gives a scalar), so (2, 2, 1) has no entry."""
    gold = np.load(os.path.join(gold_dir, "fid_cases.npz"))
    stored = dict(zip(gold["names"].tolist(), gold["fid"].tolist()))
    draws = {name: (x1, x2) for name, x1, x2 in all_draws()}
    assert sorted(stored) == sorted(n for n in draws if not n.startswith("(2, 2, 1)"))
    for name, want in stored.items():
        x1, x2 = draws[name]
        parts = FR.frechet(x1, x2)
        bound = sqrtm_bound(x1, x2, parts)
        assert abs(FR.reference_fid(x1, x2) - want) <= bound, name  # another BLAS may round sqrtm's noise differently
        assert abs(parts["fid"] - want) <= bound, name


def test_identical_sets_give_zero_on_the_scale_of_the_traces():
    _, x1, x2 = special_draws()[1]
    p = FR.frechet(x1, x2)
    assert p["ssdiff"] == 0.0 and p["tr1"] == p["tr2"]
    assert abs(p["fid"]) <= 64 * FR.EPS * (p["tr1"] + p["tr2"])


# ---- the Jacobi and its sweep bound ----------------------------------------------------------------------------------------------------
def test_restated_jacobi_converges_within_the_committed_bound():
    """MSTG_FRECHET_MAX_SWEEPS is twice the largest count seen here (include/mstg_hip.h)."""
    counts = {}
    for name, x1, x2 in all_draws() + [("(100, 100, 32) float64",) + FR.draw(100, 100, 32, 139, F64)]:
        if name.endswith("float64") and name.startswith(str(FR.CASES[-1])):
            continue  # the cap case once (22 sweeps in float32 and in float64): it is the slow one in Python
        j, want = FR.frechet_jacobi(x1, x2), FR.frechet(x1, x2)
        counts[name] = j["sweeps"]
        assert j["converged"], name
        K = max(x1.shape[0], x2.shape[0], x1.shape[1])
        assert abs(j["nuclear"] - want["nuclear"]) <= K * FR.EPS * (want["ssdiff"] + want["tr1"] + want["tr2"]), name
    print(counts)
    assert 2 * max(counts.values()) == FR.MAX_SWEEPS


def test_jacobi_pairing_and_small_matrices():
    for q in (1, 2, 3, 7, 8, 33):
        rounds = FR.round_robin(q)
        seen = sorted(p for r in rounds for p in r)
        assert seen == [(a, b) for a in range(q) for b in range(a + 1, q)]  # every pair exactly once a sweep
        for r in rounds:
            cols = [c for p in r for c in p]
            assert len(cols) == len(set(cols))                              # disjoint inside a round
    rng = np.random.RandomState(0)
    for m, n in ((1, 1), (1, 5), (5, 1), (2, 2), (7, 5), (5, 7), (33, 16)):
        M = rng.randn(m, n)
        s, sweeps, ok = FR.jacobi_singular_values(M)
        want = np.linalg.svd(M, compute_uv=False)
        assert ok and s.shape == want.shape and np.abs(s - want).max() <= max(m, n) * FR.EPS * want[0]
    s, sweeps, ok = FR.jacobi_singular_values(np.full((4, 3), np.nan))
    assert not ok and sweeps == 1 and np.isnan(s).all()  # a NaN never rotates: non-finite out, not converged, no endless loop


def test_constants_agree():
    from mstg_hip import _lib, metrics
    text = open(os.path.join(ROOT, "include", "mstg_hip.h")).read()
    samples = int(re.search(r"#define MSTG_FRECHET_MAX_SAMPLES (\d+)", text).group(1))
    sweeps = int(re.search(r"#define MSTG_FRECHET_MAX_SWEEPS (\d+)", text).group(1))
    assert (samples, sweeps) == (FR.MAX_SAMPLES, FR.MAX_SWEEPS) == (_lib.FRECHET_MAX_SAMPLES, _lib.FRECHET_MAX_SWEEPS)
    assert (metrics.MAX_SAMPLES, metrics.MAX_SWEEPS) == (samples, sweeps) and samples >= 256
    assert "restated as recalled, not compared with an OpenCV binary" in text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"MSTG_FRECHET_MAX_SWEEPS = {sweeps}" in design


# ---- refusals: every one names its value and returns before a launch (the pointers are not device pointers) ----------------------------
def test_frechet_refusals_name_the_value(lib):
    big = 1 << 40
    f = lib.mstg_frechet_distance
    assert f(8, 16, 0, 1, 5, 3, 24, 32, 40, big, None) == -1 and "n1 = 1, n2 = 5" in err(lib)
    assert f(8, 16, 0, 5, 1, 3, 24, 32, 40, big, None) == -1 and "n1 = 5, n2 = 1" in err(lib)
    assert f(8, 16, 0, 5, 5, 0, 24, 32, 40, big, None) == -1 and "d = 0" in err(lib)
    cap = FR.MAX_SAMPLES
    assert f(8, 16, 0, cap + 1, cap + 1, 3, 24, 32, 40, big, None) == -5
    assert f"min(n1, n2) = {cap + 1}" in err(lib) and "d x d form" in err(lib) and "not built" in err(lib)
    assert f(8, 16, 0, cap + 1, 1000, 3, 24, 32, 40, big, None) == -5 and f"min(n1, n2) = {cap + 1}" in err(lib)
    assert f(8, 16, 0, 1 << 20, 4, 1 << 12, 24, 32, 40, big, None) == -5 and "n1 * d = 4294967296" in err(lib)
    assert f(None, 16, 0, 5, 5, 3, 24, 32, 40, big, None) == -1 and "null" in err(lib)
    assert f(8, 16, 0, 5, 5, 3, None, 32, 40, big, None) == -1 and "null" in err(lib)
    assert f(8, 16, 0, 5, 5, 3, 24, None, 40, big, None) == -1 and "null" in err(lib)
    need = lib.mstg_frechet_workspace_bytes(5, 5, 3)
    assert need == 8 * FR.workspace_doubles(5, 5, 3)
    assert f(8, 16, 0, 5, 5, 3, 24, 32, None, big, None) == -4 and f"need {need}" in err(lib)
    assert f(8, 16, 0, 5, 5, 3, 24, 32, 40, need - 1, None) == -4 and f"workspace of {need - 1} bytes, need {need}" in err(lib)
    assert f(8, 16, 1, 5, 5, 3, 24, 32, 44, big, None) == -2 and "aligned" in err(lib)
    assert f(4, 16, 1, 5, 5, 3, 24, 32, 40, big, None) == -2  # float64 features on a 4-byte boundary
    assert lib.mstg_frechet_workspace_bytes(1, 5, 3) == 0 and "n1 = 1" in err(lib)
    assert lib.mstg_frechet_workspace_bytes(cap + 1, cap + 1, 3) == 0 and "MSTG_FRECHET_MAX_SAMPLES" in err(lib)
    # a set larger than the cap is fine as long as the other one is not
    assert lib.mstg_frechet_workspace_bytes(cap, 5000, 16) == 8 * FR.workspace_doubles(cap, 5000, 16)


def test_workspace_grows_with_n_and_d(lib):
    w = lib.mstg_frechet_workspace_bytes
    assert w(10, 10, 8) < w(11, 10, 8) < w(11, 11, 8) < w(11, 11, 9)
    assert w(100, 100, 2048) == 8 * (2 * 100 * 2048 + 3 * 2048 + 2 * 100 * 100 + 100 + 1)
    s = lib.mstg_singular_values_workspace_bytes
    assert s(7, 5) == 8 * 36 and s(7, 5) < s(8, 5) < s(8, 6)


def test_singular_values_refusals(lib):
    big, cap = 1 << 40, FR.MAX_SAMPLES
    f = lib.mstg_singular_values
    assert f(8, 0, 5, 16, 24, 32, big, None) == -1 and "m = 0, n = 5" in err(lib)
    assert f(8, cap + 1, cap + 2, 16, 24, 32, big, None) == -5 and f"min(m, n) = {cap + 1}" in err(lib)
    assert f(None, 4, 4, 16, 24, 32, big, None) == -1 and "null" in err(lib)
    assert f(8, 4, 4, 16, 24, None, big, None) == -4 and f(8, 4, 4, 16, 24, 32, 8 * 17 - 1, None) == -4 and "need 136" in err(lib)
    assert lib.mstg_singular_values_workspace_bytes(cap + 1, cap + 1) == 0 and lib.mstg_singular_values_workspace_bytes(cap, 10 ** 6) > 0


def test_display_finish_refusals(lib):
    big = 1 << 40
    g = lib.mstg_gamma_u8
    assert g(None, 0, 1, 8, 8, 1.1, 4096, None) == -1 and "null" in err(lib)
    assert g(8, 0, 0, 8, 8, 1.1, 4096, None) == -1 and "N = 0" in err(lib)
    assert g(8, 0, 1, 0, 8, 1.1, 4096, None) == -1 and "H = 0" in err(lib)
    assert g(8, 0, 1, 1 << 15, 1 << 15, 1.1, 1 << 50, None) == -5 and "H * W * 3 = 3221225472" in err(lib)
    assert g(8, 0, 1, 8, 8, 0.0, 4096, None) == -1 and "gamma = 0" in err(lib)
    assert g(8, 0, 1, 8, 8, float("nan"), 4096, None) == -1 and "gamma = nan" in err(lib)
    assert g(6, 0, 1, 8, 8, 1.1, 4096, None) == -2 and g(7, 1, 1, 8, 8, 1.1, 4096, None) == -2
    assert g(4096, 0, 1, 8, 8, 1.1, 4096 + 64, None) == -1 and "overlaps" in err(lib)
    e = lib.mstg_equalize_luma_u8
    assert e(None, 1, 8, 8, 4096, 8192, big, None) == -1 and "null" in err(lib)
    assert e(16, 1, 8, 0, 4096, 8192, big, None) == -1 and "W = 0" in err(lib)
    need = lib.mstg_equalize_luma_workspace_bytes(3, 37, 53)
    assert need == 3 * 256 * 4 + 3 * 256
    assert lib.mstg_equalize_luma_workspace_bytes(1, 256, 256) == 16 * 1024 + 256
    assert lib.mstg_equalize_luma_workspace_bytes(1, 4096, 4096) == 256 * 1024 + 256  # the chunks of an image stop at 256
    assert lib.mstg_equalize_luma_workspace_bytes(0, 8, 8) == 0
    assert e(16, 3, 37, 53, 1 << 20, None, big, None) == -4 and e(16, 3, 37, 53, 1 << 20, 1 << 21, need - 1, None) == -4
    assert f"need {need}" in err(lib)
    assert e(16, 3, 37, 53, 1 << 20, (1 << 21) + 2, big, None) == -2
    assert e(4096, 1, 8, 8, 4096 + 100, 1 << 20, 2000, None) == -1 and "overlaps" in err(lib)
    assert e(4096, 1, 8, 8, 1 << 20, 4096 + 100, 2000, None) == -1 and "overlaps" in err(lib)


def test_python_refusals():
    import torch
    from mstg_hip import image as dimg, metrics
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.frechet_distance(torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="torch tensor"):
        metrics.frechet_distance(np.zeros((4, 3)), np.zeros((4, 3)))
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.singular_values(torch.zeros(4, 3, dtype=torch.float64))
    for fn in (dimg.gamma_u8, dimg.display_finish):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(torch.zeros(3, 8, 8))
    with pytest.raises(RuntimeError, match="uint8"):
        dimg.equalize_luma_u8(torch.zeros(8, 8, 3, dtype=torch.uint8))


# ---- the restated 8-bit steps ----------------------------------------------------------------------------------------------------------
def test_equalize_hist_restated():
    const = np.full((5, 7), 93, np.uint8)
    assert np.array_equal(DR.equalize_hist(const), const)                      # a constant plane stays
    two = np.where(np.arange(35).reshape(5, 7) % 3 == 0, 40, 200).astype(np.uint8)
    assert sorted(np.unique(DR.equalize_hist(two)).tolist()) == [0, 255]       # two levels -> {0, 255}
    rng = np.random.RandomState(1)
    for plane in (rng.randint(0, 256, (64, 64)), rng.randint(90, 140, (37, 53)), (rng.rand(16, 16) ** 3 * 255)):
        lut = DR.equalize_lut(plane.astype(np.uint8))
        assert np.all(np.diff(lut.astype(int)) >= 0) and lut[plane.astype(np.uint8).max()] == 255  # monotone, the top level -> 255
        assert lut[plane.astype(np.uint8).min()] == 0
    # a flat histogram over all 256 levels: the table is the identity
    flat = np.repeat(np.arange(256, dtype=np.uint8), 4).reshape(32, 32)
    assert np.array_equal(DR.equalize_lut(flat), np.arange(256))


def test_yuv_round_trip_and_primaries():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    Y, U, V = DR.rgb2yuv(grey)
    assert np.array_equal(Y, np.arange(256)) and np.all(U == 128) and np.all(V == 128)
    assert np.array_equal(DR.yuv2rgb(Y, U, V), grey)
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]], np.uint8)
    Y, U, V = DR.rgb2yuv(prim)
    assert Y.tolist() == [76, 150, 29, 255, 0] and U.tolist() == [91, 54, 239, 128, 128] and V.tolist() == [255, 0, 103, 128, 128]
    rng = np.random.RandomState(2)
    img = rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    Y, U, V = DR.rgb2yuv(img)
    back = DR.yuv2rgb(Y, U, V).astype(int)
    ok = (U > 0) & (U < 255) & (V > 0) & (V < 255)
    assert ok.sum() > 2000 and np.abs(back - img)[ok].max() <= 2  # unsaturated U, V: back within the rounding of two 8-bit conversions


def test_gamma_restated():
    y = np.array([-1.0, 1.0, 0.0, -3.0, 2.5, np.nan, 0.5], F32).reshape(1, 1, 1, 7).repeat(3, axis=1)
    want = [0, 255, int(F32(0.5 ** 1.1) * F32(255)), 0, 255, 0, int(F32(0.75 ** 1.1) * F32(255))]
    assert DR.gamma_u8(y)[0, 0, :, 0].tolist() == want
    assert DR.gamma_u8(y.astype(np.float16)).tolist() == DR.gamma_u8(y).tolist()
    v = DR.gamma_inputs(np.linspace(-1, 1, 1001, dtype=F32))
    assert DR.gamma_margin_ulps(v) > 0
    assert DR.process_image(np.zeros((3, 4, 5), F32)).shape == (4, 5, 3) and DR.process_image(np.zeros((3, 4, 5), F32)).dtype == F64


# ---- the drop-in -----------------------------------------------------------------------------------------------------------------------
def test_drop_in_surface_without_cv2_torchvision_matplotlib_scipy():
    code = ("import sys\n"
            "for m in ('cv2', 'torchvision', 'matplotlib', 'scipy', 'tqdm'): sys.modules[m] = None\n"
            f"sys.path.insert(0, {PKG!r})\n"
            "import m_test as M\n"
            "assert callable(M.calculate_fid) and callable(M.process_image) and callable(M.run_model)\n"
            "assert not [n for n in dir(M) if n.lower().startswith('test')], dir(M)\n"
            "try:\n"
            "    M.run_model('models', 'data', 'out')\n"
            "except NotImplementedError as e:\n"
            "    assert 'InceptionV3' in str(e) and 'Inception_V3_Weights' in str(e) and 'feature_extractor' in str(e)\n"
            "else:\n"
            "    raise SystemExit('run_model ran without an extractor')\n"
            "import os\n"
            "assert not os.path.exists('out')\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=os.path.join(ROOT, "tests"))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
