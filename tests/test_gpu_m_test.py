"""The Frechet distance and the display finish of the reference's m_test.py on the device (csrc/frechet.hip through
mstg_frechet_distance and mstg_singular_values; csrc/display_finish.hip through mstg_gamma_u8 and mstg_equalize_luma_u8;
mstg_hip.metrics.frechet_distance / singular_values / calculate_fid, mstg_hip.image.gamma_u8 / equalize_luma_u8 / display_finish, and
the drop-in's process_image) against the numpy restatements of tests/fid_ref.py and tests/display_finish_ref.py.

The Frechet bars come from the arithmetic, none from what the device gives: against the float64 restatement (numpy SVD) every
output within K eps (ssdiff + tr1 + tr2), K = max(n1, n2, d) = the terms accumulated per output; against the reference's sqrtm
formula at most four times the restatement's own distance from that formula on the same draw (with the same floor).  The 8-bit
outputs are compared byte for byte with no pixel excluded.  Every C entry runs with 64 guard bytes behind every output and its inputs
unchanged.  The OpenCV steps of the restatement have not been compared with an OpenCV binary (see its docstring)."""
import functools

import numpy as np
import pytest
import torch

import display_finish_ref as DR
import fid_ref as FR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the cached inputs are read-only


def _guarded(nbytes):
    return torch.full((nbytes + GUARD,), 7, dtype=torch.uint8, device=DEV)


def _take(buf, nbytes, dtype, shape, what):
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[nbytes:] == 7).all(), f"{what} wrote behind its output"
    return out[:nbytes].view(dtype).reshape(shape)


# ---- the Frechet distance ----------------------------------------------------------------------------------------------------------------
PARTS = ("ssdiff", "tr1", "tr2", "nuclear", "fid")


@functools.lru_cache(maxsize=None)
def _draw(n1, n2, d, dtype):
    x1, x2 = FR.draw(n1, n2, d, 7 + n1 + d, F32 if dtype == "float32" else F64)
    x1.setflags(write=False)
    x2.setflags(write=False)
    return x1, x2


def _frechet(x1, x2):
    """mstg_frechet_distance of two numpy feature sets -> (dict of the five outputs, sweeps, converged)"""
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    a, b = _dev(x1), _dev(x2)
    n1, n2, d = a.shape[0], b.shape[0], a.shape[1]
    need = lib.mstg_frechet_workspace_bytes(n1, n2, d)
    assert need == 8 * FR.workspace_doubles(n1, n2, d)
    bo, bi, ws = _guarded(40), _guarded(8), _guarded(need)
    _lib.check(lib.mstg_frechet_distance(_p(a), _p(b), int(x1.dtype == F64), n1, n2, d, _p(bo), _p(bi), _p(ws), need, _stream()),
               "mstg_frechet_distance")
    out = _take(bo, 40, F64, (5,), "frechet_distance (out)")
    info = _take(bi, 8, np.int32, (2,), "frechet_distance (info)")
    _take(ws, need, np.uint8, (need,), "frechet_distance (workspace)")
    assert torch.equal(a, _dev(x1)) and torch.equal(b, _dev(x2)), "mstg_frechet_distance changed an input"
    return dict(zip(PARTS, out.tolist())), int(info[0]), int(info[1])


def _check_parts(got, want, K, what):
    scale = want["ssdiff"] + want["tr1"] + want["tr2"]
    bar = K * FR.EPS * scale
    worst = max(abs(got[k] - want[k]) for k in PARTS)
    print(f"{what}: " + ", ".join(f"{k} {abs(got[k] - want[k]) / (FR.EPS * scale):.1f}" for k in PARTS) + f" (in eps * scale; bar {K})")
    assert worst <= bar, (what, {k: (got[k], want[k]) for k in PARTS}, worst, bar)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", FR.CASES, ids=[str(c) for c in FR.CASES])
def test_frechet_equals_the_float64_restatement(shape, dtype):
    x1, x2 = _draw(*shape, dtype)
    got, sweeps, converged = _frechet(x1, x2)
    print(f"{shape} {dtype}: {sweeps} sweeps")
    assert converged == 1 and 1 <= sweeps <= FR.MAX_SWEEPS
    _check_parts(got, FR.frechet(x1, x2), max(shape), f"{shape} {dtype}")


@pytest.mark.parametrize("shape", FR.CASES, ids=[str(c) for c in FR.CASES])
def test_frechet_against_the_sqrtm_formula(shape):
    """float32 features, as the reference's extractor returns them"""
    x1, x2 = _draw(*shape, "float32")
    got, _, converged = _frechet(x1, x2)
    want, ref = FR.frechet(x1, x2), FR.reference_fid(x1, x2)
    own = abs(want["fid"] - ref)  # the restatement's distance from the formula on this draw
    floor = max(shape) * FR.EPS * (want["ssdiff"] + want["tr1"] + want["tr2"])
    print(f"{shape}: device {got['fid']!r}, restatement {want['fid']!r}, sqrtm formula {ref!r}; |device - formula| "
          f"{abs(got['fid'] - ref):.3g}, |restatement - formula| {own:.3g}, floor {floor:.3g}")
    assert converged == 1 and abs(got["fid"] - ref) <= max(4 * own, floor)


def test_frechet_constant_column_and_identical_sets():
    x1, x2 = (a.copy() for a in _draw(48, 40, 13, "float64"))
    x1[:, 4] = 0.25
    x2[:, 4] = 0.25
    got, _, converged = _frechet(x1, x2)
    assert converged == 1
    _check_parts(got, FR.frechet(x1, x2), 48, "constant column")
    for dtype in ("float32", "float64"):
        y = _draw(24, 24, 64, dtype)[0]
        got, _, converged = _frechet(y, y.copy())
        want = FR.frechet(y, y.copy())
        bar = 64 * FR.EPS * (want["tr1"] + want["tr2"])  # K = max(24, 24, 64) on the absolute scale of the traces
        print(f"identical sets {dtype}: fid {got['fid']!r}, bar {bar:.3g}")
        assert converged == 1 and got["ssdiff"] == 0.0 and got["tr1"] == got["tr2"]
        assert abs(got["fid"]) <= bar and abs(got["tr1"] - want["tr1"]) <= bar and abs(got["nuclear"] - want["nuclear"]) <= bar


def test_frechet_two_runs_are_bit_identical():
    from mstg_hip import metrics
    for shape in ((100, 100, 2048), (33, 64, 16), FR.CASES[-1]):
        a, b = (_dev(x) for x in _draw(*shape, "float32"))
        runs = []
        for _ in range(2):
            p = metrics.frechet_distance(a, b, return_parts=True)
            runs.append(torch.stack([p[k] for k in PARTS]).cpu().numpy().tobytes() + p["info"].cpu().numpy().tobytes())
        assert runs[0] == runs[1], shape


def test_frechet_python_surface():
    import m_test
    from mstg_hip import metrics
    x1, x2 = _draw(33, 64, 16, "float32")
    want = FR.frechet(x1, x2)
    bar = 64 * FR.EPS * (want["ssdiff"] + want["tr1"] + want["tr2"])
    fid = metrics.frechet_distance(_dev(x1), _dev(x2))
    assert fid.is_cuda and fid.dtype == torch.float64 and fid.dim() == 0 and abs(float(fid) - want["fid"]) <= bar
    parts = metrics.frechet_distance(_dev(x1), _dev(x2), return_parts=True)
    assert sorted(parts) == sorted(PARTS + ("info",)) and parts["info"].dtype == torch.int32 and int(parts["info"][1]) == 1
    for f in (m_test.calculate_fid(x1, x2), m_test.calculate_fid(_dev(x1), _dev(x2)), metrics.calculate_fid(x1, x2)):
        assert isinstance(f, float) and f == float(fid)
    with pytest.raises(RuntimeError, match="did not converge"):
        m_test.calculate_fid(np.full((4, 3), np.nan, F32), np.ones((4, 3), F32) * np.arange(4, dtype=F32)[:, None])
    with pytest.raises(RuntimeError, match=f"min\\(n1, n2\\) = {FR.MAX_SAMPLES + 1}"):
        metrics.frechet_distance(torch.zeros(FR.MAX_SAMPLES + 1, 4, device=DEV), torch.zeros(FR.MAX_SAMPLES + 2, 4, device=DEV))
    with pytest.raises(RuntimeError, match="n1 = 1"):
        metrics.frechet_distance(torch.zeros(1, 4, device=DEV), torch.zeros(5, 4, device=DEV))


def test_non_finite_features_end_within_the_sweep_bound():
    x1, x2 = (a.copy() for a in _draw(33, 64, 16, "float32"))
    x1[3, 5] = np.inf
    got, sweeps, _ = _frechet(x1, x2)
    assert sweeps <= FR.MAX_SWEEPS and not np.isfinite(got["fid"])


# ---- the Jacobi alone ------------------------------------------------------------------------------------------------------------------
def _singular_values(M):
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    x = _dev(M)
    m, n = x.shape
    q = min(m, n)
    need = lib.mstg_singular_values_workspace_bytes(m, n)
    assert need == 8 * (m * n + 1)
    bs, bi, ws = _guarded(8 * q), _guarded(8), _guarded(need)
    _lib.check(lib.mstg_singular_values(_p(x), m, n, _p(bs), _p(bi), _p(ws), need, _stream()), "mstg_singular_values")
    sigma = _take(bs, 8 * q, F64, (q,), "singular_values (sigma)")
    info = _take(bi, 8, np.int32, (2,), "singular_values (info)")
    _take(ws, need, np.uint8, (need,), "singular_values (workspace)")
    assert torch.equal(x, _dev(M)), "mstg_singular_values changed its input"
    return sigma, int(info[0]), int(info[1])


# (m, n): one element, one row / column, both orientations, an odd column count, the largest square that lives in LDS, the first
# shapes that live in the workspace, the cap
SVD_SHAPES = [(1, 1), (1, 5), (5, 1), (7, 5), (5, 7), (33, 16), (64, 33), (128, 128), (130, 128), (100, 200), (FR.MAX_SAMPLES, FR.MAX_SAMPLES)]


@pytest.mark.parametrize("shape", SVD_SHAPES, ids=[str(s) for s in SVD_SHAPES])
def test_singular_values_equal_numpy(shape):
    from mstg_hip import metrics
    m, n = shape
    M = np.random.RandomState(100 + m + n).randn(m, n)
    sigma, sweeps, converged = _singular_values(M)
    want = np.linalg.svd(M, compute_uv=False)
    bar = max(m, n) * FR.EPS * want[0]
    print(f"{shape}: {sweeps} sweeps, max |diff| {np.abs(sigma - want).max() / (FR.EPS * want[0]):.1f} eps * sigma_max (bar {max(m, n)})")
    assert converged == 1 and sweeps <= FR.MAX_SWEEPS
    assert np.all(np.diff(sigma) <= 0) and np.abs(sigma - want).max() <= bar
    again = metrics.singular_values(_dev(M))
    assert again.cpu().numpy().tobytes() == sigma.tobytes()  # two runs, the same bits


def test_singular_values_of_a_rank_deficient_product():
    A, B = FR.factors(*_draw(24, 24, 64, "float64"))[:2]
    M = A @ B.T
    sigma, _, converged = _singular_values(M)
    want = np.linalg.svd(M, compute_uv=False)
    assert converged == 1 and np.abs(sigma - want).max() <= 24 * FR.EPS * want[0]


# ---- the display finish ----------------------------------------------------------------------------------------------------------------
def _equalize(x):
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    xin = _dev(x)
    N, H, W = xin.shape[:3]
    need = lib.mstg_equalize_luma_workspace_bytes(N, H, W)
    assert need > 0
    bo, ws = _guarded(N * H * W * 3), _guarded(need)
    _lib.check(lib.mstg_equalize_luma_u8(_p(xin), N, H, W, _p(bo), _p(ws), need, _stream()), "mstg_equalize_luma_u8")
    out = _take(bo, N * H * W * 3, np.uint8, (N, H, W, 3), "equalize_luma_u8 (out)")
    _take(ws, need, np.uint8, (need,), "equalize_luma_u8 (workspace)")
    assert torch.equal(xin, _dev(x)), "mstg_equalize_luma_u8 changed its input"
    return out


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


def _u8_cases():
    rng = np.random.RandomState(11)
    ramp = np.linspace(0, 1, 37 * 53 * 3).reshape(1, 37, 53, 3)
    three = np.stack([rng.randint(0, 256, (40, 72, 3)), rng.randint(100, 140, (40, 72, 3)), (rng.rand(40, 72, 3) ** 4 * 255).astype(int)])
    two = np.where(rng.rand(1, 19, 23, 1) < 0.3, [[[[30, 60, 90]]]], [[[[200, 180, 220]]]])
    return {"1x1": rng.randint(0, 256, (1, 1, 1, 3)), "37x53": (rng.rand(1, 37, 53, 3) * 200 + 55 * ramp).astype(int),
            "three histograms": three, "constant": np.full((2, 9, 13, 3), 77), "constant colour": np.tile([[[[10, 200, 90]]]], (1, 8, 8, 1)),
            "two levels": two, "noise 256x256": rng.randint(0, 256, (1, 256, 256, 3)), "one row": rng.randint(0, 256, (1, 1, 1030, 3)),
            "more than a chunk": rng.randint(20, 90, (1, 67, 131, 3))}


@pytest.mark.parametrize("name", list(_u8_cases()))
def test_equalize_luma_equals_the_restatement(name):
    from mstg_hip import image as dimg
    x = _u8_cases()[name].astype(np.uint8)
    want = DR.equalize_luma_u8(x)
    _same(_equalize(x), want, name)
    _same(dimg.equalize_luma_u8(_dev(x)).cpu().numpy(), want, name + " (python)")
    _same(dimg.equalize_luma_u8(_dev(x[0])).cpu().numpy(), want[0], name + " (python, one image)")
    if name == "constant":
        _same(want, x, "a constant image stays as it is")


def _gamma_inputs(seed, shape):
    """generator-like values with -1, 1, a NaN and values outside [-1, 1] put in"""
    rng = np.random.RandomState(seed)
    y = np.tanh(rng.randn(*shape) * 1.5).astype(F32)
    flat = y.reshape(-1)
    special = np.array([-1.0, 1.0, -1.5, 1.25, 0.0, np.nan, -0.999999, 0.999999], F32)
    flat[:8] = special[:flat[:8].size]
    if flat.size > 8:
        flat[rng.randint(8, flat.size, 16)] = rng.choice([-1.0, 1.0, -2.0, 3.0], 16).astype(F32)
    return y


# seeds checked on the CPU for the precondition below
GAMMA_CASES = [(21, (1, 3, 1, 1), "float32"), (22, (1, 3, 37, 53), "float32"), (23, (3, 3, 40, 72), "float32"), (24, (2, 3, 64, 64), "float16"),
               (25, (1, 3, 128, 128), "float32")]


def _gamma(y):
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    yin = _dev(y)
    N, _, H, W = yin.shape
    bo = _guarded(N * H * W * 3)
    _lib.check(lib.mstg_gamma_u8(_p(yin), int(y.dtype == np.float16), N, H, W, 1.1, _p(bo), _stream()), "mstg_gamma_u8")
    out = _take(bo, N * H * W * 3, np.uint8, (N, H, W, 3), "gamma_u8 (out)")
    assert yin.cpu().numpy().tobytes() == y.tobytes(), "mstg_gamma_u8 changed its input"
    return out


@pytest.mark.parametrize("seed,shape,dtype", GAMMA_CASES, ids=[f"{s[1]} {s[2]}" for s in GAMMA_CASES])
def test_gamma_and_display_finish_equal_the_restatement(seed, shape, dtype):
    from mstg_hip import image as dimg
    y = _gamma_inputs(seed, shape).astype(dtype)
    margin = DR.gamma_margin_ulps(DR.gamma_inputs(y))
    assert margin > 64, f"seed {seed}: a power lies {margin:.1f} double ulps from a float32 midpoint; choose another seed"
    want = DR.gamma_u8(y)
    _same(_gamma(y), want, "gamma_u8")
    _same(dimg.gamma_u8(_dev(y)).cpu().numpy(), want, "gamma_u8 (python)")
    _same(dimg.gamma_u8(_dev(y[0])).cpu().numpy(), want[:1], "gamma_u8 (python, one image)")
    _same(dimg.display_finish(_dev(y)).cpu().numpy(), DR.display_finish(y), "display_finish")


def test_process_image_through_the_drop_in():
    import m_test
    y = _gamma_inputs(22, (1, 3, 37, 53))[0]
    got = m_test.process_image(_dev(y))
    want = DR.process_image(y)
    assert got.dtype == np.float64 and got.shape == (37, 53, 3) and got.tobytes() == want.tobytes()
    assert got.min() >= 0.0 and got.max() <= 1.0
