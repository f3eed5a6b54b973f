"""Device image-quality metrics (csrc/metrics.hip, mstg_hip/metrics.py) against the float64 CPU restatement of scikit-image's
evaluation (tests/metrics_ref.py, pinned by tests/test_metrics_cpu.py).

Bars: the integer formulation and the float64 restatement agree to a few 1e-15 on mean SSIM (each S carries a few ulp; the
restatement's cancellation error is ~1e-16 absolute against C2 = 9e-4), so SSIM and each channel's SSIM are held to 1e-12
absolute, MSE to 1e-12 relative and PSNR to 1e-10 dB -- three orders above fp64 rounding.  Identical inputs, repeated calls and
batch-versus-single are exact."""
import numpy as np
import pytest
import torch

import metrics_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SSIM_TOL, MSE_RTOL, PSNR_TOL = 1e-12, 1e-12, 1e-10


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _check(got, ref, what):
    """got: row n of image_metrics as Python floats {'mse', 'psnr', 'ssim', 'ssim_channels'}"""
    d_ssim = max(abs(got["ssim"] - ref["ssim"]), *[abs(u - v) for u, v in zip(got["ssim_channels"], ref["ssim_channels"])])
    d_mse = abs(got["mse"] - ref["mse"]) / ref["mse"] if ref["mse"] else abs(got["mse"])
    d_psnr = 0.0 if got["psnr"] == ref["psnr"] else abs(got["psnr"] - ref["psnr"])  # inf == inf
    print(f"{what}: ssim diff {d_ssim:.2e}  mse rel {d_mse:.2e}  psnr diff {d_psnr:.2e}")
    assert d_ssim <= SSIM_TOL and d_mse <= MSE_RTOL and d_psnr <= PSNR_TOL, (what, got, ref)


def _rows(m):
    host = {k: v.cpu().tolist() for k, v in m.items()}
    return [{k: host[k][n] for k in host} for n in range(len(host["mse"]))]


def _tile_shape():
    from mstg_hip import metrics
    return (metrics.TILE_H + 1 + 6, metrics.TILE_W + 1 + 6)  # one full tile plus one row and one column of windows


SHAPES = [(7, 7), (7, 40), (40, 7), (8, 9), (23, 37), (70, 130), (129, 67), "tile"]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_shapes_and_pair_kinds_against_the_oracle(shape):
    """every pair kind at the smallest and the awkward shapes, all kinds of one shape in one batch"""
    from mstg_hip import metrics
    h, w = _tile_shape() if shape == "tile" else shape
    pairs = [MR.pair(kind, h, w, seed=i) for i, kind in enumerate(MR.KINDS)]
    m = metrics.image_metrics(_dev(np.stack([p[0] for p in pairs])), _dev(np.stack([p[1] for p in pairs])))
    assert m["mse"].dtype == torch.float64 and m["mse"].is_cuda and m["ssim_channels"].shape == (len(pairs), 3)
    for kind, (a, b), got in zip(MR.KINDS, pairs, _rows(m)):
        _check(got, MR.metrics(a, b), f"{kind} {h}x{w}")
        if kind == "identical":
            assert got["ssim"] == 1.0 and got["ssim_channels"] == [1.0, 1.0, 1.0] and got["mse"] == 0.0 and got["psnr"] == float("inf")
        if kind == "blackwhite":
            assert got["mse"] == 1.0 and got["psnr"] == 0.0
        if kind == "constant":
            # closed form: both variances and the covariance vanish (the oracle carries a ~1e-14 residue of uxx - ux ux here).
            # Bar: S <= 1 goes through ~10 roundings per window and ~25 additions of equal values (4 rows, 6 butterfly steps, 4
            # waves, tiles, the channel mean), the closed form through ~8: below 45 x 1.1e-16 = 5e-15; held to 1e-14.
            p, q = float(a[0, 0, 0]), float(b[0, 0, 0])
            want = (2.0 * p * q / 255.0 ** 2 + 1e-4) / ((p * p + q * q) / 255.0 ** 2 + 1e-4)
            d = max(abs(c - want) for c in got["ssim_channels"] + [got["ssim"]])
            print(f"constant {h}x{w}: closed-form diff {d:.2e}")
            assert d <= 1e-14


def test_batch_of_three_different_pairs_and_bit_identity():
    """per-image indexing and workspace stride; a repeated call and each pair run alone give the same bits"""
    from mstg_hip import metrics
    pairs = [MR.pair("noise", 70, 130, seed=1), MR.pair("binary", 70, 130, seed=2), MR.pair("noise", 70, 130, seed=3)]
    a, b = _dev(np.stack([p[0] for p in pairs])), _dev(np.stack([p[1] for p in pairs]))
    m1, m2 = metrics.image_metrics(a, b), metrics.image_metrics(a, b)
    for k in m1:
        assert torch.equal(m1[k], m2[k]), k
    rows = _rows(m1)
    assert len({r["ssim"] for r in rows}) == 3
    for i, ((x, y), got) in enumerate(zip(pairs, rows)):
        _check(got, MR.metrics(x, y), f"batch item {i}")
        single = metrics.image_metrics(a[i], b[i])  # the (H, W, 3) call form
        assert single["ssim"].shape == (1,) and single["ssim_channels"].shape == (1, 3)
        for k in m1:
            assert torch.equal(single[k][0], m1[k][i]), (i, k)


def test_large_image_once():
    from mstg_hip import metrics
    a, b = MR.pair("noise", 1024, 1024, seed=5)
    m = metrics.image_metrics(_dev(a), _dev(b))
    _check(_rows(m)[0], MR.metrics(a, b), "noise 1024x1024")


def test_non_contiguous_input_and_numpy_calculate_metrics():
    from mstg_hip import metrics
    a, b = MR.pair("noise", 60, 90, seed=7)
    big_a, big_b = _dev(a), _dev(b)
    va, vb = big_a[3:50:2, 5:81], big_b[3:50:2, 5:81]  # rows strided, columns offset
    assert not va.is_contiguous()
    ref = MR.metrics(np.ascontiguousarray(a[3:50:2, 5:81]), np.ascontiguousarray(b[3:50:2, 5:81]))
    _check(_rows(metrics.image_metrics(va, vb))[0], ref, "sliced")
    got = metrics.calculate_metrics(a, b)  # numpy in, Python floats out
    assert set(got) == {"mse", "psnr", "ssim"} and all(isinstance(v, float) for v in got.values())
    ref = MR.metrics(a, b)
    _check({**got, "ssim_channels": ref["ssim_channels"]}, ref, "calculate_metrics(numpy)")
    got_t = metrics.calculate_metrics(big_a, big_b)  # cuda tensors in
    assert got_t == got


def test_unaligned_base_pointers():
    """images that start at every byte offset of a dword: the staging loads whole dwords where a row allows it"""
    from mstg_hip import metrics
    a, b = MR.pair("noise", 30, 75, seed=9)
    ref = MR.metrics(a, b)
    n = a.size
    for off_a, off_b in [(1, 2), (3, 0), (2, 3)]:
        buf_a = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
        buf_b = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
        buf_a[off_a:off_a + n] = _dev(a).reshape(-1)
        buf_b[off_b:off_b + n] = _dev(b).reshape(-1)
        va, vb = buf_a[off_a:off_a + n].view(30, 75, 3), buf_b[off_b:off_b + n].view(30, 75, 3)
        assert va.is_contiguous() and va.data_ptr() % 4 == off_a
        _check(_rows(metrics.image_metrics(va, vb))[0], ref, f"offsets {off_a}, {off_b}")


def test_bad_input_raises():
    from mstg_hip import metrics
    a = torch.zeros((20, 20, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r"shapes differ \(20, 20, 3\) vs \(20, 21, 3\)"):
        metrics.image_metrics(a, torch.zeros((20, 21, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="7x7"):
        metrics.image_metrics(a[:6], a[:6])  # 6 x 20: smaller than the window
    with pytest.raises(RuntimeError, match="uint8.*float32"):
        metrics.image_metrics(a.float(), a.float())
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.image_metrics(a.cpu(), a.cpu())
    with pytest.raises(ValueError, match=r"\(20, 20, 3\).*\(6, 20, 3\)"):
        metrics.calculate_metrics(a, a[:6])


def test_evaluate_pairs_on_the_device():
    from mstg_hip import metrics
    shapes = [(30, 40), (16, 16), (30, 40)]
    pairs = [MR.pair("noise", h, w, seed=20 + i) for i, (h, w) in enumerate(shapes)]
    results, averages = metrics.evaluate_pairs([(_dev(a), b) for a, b in pairs])  # tensors and arrays mix
    want = [MR.metrics(a, b) for a, b in pairs]
    for i, (r, w) in enumerate(zip(results, want)):
        _check({**r, "ssim_channels": w["ssim_channels"]}, w, f"pair {i}")
    for k in ("mse", "psnr", "ssim"):
        assert averages[k] == sum(r[k] for r in results) / 3


def test_process_cyclegan_output_is_scored_on_the_device(monkeypatch):
    """end to end: the generator's uint8 output goes from process_cyclegan into the metric kernels as the cuda tensor it is"""
    import warnings

    import enhanced_generator as eg
    from mstg_hip import image as dimg, metrics
    from oracle import restatement as R
    model = eg.EnhancedGenerator(16, 0)
    model.load_state_dict(R.make_state_dict(R.generator_spec(16), 31))
    model.to(DEV).eval()
    src = _dev(MR.image(96, 128, 4))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = dimg.process_cyclegan(model, src)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == src.shape
    seen = []
    real = metrics._launch

    def spy(a, b):
        seen.append((a.is_cuda, a.data_ptr(), b.is_cuda, b.data_ptr()))
        return real(a, b)

    monkeypatch.setattr(metrics, "_launch", spy)
    m = metrics.image_metrics(src, out)
    assert seen == [(True, src.data_ptr(), True, out.data_ptr())]  # the very tensors: no copy through the host
    _check(_rows(m)[0], MR.metrics(src.cpu().numpy(), out.cpu().numpy()), "process_cyclegan 96x128")
