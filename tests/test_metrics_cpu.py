"""CPU: the image-quality metrics (csrc/metrics.hip, mstg_hip/metrics.py, image_quality_comparison.py) up to the launch.  The
float64 oracle of the GPU tests (tests/metrics_ref.py) is pinned with closed forms, the integer formulation the kernel evaluates
is checked against it in numpy, the two C-ABI entry points validate on the host, ``evaluate_pairs`` groups by shape with the launch
stubbed, and the drop-in matches file names the way the reference does.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as MR
from conftest import ROOT

C1, C2 = 1e-4, 9e-4


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


# ---- the oracle, pinned with closed forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 7), (8, 9), (23, 37)])
def test_oracle_identical_images_are_exactly_one(shape):
    a, _ = MR.pair("noise", *shape, seed=3)
    m = MR.metrics(a, a.copy())
    assert m["ssim"] == 1.0 and m["ssim_channels"] == [1.0, 1.0, 1.0]
    assert m["mse"] == 0.0 and m["psnr"] == float("inf")


@pytest.mark.parametrize("p,q", [(37, 201), (0, 255), (255, 254), (1, 0), (128, 128)])
def test_oracle_constant_images_closed_form(p, q):
    a, b = np.full((9, 12, 3), p, np.uint8), np.full((9, 12, 3), q, np.uint8)
    m = MR.metrics(a, b)
    want = (2.0 * p * q / 255.0 ** 2 + C1) / ((p * p + q * q) / 255.0 ** 2 + C1)  # both variances and the covariance vanish
    assert abs(m["ssim"] - want) <= 1e-12 and all(abs(c - want) <= 1e-12 for c in m["ssim_channels"])
    assert abs(m["mse"] - ((p - q) / 255.0) ** 2) <= 1e-12 * max(m["mse"], 1e-300)


def test_oracle_black_against_white():
    m = MR.metrics(*MR.pair("blackwhite", 10, 8))
    assert abs(m["ssim"] - 1e-4 / 1.0001) <= 1e-15
    assert m["mse"] == 1.0 and m["psnr"] == 0.0


def test_oracle_rejects_images_smaller_than_the_window():
    with pytest.raises(ValueError):
        MR.metrics(np.zeros((6, 20, 3), np.uint8), np.zeros((6, 20, 3), np.uint8))


# ---- the integer formulation of csrc/metrics.hip, in numpy ----------------------------------------------------------------------
def _box7(v):
    c = np.cumsum(np.cumsum(np.pad(v, ((1, 0), (1, 0))), axis=0), axis=1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def integer_ssim(a_u8, b_u8):
    """exact int64 window sums, S scaled by D1 D2 as in the kernel; returns (per-channel means, largest intermediates)"""
    d1, d2 = 12495.0 * 12495.0, 49.0 * 48.0 * 65025.0
    ch, big = [], 0
    for c in range(3):
        x, y = a_u8[..., c].astype(np.int64), b_u8[..., c].astype(np.int64)
        sx, sy, sq, sxy = _box7(x), _box7(y), _box7(x * x + y * y), _box7(x * y)
        mxy, mm = sx * sy, sx * sx + sy * sy
        n2, dd = 2 * (49 * sxy - mxy), 49 * sq - mm
        big = max(big, int(np.abs(2 * mxy).max()), int(mm.max()), int(np.abs(n2).max()), int(dd.max()), int((49 * sq).max()))
        s = ((2 * mxy + C1 * d1) * (n2 + C2 * d2)) / ((mm + C1 * d1) * (dd + C2 * d2))
        ch.append(float(s.mean(dtype=np.float64)))
    return ch, big


@pytest.mark.parametrize("shape", [(7, 7), (8, 9), (23, 37), (70, 130)])
@pytest.mark.parametrize("kind", MR.KINDS)
def test_integer_formulation_matches_the_oracle(kind, shape):
    a, b = MR.pair(kind, *shape, seed=2)
    ch, big = integer_ssim(a, b)
    ref = MR.metrics(a, b)
    assert big < 2 ** 31  # every intermediate the kernel holds in int32
    assert max(abs(u - v) for u, v in zip(ch, ref["ssim_channels"])) <= 1e-13
    if kind == "identical":
        assert ch == [1.0, 1.0, 1.0]


# ---- C ABI: host-side validation, no launch -------------------------------------------------------------------------------------
def test_tile_constants_match_the_header():
    from mstg_hip import metrics
    text = open(os.path.join(ROOT, "include", "mstg_hip.h")).read()
    assert int(re.search(r"#define MSTG_METRICS_TILE_H (\d+)", text).group(1)) == metrics.TILE_H
    assert int(re.search(r"#define MSTG_METRICS_TILE_W (\d+)", text).group(1)) == metrics.TILE_W


def test_workspace_bytes(lib):
    from mstg_hip import metrics
    wb = lib.mstg_image_metrics_workspace_bytes
    assert wb(1, 7, 7) == 32  # one tile: three fp64 channel sums and one int64 sum of squared differences
    th, tw = metrics.TILE_H, metrics.TILE_W
    assert wb(1, th + 6, tw + 6) == 32 and wb(1, th + 7, tw + 6) == 64 and wb(3, th + 7, tw + 7) == 3 * 4 * 32
    for bad in [(0, 16, 16), (-1, 16, 16), (1, 6, 20), (1, 20, 6), (1, 0, 0), (1, 30000, 30000)]:
        assert wb(*bad) == 0, bad


def test_host_side_validation(lib):
    f, err = lib.mstg_image_metrics_u8, lib.mstg_last_error
    p = 4096  # never dereferenced: every call below fails before a launch
    assert f(None, p, 1, 16, 16, p, p, 1 << 20, None) == -1
    assert f(p, None, 1, 16, 16, p, p, 1 << 20, None) == -1
    assert f(p, p, 1, 16, 16, None, p, 1 << 20, None) == -1
    assert f(p, p, 0, 16, 16, p, p, 1 << 20, None) == -1
    for h, w in [(6, 20), (20, 6)]:
        assert f(p, p, 1, h, w, p, p, 1 << 20, None) == -1
        assert b"7x7" in err() and b"window" in err(), err()
    assert f(p, p, 1, 30000, 30000, p, p, 1 << 20, None) == -5  # H * W * 3 >= 2^31
    assert f(p, p, 1, 26758, 26755, p, p, 1 << 40, None) == -5 and 26758 * 26755 * 3 >= 2 ** 31
    need = lib.mstg_image_metrics_workspace_bytes(2, 100, 100)
    assert need > 0
    assert f(p, p, 2, 100, 100, p, p, need - 1, None) == -4
    assert f(p, p, 2, 100, 100, p, None, need, None) == -4


# ---- Python surface up to the launch --------------------------------------------------------------------------------------------
def test_image_metrics_rejects_what_it_cannot_take():
    from mstg_hip import metrics
    a = torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU.*cpu"):
        metrics.image_metrics(a, a)
    with pytest.raises(ValueError, match=r"\(8, 8, 3\).*\(8, 9, 3\)"):
        metrics.calculate_metrics(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 9, 3), np.uint8))
    with pytest.raises(ValueError, match=r"pair 1.*\(8, 8, 3\).*\(9, 8, 3\)"):
        metrics.evaluate_pairs([(a, a), (a, torch.zeros((9, 8, 3), dtype=torch.uint8))])


def test_evaluate_pairs_groups_by_shape(monkeypatch):
    """one launch per image size, results back in the order given, plain means; the launch is stubbed with the oracle"""
    from mstg_hip import metrics
    shapes = [(9, 12), (8, 8), (9, 12), (12, 9), (8, 8), (9, 12)]
    pairs = [MR.pair("noise", h, w, seed=i) for i, (h, w) in enumerate(shapes)]
    calls = []

    def fake_group(imgs_a, imgs_b):
        calls.append([tuple(t.shape) for t in imgs_a])
        assert [tuple(t.shape) for t in imgs_b] == calls[-1]
        rows = [MR.metrics(np.asarray(x), np.asarray(y)) for x, y in zip(imgs_a, imgs_b)]
        return torch.tensor([[r["mse"], r["psnr"], r["ssim"]] for r in rows], dtype=torch.float64)

    monkeypatch.setattr(metrics, "_launch_group", fake_group)
    results, averages = metrics.evaluate_pairs(pairs)
    assert calls == [[(9, 12, 3)] * 3, [(8, 8, 3)] * 2, [(12, 9, 3)]]
    want = [MR.metrics(a, b) for a, b in pairs]
    assert [set(r) for r in results] == [{"mse", "psnr", "ssim"}] * 6
    for r, w in zip(results, want):
        assert all(isinstance(r[k], float) and r[k] == w[k] for k in ("mse", "psnr", "ssim"))
    for k in ("mse", "psnr", "ssim"):
        assert averages[k] == sum(w[k] for w in want) / 6
    assert metrics.evaluate_pairs([]) == ([], None)
    assert len(calls) == 3


def test_drop_in_matches_names_like_the_reference(tmp_path):
    import image_quality_comparison as iqc
    d1, d2 = tmp_path / "a", tmp_path / "b"
    d1.mkdir()
    d2.mkdir()
    for n in ("001.jpg", "sky.png", "cyclegan_tree.jpg", "alone.bmp", "notes.txt", "UP.PNG"):
        (d1 / n).write_bytes(b"")
    for n in ("cyclegan_001.jpg", "sky.png", "tree.jpg", "other.bmp", "UP.PNG", "local_style_UP.PNG"):
        (d2 / n).write_bytes(b"")
    files1, files2 = iqc.list_images(str(d1)), iqc.list_images(str(d2))
    assert sorted(os.path.basename(f) for f in files1) == ["001.jpg", "UP.PNG", "alone.bmp", "cyclegan_tree.jpg", "sky.png"]
    got = {(os.path.basename(x), os.path.basename(y)) for x, y in iqc.match_images(files1, files2)}
    assert {("001.jpg", "cyclegan_001.jpg"), ("sky.png", "sky.png"), ("cyclegan_tree.jpg", "tree.jpg")} <= got
    assert len(got) == 4 and not any(x == "alone.bmp" for x, _ in got)
    assert [y for x, y in got if x == "UP.PNG"][0] in ("UP.PNG", "local_style_UP.PNG")  # the first match in listing order
    # first match wins, in the order of the second list
    assert iqc.match_images(["/x/a.png"], ["/y/zz_a.png", "/y/a.png"]) == [("/x/a.png", "/y/zz_a.png")]
    assert iqc.match_images(["/x/long_a.png"], ["/y/b.png", "/y/a.png"]) == [("/x/long_a.png", "/y/a.png")]
    assert iqc.compare_folders(str(tmp_path / "a"), str(tmp_path)) is None  # nothing matches: nothing is decoded or launched
    with pytest.raises(ValueError):
        iqc.compare_folders(str(d1), str(d2), output_excel="x.xlsx")
    assert iqc.calculate_metrics is not None
