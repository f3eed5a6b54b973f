"""Mixed-size image comparison on the device (csrc/compare.hip; mstg_hip.image.cv_resize_u8, mstg_hip.metrics.pair_metrics,
evaluate_pairs_resized, compare_three_way and the three three-way drop-ins).

``cv_resize_u8`` is held byte for byte to the numpy restatement of the 8-bit cv2.resize (tests/cv_resize_ref.py, pinned by
tests/test_compare_cpu.py; not compared with an OpenCV binary).  A row of ``pair_metrics`` is held BIT FOR BIT to
``image_metrics(a, cv_resize_u8(b))`` -- the fused kernel must be the composition -- and, with the bars of
tests/test_gpu_metrics.py (SSIM 1e-12 absolute, MSE 1e-12 relative, PSNR 1e-10 dB), to the float64 restatement of the metrics on
the restated resize.  The Python surface runs under ``guard_helpers.memory_contract(check_inputs=True)``; the direct C calls have
guard bytes behind every output and workspace."""
import csv
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cv_resize_ref as CV
import metrics_ref as MR
from conftest import ROOT
from guard_helpers import memory_contract

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SSIM_TOL, MSE_RTOL, PSNR_TOL = 1e-12, 1e-12, 1e-10
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _assert_bytes(got, want, what):
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype == np.uint8, (what, g.shape, want.shape)
    bad = np.argwhere(g != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {want.size} bytes differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} for {want[tuple(bad[0])]}"


# ---- cv_resize_u8 against the restatement, byte for byte ------------------------------------------------------------------------------
RESIZES = [((1, 1), (7, 7)), ((2, 3), (9, 8)), ((7, 7), (7, 7)), ((22, 36), (11, 18)), ((23, 37), (40, 64)), ((129, 67), (8, 9)),
           ((64, 64), (63, 65)), ((5, 300), (7, 7))]


@pytest.mark.parametrize("src,dst", RESIZES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in RESIZES])
def test_cv_resize_matches_the_restatement(src, dst):
    from mstg_hip import image as dimg
    img = _noise(*src, seed=src[0] * 1000 + src[1])
    with memory_contract(check_inputs=True) as g:
        out = dimg.cv_resize_u8(_dev(img), (dst[1], dst[0]))
        assert g.outputs >= 1
    _assert_bytes(out, CV.resize(img, (dst[1], dst[0])), f"{src} -> {dst}")


def test_cv_resize_batch_of_three_equals_the_single_calls():
    from mstg_hip import image as dimg
    imgs = np.stack([_noise(23, 37, seed=40 + i) for i in range(3)])
    with memory_contract(check_inputs=True):
        x = _dev(imgs)
        batch = dimg.cv_resize_u8(x, (64, 40))
        singles = [dimg.cv_resize_u8(x[i], (64, 40)) for i in range(3)]
    assert batch.shape == (3, 40, 64, 3) and singles[0].shape == (40, 64, 3)
    for i in range(3):
        assert torch.equal(batch[i], singles[i]), i
        _assert_bytes(batch[i], CV.resize(imgs[i], (64, 40)), f"batch item {i}")
    assert len({batch[i].cpu().numpy().tobytes() for i in range(3)}) == 3


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_cv_resize_unaligned_base_pointers(offset):
    from mstg_hip import image as dimg
    img = _noise(23, 37, seed=50)
    buf = torch.zeros(img.size + 8, dtype=torch.uint8, device=DEV)
    buf[offset:offset + img.size] = _dev(img).reshape(-1)
    view = buf[offset:offset + img.size].view(23, 37, 3)
    assert view.is_contiguous() and view.data_ptr() % 4 == offset
    for size in [(64, 40), (9, 8)]:
        _assert_bytes(dimg.cv_resize_u8(view, size), CV.resize(img, size), f"offset {offset} -> {size}")


def test_cv_resize_c_entry_with_guard_bytes():
    """the C entry directly: nothing is written behind the output, the source is unchanged, an overlapping output is refused"""
    from mstg_hip import _lib, image as dimg
    lib = _lib.load()
    imgs = np.stack([_noise(22, 36, seed=60), _noise(22, 36, seed=61)])
    src = _dev(imgs)
    tv = _dev(dimg._cv_table_host(22, 9, False))
    th = _dev(dimg._cv_table_host(36, 50, True))
    n = 2 * 9 * 50 * 3
    out = torch.full((n + GUARD,), 7, dtype=torch.uint8, device=DEV)
    assert lib.mstg_cv_resize_linear_u8(src.data_ptr(), 2, 22, 36, 9, 50, tv.data_ptr(), th.data_ptr(), out.data_ptr(), None) == 0, lib.mstg_last_error()
    torch.cuda.synchronize()
    assert bool((out[n:] == 7).all()) and torch.equal(src.cpu(), torch.from_numpy(imgs))
    for i in range(2):
        _assert_bytes(out[:n].view(2, 9, 50, 3)[i], CV.resize(imgs[i], (50, 9)), f"C entry item {i}")
    assert lib.mstg_cv_resize_linear_u8(src.data_ptr(), 2, 22, 36, 9, 50, tv.data_ptr(), th.data_ptr(), src.data_ptr() + 100, None) == -1
    assert b"overlaps" in lib.mstg_last_error()


# ---- pair_metrics: every pair of the issue in ONE call ------------------------------------------------------------------------------
def _tile_plus_7():
    from mstg_hip import metrics
    return metrics.TILE_H + 7, metrics.TILE_W + 7


@pytest.fixture(scope="module")
def mixed():
    """the pairs (numpy), computed once: a 7x7 / b 1x1; a at the tile shape / a larger b; a 70x130 / b 35x65; a 40x7 / b 7x40; a pair of
    equal shape; two pairs that share one a.  'ref' = the float64 restatement of the metrics on the restated resize."""
    th, tw = _tile_plus_7()
    shared = MR.image(33, 45, 76)
    pairs = [(MR.image(7, 7, 70), _noise(1, 1, 71)), (MR.image(th, tw, 72), _noise(50, 97, 73)), (MR.image(70, 130, 74), MR.image(35, 65, 75)),
             (MR.image(40, 7, 77), _noise(7, 40, 78)), MR.pair("noise", 23, 37, seed=79), (shared, _noise(20, 60, 80)), (shared, MR.image(66, 90, 81))]
    ref = [MR.metrics(a, b if a.shape == b.shape else CV.resize(b, (a.shape[1], a.shape[0]))) for a, b in pairs]
    return {"pairs": pairs, "ref": ref, "shared": (5, 6)}


def _upload(mixed):
    """device tensors of the pairs; the two pairs that share an a get the SAME tensor"""
    A = [_dev(a) for a, _ in mixed["pairs"]]
    i, j = mixed["shared"]
    A[j] = A[i]
    return A, [_dev(b) for _, b in mixed["pairs"]]


def _rows(m):
    host = {k: v.cpu().tolist() for k, v in m.items()}
    return [{k: host[k][n] for k in host} for n in range(len(host["mse"]))]


def _check(got, ref, what):
    d_ssim = max(abs(got["ssim"] - ref["ssim"]), *[abs(u - v) for u, v in zip(got["ssim_channels"], ref["ssim_channels"])])
    d_mse = abs(got["mse"] - ref["mse"]) / ref["mse"] if ref["mse"] else abs(got["mse"])
    d_psnr = 0.0 if got["psnr"] == ref["psnr"] else abs(got["psnr"] - ref["psnr"])
    print(f"{what}: ssim diff {d_ssim:.2e}  mse rel {d_mse:.2e}  psnr diff {d_psnr:.2e}")
    assert d_ssim <= SSIM_TOL and d_mse <= MSE_RTOL and d_psnr <= PSNR_TOL, (what, got, ref)


def test_pair_metrics_one_call_is_the_composition_bit_for_bit(mixed):
    from mstg_hip import image as dimg, metrics
    with memory_contract(check_inputs=True) as g:
        A, B = _upload(mixed)
        m = metrics.pair_metrics(A, B)  # ONE call, seven pairs, six distinct shapes of a
        assert g.outputs >= 2 and g.uploads >= len(A) + len(B)
        P = len(A)
        assert m["mse"].shape == (P,) and m["ssim_channels"].shape == (P, 3) and m["ssim"].dtype == torch.float64 and m["psnr"].is_cuda
        for i, (a, b) in enumerate(zip(A, B)):
            resized = b if a.shape == b.shape else dimg.cv_resize_u8(b, (a.shape[1], a.shape[0]))
            want = metrics.image_metrics(a, resized)
            for k in m:
                assert torch.equal(m[k][i], want[k][0]), (i, k, m[k][i].tolist(), want[k][0].tolist())
    for i, (got, ref) in enumerate(zip(_rows(m), mixed["ref"])):
        _check(got, ref, f"pair {i} {mixed['pairs'][i][0].shape[:2]} <- {mixed['pairs'][i][1].shape[:2]}")
    assert len({r["ssim"] for r in _rows(m)}) == len(A)  # no row stands in for another


def test_pair_metrics_order_and_count_do_not_change_the_bits(mixed):
    from mstg_hip import metrics
    with memory_contract(check_inputs=True):
        A, B = _upload(mixed)
        m = metrics.pair_metrics(A, B)
        again = metrics.pair_metrics(A, B)
        perm = [4, 6, 0, 2, 5, 1, 3]
        mp = metrics.pair_metrics([A[i] for i in perm], [B[i] for i in perm])
        alone = [metrics.pair_metrics([A[i]], [B[i]]) for i in range(len(A))]
    for k in m:
        assert torch.equal(m[k], again[k]), k
        assert torch.equal(mp[k], m[k][perm]), k
        for i in range(len(A)):
            assert torch.equal(alone[i][k][0], m[k][i]), (i, k)


def _launches(fn):
    from mstg_hip import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.mstg_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        return lib.mstg_prof_count()
    finally:
        lib.mstg_prof_enable(0)


def test_launch_count_is_the_headers_constant(mixed):
    from mstg_hip import _lib, metrics
    text = open(os.path.join(ROOT, "include", "mstg_hip.h")).read()
    want = int(re.search(r"#define MSTG_PAIR_METRICS_LAUNCHES (\d+)", text).group(1))
    A, B = _upload(mixed)
    assert len({tuple(a.shape) for a in A[:6]}) == 6
    assert _launches(lambda: metrics.pair_metrics(A[:1], B[:1])) == want == _lib.PAIR_METRICS_LAUNCHES
    assert _launches(lambda: metrics.pair_metrics(A[:6], B[:6])) == want


def test_pair_metrics_c_entry_with_guard_bytes(mixed):
    """the C entries directly, descriptors built here: nothing is written behind out or the workspace, and the rows are pair_metrics'"""
    from mstg_hip import _lib, image as dimg, metrics
    lib = _lib.load()
    idx = [2, 4, 3]
    A, B = _upload(mixed)
    A, B = [A[i] for i in idx], [B[i] for i in idx]
    want = metrics.pair_metrics(A, B)
    descs = (_lib.PairDesc * 3)()
    parts, off = [], 0
    for d, a, b in zip(descs, A, B):
        d.a, d.b, d.ha, d.wa, d.hb, d.wb = a.data_ptr(), b.data_ptr(), a.shape[0], a.shape[1], b.shape[0], b.shape[1]
        if a.shape != b.shape:
            tv, th = dimg._cv_table_host(b.shape[0], a.shape[0], False), dimg._cv_table_host(b.shape[1], a.shape[1], True)
            d.table_v, d.table_h = off, off + tv.size
            off += tv.size + th.size
            parts += [tv, th]
    ntiles = lib.mstg_pair_metrics_tiles(descs, 3, None, 0)
    tiles = np.zeros((ntiles, 4), np.int32)
    assert lib.mstg_pair_metrics_tiles(descs, 3, tiles.ctypes.data, ntiles) == ntiles > 3
    table = np.concatenate(parts)
    need = lib.mstg_pair_metrics_workspace_bytes(descs, 3)
    assert need == 32 * ntiles
    descs_dev = _dev(np.frombuffer(bytes(descs), dtype=np.uint8).copy().view(np.int64))  # 8-byte aligned
    tiles_dev, table_dev = _dev(tiles), _dev(table)
    out = torch.full((3 * 48 + GUARD,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.full((need + GUARD,), 7, dtype=torch.uint8, device=DEV)
    assert C.sizeof(descs) == descs_dev.numel() * 8
    rc = lib.mstg_pair_metrics_u8(descs, 3, table.ctypes.data, table.size, descs_dev.data_ptr(), tiles_dev.data_ptr(), ntiles, table_dev.data_ptr(),
                                  out.data_ptr(), ws.data_ptr(), need, None)
    assert rc == 0, lib.mstg_last_error()
    torch.cuda.synchronize()
    assert bool((out[3 * 48:] == 7).all()) and bool((ws[need:] == 7).all())
    got = out[:3 * 48].view(torch.float64).view(3, 6)
    assert torch.equal(got[:, 0], want["mse"]) and torch.equal(got[:, 1], want["psnr"]) and torch.equal(got[:, 2], want["ssim"])
    assert torch.equal(got[:, 3:6], want["ssim_channels"])
    assert lib.mstg_pair_metrics_u8(descs, 3, table.ctypes.data, table.size, descs_dev.data_ptr(), tiles_dev.data_ptr(), ntiles, table_dev.data_ptr(),
                                    out.data_ptr(), ws.data_ptr(), need - 1, None) == -4


# ---- evaluate_pairs_resized, compare_three_way ----------------------------------------------------------------------------------------
def test_evaluate_pairs_resized_equals_evaluate_pairs_on_resized_images(mixed):
    from mstg_hip import image as dimg, metrics
    pairs = mixed["pairs"]
    with memory_contract(check_inputs=True):
        given = [(a, _dev(b)) if i % 2 else (_dev(a), b) for i, (a, b) in enumerate(pairs)]  # numpy arrays and tensors mix
        results, averages = metrics.evaluate_pairs_resized(given)
        before = []
        for a, b in pairs:
            tb = _dev(b)
            before.append((a, tb if a.shape == b.shape else dimg.cv_resize_u8(tb, (a.shape[1], a.shape[0]))))
        want, want_avg = metrics.evaluate_pairs(before)
    assert [r["resized"] for r in results] == [True, True, True, True, False, True, True]
    for r, w in zip(results, want):
        assert set(r) == {"mse", "psnr", "ssim", "resized"} and all(isinstance(r[k], float) and r[k] == w[k] for k in w), (r, w)
    assert averages == want_avg


def _direct(a_np, b_np):
    """{'mse', 'psnr', 'ssim'} of the composition cv_resize_u8 + image_metrics, as floats"""
    from mstg_hip import image as dimg, metrics
    a, b = _dev(a_np), _dev(b_np)
    if a.shape != b.shape:
        b = dimg.cv_resize_u8(b, (a.shape[1], a.shape[0]))
    m = metrics.image_metrics(a, b)
    return {k: float(m[k][0]) for k in ("mse", "psnr", "ssim")}


def _label(cy, ls):
    return {"mse_better": "LocalStyle" if ls["mse"] < cy["mse"] else "CycleGAN", "psnr_better": "LocalStyle" if ls["psnr"] > cy["psnr"] else "CycleGAN",
            "ssim_better": "LocalStyle" if ls["ssim"] > cy["ssim"] else "CycleGAN"}


@pytest.fixture(scope="module")
def three_sets():
    """three images: originals, CycleGAN outputs and local-style outputs (RGB, as the PNGs hold them) of different sizes; the last
    set has IDENTICAL outputs, a tie in every metric; in the first the local style is the closer one"""
    o = [MR.image(30, 40, 90), MR.image(24, 50, 91), MR.image(20, 20, 92)]
    near = (o[0].astype(np.int32) + np.random.RandomState(5).randint(-3, 4, size=o[0].shape)).clip(0, 255).astype(np.uint8)
    tie = _noise(33, 17, 97)
    cy = [_noise(60, 80, 93), MR.image(24, 50, 94), tie]
    ls = [near, _noise(12, 25, 96), tie.copy()]
    return o, cy, ls


def _want_rows(three_sets, bgr=False):
    flip = (lambda x: np.ascontiguousarray(x[:, :, ::-1])) if bgr else (lambda x: x)
    o, cy, ls = three_sets
    rows = []
    for a, c, l in zip(o, cy, ls):
        mc, ml = _direct(flip(a), flip(c)), _direct(flip(a), flip(l))
        rows.append((mc, ml, _label(mc, ml)))
    return rows


def test_compare_three_way_numbers_labels_and_one_call(three_sets, monkeypatch):
    from mstg_hip import metrics
    o, cy, ls = three_sets
    want = _want_rows(three_sets)
    calls = []
    real = metrics.pair_metrics
    monkeypatch.setattr(metrics, "pair_metrics", lambda a, b: calls.append(len(a)) or real(a, b))
    with memory_contract(check_inputs=True):
        rows, avg_cy, avg_ls = metrics.compare_three_way(o, [_dev(c) for c in cy], ls)
    assert calls == [6]  # all 2 P comparisons in one call
    for row, (mc, ml, lab) in zip(rows, want):
        assert {k: row["cyclegan"][k] for k in mc} == mc and {k: row["local_style"][k] for k in ml} == ml
        assert row["comparison"] == lab
    assert [r["cyclegan"]["resized"] for r in rows] == [True, False, True] and [r["local_style"]["resized"] for r in rows] == [False, True, True]
    assert rows[0]["comparison"] == {"mse_better": "LocalStyle", "psnr_better": "LocalStyle", "ssim_better": "LocalStyle"}
    assert rows[2]["comparison"] == {"mse_better": "CycleGAN", "psnr_better": "CycleGAN", "ssim_better": "CycleGAN"}  # the tie
    assert rows[2]["cyclegan"]["mse"] == rows[2]["local_style"]["mse"]
    for avg, part in ((avg_cy, [w[0] for w in want]), (avg_ls, [w[1] for w in want])):
        assert avg == {k: sum(p[k] for p in part) / 3 for k in ("mse", "psnr", "ssim")}


def _write_folders(tmp_path, three_sets, names):
    """names: per image (original, cyclegan, local style) file names"""
    from PIL import Image
    folders = [tmp_path / "orig", tmp_path / "cy", tmp_path / "ls"]
    for f in folders:
        f.mkdir()
    for i, trio in enumerate(names):
        for folder, name, imgs in zip(folders, trio, three_sets):
            Image.fromarray(imgs[i]).save(str(folder / name))
    return [str(f) for f in folders]


def _check_csv(path, columns, first, rows):
    with open(path, newline="", encoding="utf-8") as f:
        table = list(csv.reader(f))
    assert tuple(table[0]) == tuple(columns) and len(table) == rows + 2
    assert table[1][0] == first and table[-1][0] in ("AVERAGE", "平均值")
    return table


def test_complete_comparison_and_improved_image_compare_on_folders(tmp_path, three_sets):
    import complete_comparison as cc
    import improved_image_compare as iic
    names = [("img01.png", "cyclegan_img01.png", "local_style_img01.png"), ("img02.png", "img02.png", "img02.png"), ("tie03.png", "tie03.png", "tie03.png")]
    orig, cy, ls = _write_folders(tmp_path, three_sets, names)
    (tmp_path / "orig" / "broken.png").write_bytes(b"not a png")  # matched, unreadable: skipped with a message
    (tmp_path / "cy" / "broken.png").write_bytes(b"not a png")
    (tmp_path / "ls" / "broken.png").write_bytes(b"not a png")
    want = {n[0]: w for n, w in zip(names, _want_rows(three_sets, bgr=True))}  # the files are decoded to B, G, R like cv2.imread
    for mod, fn in ((cc, cc.compare_with_original), (iic, iic.compare_folders_with_original)):
        out_csv = str(tmp_path / f"{mod.__name__}.csv")
        with memory_contract(check_inputs=True):
            res = fn(orig, cy, ls, output=out_csv)
        assert sorted(r["orig_name"] for r in res["results"]) == ["img01.png", "img02.png", "tie03.png"]
        for r in res["results"]:
            mc, ml, lab = want[r["orig_name"]]
            assert {k: r["cyclegan"][k] for k in mc} == mc and {k: r["local_style"][k] for k in ml} == ml and r["comparison"] == lab
            trio = [n for n in names if n[0] == r["orig_name"]][0]
            assert (r["cyclegan"]["name"], r["local_style"]["name"]) == trio[1:]
        assert res["wins"]["mse"] == {"CycleGAN": sum(w[2]["mse_better"] == "CycleGAN" for w in want.values()),
                                      "LocalStyle": sum(w[2]["mse_better"] == "LocalStyle" for w in want.values())}
        assert res["cyclegan_averages"]["ssim"] == sum(r["cyclegan"]["ssim"] for r in res["results"]) / 3
        table = _check_csv(out_csv, cc.COLUMNS, res["results"][0]["orig_name"], 3)
        first = res["results"][0]
        assert float(table[1][1]) == first["cyclegan"]["mse"] and float(table[1][8]) == first["local_style"]["ssim"] and table[1][3] == first["comparison"]["mse_better"]
        with pytest.raises(ValueError, match=r"\.xlsx"):
            fn(orig, cy, ls, output=str(tmp_path / "out.xlsx"))
    assert [r["orig_name"] for r in iic.compare_folders_with_original(orig, cy, ls)["results"]] == ["img01.png", "img02.png", "tie03.png"]  # sorted stems
    assert iic.compare_folders_with_original(orig, cy, ls)["better_count"] == {m: res["wins"][m]["LocalStyle"] for m in ("mse", "psnr", "ssim")}
    mse, psnr, ssim = cc.calculate_metrics(three_sets[0][0], three_sets[1][0])  # the reference's tuple, with the resize
    assert (mse, psnr, ssim) == tuple(_direct(three_sets[0][0], three_sets[1][0])[k] for k in ("mse", "psnr", "ssim"))


def test_compare_image_quality_on_folders(tmp_path, three_sets):
    import compare_image_quality as ciq
    names = [("img01.png",) * 3, ("img02.png",) * 3, ("tie03.png",) * 3]
    orig, cy, ls = _write_folders(tmp_path, three_sets, names)
    want = _want_rows(three_sets, bgr=True)
    out_csv = str(tmp_path / "test_images.csv")
    with memory_contract(check_inputs=True):
        res = ciq.compare_with_test_images(ls, cy, orig, output_file=out_csv)
    by_name = {d["image"]: d for d in res["details"]}
    for (n, _, _), (mc, ml, _) in zip(names, want):
        d = by_name[n]
        assert (d["cyclegan_mse"], d["cyclegan_psnr"], d["cyclegan_ssim"]) == (mc["mse"], mc["psnr"], mc["ssim"])
        assert (d["local_style_mse"], d["local_style_psnr"], d["local_style_ssim"]) == (ml["mse"], ml["psnr"], ml["ssim"])
    assert res["avg_local_ssim"] == sum(d["local_style_ssim"] for d in res["details"]) / 3
    assert res["avg_cyclegan_mse"] == sum(d["cyclegan_mse"] for d in res["details"]) / 3
    table = _check_csv(out_csv, ciq.TEST_COLUMNS, res["details"][0]["image"], 3)
    assert float(table[1][1]) == res["details"][0]["local_style_ssim"] and float(table[-1][6]) == res["avg_cyclegan_mse"]
    # one base folder against two: the originals against the CycleGAN folder (mixed sizes) and against a copy of themselves
    from PIL import Image
    same = tmp_path / "same"
    same.mkdir()
    for n, img in zip(names, three_sets[0]):
        Image.fromarray(img).save(str(same / n[0]))
    folders_csv = str(tmp_path / "folders.csv")
    with memory_contract(check_inputs=True):
        got = ciq.compare_image_folders(orig, [orig, cy, str(same)], output_file=folders_csv)
    assert [r["folder"] for r in got] == ["cy", "same"] and [r["images_count"] for r in got] == [3, 3]
    assert [d["image"] for d in got[0]["details"]] == ["img01.png", "img02.png", "tie03.png"]  # sorted
    for d, (mc, _, _) in zip(got[0]["details"], want):
        assert (d["mse"], d["psnr"], d["ssim"]) == (mc["mse"], mc["psnr"], mc["ssim"])
    assert got[0]["avg_psnr"] == sum(d["psnr"] for d in got[0]["details"]) / 3
    assert got[1]["details"] == [] and got[1]["avg_ssim"] == 0.0  # identical images are skipped, as in the reference
    with open(folders_csv, newline="", encoding="utf-8") as f:
        table = list(csv.reader(f))
    assert tuple(table[0]) == ciq.FOLDER_COLUMNS and table[1][0] == "cy" and float(table[1][2]) == got[0]["avg_ssim"]
    # the three metric functions: uint8 arrays and the reference's float images give the same numbers
    a, b = three_sets[0][1], three_sets[1][1]
    d = _direct(a, b)
    assert (ciq.calculate_mse(a, b), ciq.calculate_psnr(a, b), ciq.calculate_ssim(a, b)) == (d["mse"], d["psnr"], d["ssim"])
    fa, fb = a.astype(float) / 255.0, b.astype(float) / 255.0
    assert (ciq.calculate_mse(fa, fb), ciq.calculate_psnr(fa, fb), ciq.calculate_ssim(fa, fb)) == (d["mse"], d["psnr"], d["ssim"])
    with pytest.raises(ValueError, match="off the byte grid"):
        ciq.calculate_ssim(fa + 1e-5, fb)
    with pytest.raises(ValueError, match=r"\.xlsx"):
        ciq.compare_with_test_images(ls, cy, orig, output_file=str(tmp_path / "r.xlsx"))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_raises_and_names_its_value():
    from mstg_hip import image as dimg, metrics
    a = torch.zeros((20, 20, 3), dtype=torch.uint8, device=DEV)
    b = torch.zeros((9, 11, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r"pair 1: an extent is below 1: a is 20 x 20, b is 0 x 11"):
        metrics.pair_metrics([a, a], [b, b[:0]])
    with pytest.raises(RuntimeError, match=r"pair 0: an extent is below 1: a is 20 x 0"):
        metrics.pair_metrics([a[:, :0]], [b])
    with pytest.raises(RuntimeError, match=r"pair 2: image a 6 x 20 is smaller than the 7x7 SSIM window"):
        metrics.pair_metrics([a, a, a[:6]], [b, b, b])
    with pytest.raises(RuntimeError, match=r"pair 0: image a 20 x 6 is smaller than the 7x7"):
        metrics.pair_metrics([a[:, :6]], [b])
    with pytest.raises(RuntimeError, match=r"images_b\[1\] must be uint8.*float32"):
        metrics.pair_metrics([a, a], [b, b.float()])
    with pytest.raises(RuntimeError, match=r"images_a\[0\] must be \(H, W, 3\)"):
        metrics.pair_metrics([a[None]], [b])
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.pair_metrics([a.cpu()], [b])
    with pytest.raises(RuntimeError, match=r"20 x 20 to 0 x 5"):
        dimg.cv_resize_u8(a, (5, 0))
    with pytest.raises(RuntimeError, match="uint8"):
        dimg.cv_resize_u8(a.float(), (5, 5))
    # sizes past the kernels' 31-bit offsets and past one launch: memory that is allocated and never touched
    big = torch.empty((26758, 26755, 3), dtype=torch.uint8, device=DEV)
    value = 26758 * 26755 * 3
    assert value >= 2 ** 31
    with pytest.raises(RuntimeError, match=rf"pair 1: H \* W \* 3 = {value} of image b does not fit 31 bits"):
        metrics.pair_metrics([a, a], [b, big])
    with pytest.raises(RuntimeError, match=rf"pair 0: H \* W \* 3 = {value} of image a does not fit 31 bits"):
        metrics.pair_metrics([big], [b])
    with pytest.raises(RuntimeError, match=rf"{value}.*does not fit 31 bits"):
        dimg.cv_resize_u8(big, (5, 5))
    del big
    wide = torch.empty((26000, 26000, 3), dtype=torch.uint8, device=DEV)  # 407 x 1625 tiles each
    count = (1 << 24) // (407 * 1625) + 1
    with pytest.raises(RuntimeError, match=rf"pair {count - 1}: the total tile count reaches {407 * 1625 * count}"):
        metrics.pair_metrics([wide] * count, [b] * count)
