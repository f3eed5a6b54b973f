"""Image-quality metrics of the reference's evaluation scripts on the device (csrc/metrics.hip): MSE, PSNR and SSIM of uint8 HWC
image pairs as compare_image_quality.py:14-33, image_quality_comparison.py:11-34, complete_comparison.py:13-32 and
improved_image_compare.py:8-27 compute them (images / 255, ``np.mean((a - b) ** 2)``, skimage ``peak_signal_noise_ratio`` and
``structural_similarity(channel_axis=2)`` with ``data_range=1.0``).  The images stay on the GPU, e.g. straight from
``image.process_cyclegan``; only ``calculate_metrics`` and ``evaluate_pairs`` bring numbers to the host, once per call.
Pairs of DIFFERENT shapes, which those scripts resize with ``cv2.resize`` before they measure, go through ``pair_metrics``,
``evaluate_pairs_resized`` and ``compare_three_way`` (csrc/compare.hip): the resize is fused into the metric kernel.
Below them the Frechet distance of two feature sets as the reference's m_test.py:37-50 computes it (csrc/frechet.hip):
``frechet_distance``, its Jacobi SVD alone (``singular_values``) and ``calculate_fid`` with the reference's signature.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .ops import _p, _stream

# windows per workgroup tile of csrc/metrics.hip (MSTG_METRICS_TILE_H / _W of include/mstg_hip.h)
TILE_H, TILE_W = 16, 64


def _req_pair(a: torch.Tensor, b: torch.Tensor):
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"mstg_hip metrics: {name} must be a torch tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"mstg_hip metrics: {name} must live on the GPU, got a {t.device} tensor")
        if t.dtype != torch.uint8:
            raise RuntimeError(f"mstg_hip metrics: {name} must be uint8, got {t.dtype}")
        if t.dim() not in (3, 4) or t.shape[-1] != 3:
            raise RuntimeError(f"mstg_hip metrics: {name} must be (H, W, 3) or (N, H, W, 3), got {tuple(t.shape)}")
    if a.shape != b.shape:
        raise RuntimeError(f"mstg_hip metrics: shapes differ {tuple(a.shape)} vs {tuple(b.shape)}")
    if a.device != b.device:
        raise RuntimeError(f"mstg_hip metrics: devices differ {a.device} vs {b.device}")
    if a.dim() == 3:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    return a.contiguous(), b.contiguous()


def _launch(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(N, H, W, 3) uint8 cuda, contiguous, equal shapes -> (N, 6) float64 cuda {mse, psnr, ssim, ssim_c0, ssim_c1, ssim_c2}"""
    lib = _lib.load()
    N, H, W = a.shape[:3]
    out = torch.empty((N, 6), dtype=torch.float64, device=a.device)
    nbytes = lib.mstg_image_metrics_workspace_bytes(N, H, W)  # 0 for a bad shape: the call below names what is wrong
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=a.device)
    _lib.check(lib.mstg_image_metrics_u8(_p(a), _p(b), N, H, W, _p(out), _p(ws), ws.numel() * 8, _stream()), "mstg_image_metrics_u8")
    return out


def _launch_group(imgs_a, imgs_b) -> torch.Tensor:
    """One batched launch for lists of (H, W, 3) images of one shape -> (len, 3) float64 cuda {mse, psnr, ssim}"""
    a, b = _req_pair(torch.stack([_as_cuda_u8(t, "a") for t in imgs_a]), torch.stack([_as_cuda_u8(t, "b") for t in imgs_b]))
    return _launch(a, b)[:, :3]


def image_metrics(a: torch.Tensor, b: torch.Tensor) -> dict:
    """MSE, PSNR and SSIM of uint8 cuda images ``a`` against ``b``, (H, W, 3) or (N, H, W, 3) of equal shape: float64 cuda tensors
    ``mse``, ``psnr``, ``ssim`` of shape (N,) and ``ssim_channels`` (N, 3).  No host synchronisation."""
    a, b = _req_pair(a, b)
    out = _launch(a, b)
    return {"mse": out[:, 0], "psnr": out[:, 1], "ssim": out[:, 2], "ssim_channels": out[:, 3:6]}


def _as_cuda_u8(img, name: str) -> torch.Tensor:
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8:
            raise RuntimeError(f"mstg_hip metrics: {name} must be uint8, got {img.dtype}")
        return torch.from_numpy(np.ascontiguousarray(img)).cuda()
    return img


def calculate_metrics(img1, img2) -> dict:
    """``calculate_metrics`` of image_quality_comparison.py:11-34: {'mse', 'psnr', 'ssim'} as Python floats for two uint8
    (H, W, 3) images, numpy arrays or cuda tensors.  Images of different shapes raise ValueError: the reference resizes the second
    one with cv2.resize there; this function keeps refusing -- ``evaluate_pairs_resized`` / ``pair_metrics`` resize as the reference
    does (``image.cv_resize_u8``), ``image.resize_u8`` is Pillow's resampling."""
    if tuple(img1.shape) != tuple(img2.shape):
        raise ValueError(f"mstg_hip metrics: image shapes differ, {tuple(img1.shape)} vs {tuple(img2.shape)}; "
                         "resize one with mstg_hip.image.resize_u8 first")
    a, b = _req_pair(_as_cuda_u8(img1, "img1"), _as_cuda_u8(img2, "img2"))
    if a.shape[0] != 1:
        raise ValueError(f"mstg_hip metrics: calculate_metrics takes one (H, W, 3) pair, got {tuple(img1.shape)}")
    mse, psnr, ssim = _launch(a, b)[0, :3].tolist()
    return {"mse": mse, "psnr": psnr, "ssim": ssim}


def evaluate_pairs(pairs):
    """Metrics of a list of (a_u8, b_u8) image pairs ((H, W, 3) uint8, numpy arrays or cuda tensors): pairs of equal (H, W) go
    through one batched launch, and all results come to the host in ONE copy at the end.  Returns (results, averages): a dict
    {'mse', 'psnr', 'ssim'} of Python floats per pair in the order given, and the plain arithmetic means over the pairs
    {'mse', 'psnr', 'ssim'} that the reference's folder comparison prints (None for an empty list).  A pair of different shapes
    raises ValueError; ``evaluate_pairs_resized`` takes such pairs."""
    groups = {}
    for i, (a, b) in enumerate(pairs):
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"mstg_hip metrics: pair {i}: image shapes differ, {tuple(a.shape)} vs {tuple(b.shape)}; "
                             "resize one with mstg_hip.image.resize_u8 first")
        if len(a.shape) != 3:
            raise ValueError(f"mstg_hip metrics: pair {i}: expected (H, W, 3) images, got {tuple(a.shape)}")
        groups.setdefault(tuple(a.shape[:2]), []).append(i)
    if not groups:
        return [], None
    order, outs = [], []
    for idx in groups.values():
        outs.append(_launch_group([pairs[i][0] for i in idx], [pairs[i][1] for i in idx]))
        order += idx
    host = torch.cat(outs).cpu().tolist()  # the one device-to-host copy
    results = [None] * len(order)
    for i, (mse, psnr, ssim) in zip(order, host):
        results[i] = {"mse": mse, "psnr": psnr, "ssim": ssim}
    n = len(results)
    averages = {k: sum(r[k] for r in results) / n for k in ("mse", "psnr", "ssim")}
    return results, averages


# ---- mixed-size comparison: the reference's cv2.resize fused into the metrics (csrc/compare.hip) -----------------------------------
_PAIR = np.dtype([("a", "<u8"), ("b", "<u8")] + [(n, "<i4") for n in ("ha", "wa", "hb", "wb", "tile0", "ntiles")] +
                 [("table_v", "<i8"), ("table_h", "<i8")], align=True)
assert _PAIR.itemsize == C.sizeof(_lib.PairDesc)


def _req_image(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"mstg_hip metrics: {name} must be a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"mstg_hip metrics: {name} must live on the GPU, got a {t.device} tensor")
    if t.dtype != torch.uint8:
        raise RuntimeError(f"mstg_hip metrics: {name} must be uint8, got {t.dtype}")
    if t.dim() != 3 or t.shape[-1] != 3:
        raise RuntimeError(f"mstg_hip metrics: {name} must be (H, W, 3), got {tuple(t.shape)}")
    return t.contiguous()


def _pair_launch(images_a, images_b) -> torch.Tensor:
    """-> (P, 6) float64 cuda {mse, psnr, ssim, ssim_c0, ssim_c1, ssim_c2}: descriptors, tile list and coefficient tables go to the
    device in ONE copy from one pinned buffer, then the two launches of mstg_pair_metrics_u8"""
    from . import image
    if len(images_a) != len(images_b):
        raise ValueError(f"mstg_hip metrics: {len(images_a)} images against {len(images_b)}")
    if not images_a:
        raise ValueError("mstg_hip metrics: pair_metrics needs at least one pair")
    a = [_req_image(t, f"images_a[{i}]") for i, t in enumerate(images_a)]
    b = [_req_image(t, f"images_b[{i}]") for i, t in enumerate(images_b)]
    dev = a[0].device
    if any(t.device != dev for t in a + b):
        raise RuntimeError("mstg_hip metrics: the images of one pair_metrics call must live on one device")
    lib, P = _lib.load(), len(a)
    descs = np.zeros(P, dtype=_PAIR)
    for i, (x, y) in enumerate(zip(a, b)):
        descs[i] = (x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], y.shape[0], y.shape[1], 0, 0, 0, 0)
    ntiles = lib.mstg_pair_metrics_tiles(descs.ctypes.data, P, None, 0)  # refuses a bad shape by pair index, before any table is built
    if ntiles <= 0:
        _lib.check(ntiles or -1, "mstg_pair_metrics_tiles")
    parts, index, table_len = [], {}, 0
    for i, (x, y) in enumerate(zip(a, b)):
        if x.shape == y.shape:
            continue
        for field, key in (("table_v", (int(y.shape[0]), int(x.shape[0]), False)), ("table_h", (int(y.shape[1]), int(x.shape[1]), True))):
            if key not in index:
                t = image._cv_table_host(*key)
                index[key] = table_len
                parts.append(t)
                table_len += t.size
            descs[field][i] = index[key]
    table = np.concatenate(parts) if parts else np.zeros(4, dtype=np.int32)
    off_tiles = (descs.nbytes + 15) & ~15
    off_table = off_tiles + 16 * ntiles
    host = torch.empty(off_table + ((table.nbytes + 15) & ~15), dtype=torch.uint8, pin_memory=True)
    hb = host.numpy()
    hp = hb.ctypes.data
    hb[:descs.nbytes] = descs.view(np.uint8)
    hb[off_table:off_table + table.nbytes] = table.view(np.uint8)
    got = lib.mstg_pair_metrics_tiles(hp, P, hp + off_tiles, ntiles)
    if got != ntiles:
        _lib.check(got if got < 0 else -1, "mstg_pair_metrics_tiles")
    devbuf = host.to(dev, non_blocking=True)
    dp = devbuf.data_ptr()
    out = torch.empty((P, 6), dtype=torch.float64, device=dev)
    nbytes = lib.mstg_pair_metrics_workspace_bytes(hp, P)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
    _lib.check(lib.mstg_pair_metrics_u8(hp, P, hp + off_table, int(table.size), dp, dp + off_tiles, ntiles, dp + off_table, _p(out), _p(ws),
                                        ws.numel() * 8, _stream()), "mstg_pair_metrics_u8")
    return out


def pair_metrics(images_a, images_b) -> dict:
    """MSE, PSNR and SSIM of ``images_a[i]`` against ``images_b[i]`` for two equal-length sequences of (H, W, 3) uint8 cuda tensors of
    ANY sizes, in one call: where the shapes of a pair differ, ``images_b[i]`` is resized to ``images_a[i]``'s shape as the
    reference's ``cv2.resize(img, (W, H))`` does (``image.cv_resize_u8``; this build's restatement, not compared with an OpenCV
    binary) while the kernel stages it -- the resized image is never written.  Two launches whatever the number of pairs and
    shapes.  Returns float64 cuda tensors ``mse``, ``psnr``, ``ssim`` (P,) and ``ssim_channels`` (P, 3); row i holds the bits of
    ``image_metrics(images_a[i], cv_resize_u8(images_b[i], ...))``, whatever else is in the call.  The same tensor may appear in
    several pairs.  No host synchronisation."""
    out = _pair_launch(list(images_a), list(images_b))
    return {"mse": out[:, 0], "psnr": out[:, 1], "ssim": out[:, 2], "ssim_channels": out[:, 3:6]}


def _stage_pairs(pairs):
    """[(a, b)] of numpy arrays or cuda tensors -> (list of a, list of b, resized flags) on the device"""
    A, B, resized = [], [], []
    for i, (a, b) in enumerate(pairs):
        if len(a.shape) != 3 or len(b.shape) != 3:
            raise ValueError(f"mstg_hip metrics: pair {i}: expected (H, W, 3) images, got {tuple(a.shape)} and {tuple(b.shape)}")
        A.append(_as_cuda_u8(a, "a"))
        B.append(_as_cuda_u8(b, "b"))
        resized.append(tuple(a.shape) != tuple(b.shape))
    return A, B, resized


def evaluate_pairs_resized(pairs):
    """``evaluate_pairs`` for pairs whose shapes may differ, as the reference's folder comparisons evaluate them: the second image
    of a pair is resized to the first one's shape with the reference's ``cv2.resize`` (see ``pair_metrics``).  ALL pairs go through
    one ``pair_metrics`` call and the results come to the host in ONE copy.  Returns (results, averages): per pair a dict {'mse',
    'psnr', 'ssim'} of Python floats and ``resized`` (bool), in the order given, and the plain means (None for an empty list)."""
    A, B, resized = _stage_pairs(pairs)
    if not A:
        return [], None
    m = pair_metrics(A, B)
    host = torch.stack([m["mse"], m["psnr"], m["ssim"]], dim=1).cpu().tolist()  # the one device-to-host copy
    results = [{"mse": mse, "psnr": psnr, "ssim": ssim, "resized": r} for (mse, psnr, ssim), r in zip(host, resized)]
    n = len(results)
    return results, {k: sum(r[k] for r in results) / n for k in ("mse", "psnr", "ssim")}


def better_labels(cyclegan: dict, local_style: dict) -> dict:
    """the reference's "which is better" (complete_comparison.py:139-141): lower MSE, higher PSNR, higher SSIM win, and a tie goes
    to "CycleGAN", as its ``<`` / ``>`` decide"""
    return {"mse_better": "LocalStyle" if local_style["mse"] < cyclegan["mse"] else "CycleGAN",
            "psnr_better": "LocalStyle" if local_style["psnr"] > cyclegan["psnr"] else "CycleGAN",
            "ssim_better": "LocalStyle" if local_style["ssim"] > cyclegan["ssim"] else "CycleGAN"}


def compare_three_way(originals, cyclegan, local_style):
    """The three-way comparison of compare_image_quality.py:61-215, complete_comparison.py:98-158 and
    improved_image_compare.py:119-148: every original against its CycleGAN output and against its local-style output (each resized
    to the original's shape where it differs).  Three equal-length sequences of (H, W, 3) uint8 images, numpy arrays or cuda
    tensors; all 2 P comparisons go through ONE ``pair_metrics`` call (each original appears twice) and one copy to the host.
    Returns (rows, cyclegan_averages, local_style_averages): per image {'cyclegan': {'mse', 'psnr', 'ssim', 'resized'},
    'local_style': {...}, 'comparison': ``better_labels``}; the averages are plain means (all None for empty input)."""
    if not (len(originals) == len(cyclegan) == len(local_style)):
        raise ValueError(f"mstg_hip metrics: {len(originals)} originals, {len(cyclegan)} CycleGAN and {len(local_style)} local-style images")
    P = len(originals)
    if P == 0:
        return [], None, None
    orig = [_as_cuda_u8(o, "original") for o in originals]  # uploaded once, used twice
    results, _ = evaluate_pairs_resized(list(zip(orig, cyclegan)) + list(zip(orig, local_style)))
    rows = [{"cyclegan": results[i], "local_style": results[P + i], "comparison": better_labels(results[i], results[P + i])} for i in range(P)]
    avg = [{k: sum(r[k] for r in part) / P for k in ("mse", "psnr", "ssim")} for part in (results[:P], results[P:])]
    return rows, avg[0], avg[1]


# ---- the Frechet distance of the reference's m_test.py (csrc/frechet.hip) ------------------------------------------------------------
MAX_SAMPLES, MAX_SWEEPS = _lib.FRECHET_MAX_SAMPLES, _lib.FRECHET_MAX_SWEEPS


def _req_features(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"mstg_hip metrics: {name} must be a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"mstg_hip metrics: {name} must live on the GPU, got a {t.device} tensor")
    if t.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"mstg_hip metrics: {name} must be float32 or float64, got {t.dtype}")
    if t.dim() != 2:
        raise RuntimeError(f"mstg_hip metrics: {name} must be (n, d), got {tuple(t.shape)}")
    return t.contiguous()


def _frechet_launch(real: torch.Tensor, fake: torch.Tensor):
    """-> (out (5,) float64 cuda {ssdiff, tr1, tr2, nuclear, fid}, info (2,) int32 cuda {sweeps, converged})"""
    a, b = _req_features(real, "real"), _req_features(fake, "fake")
    if a.dtype != b.dtype or a.device != b.device:
        raise RuntimeError(f"mstg_hip metrics: feature sets differ in dtype or device: {a.dtype} {a.device} vs {b.dtype} {b.device}")
    if a.shape[1] != b.shape[1]:
        raise RuntimeError(f"mstg_hip metrics: feature widths differ, {a.shape[1]} vs {b.shape[1]}")
    lib = _lib.load()
    n1, n2, d = a.shape[0], b.shape[0], a.shape[1]
    out = torch.empty(5, dtype=torch.float64, device=a.device)
    info = torch.empty(2, dtype=torch.int32, device=a.device)
    nbytes = lib.mstg_frechet_workspace_bytes(n1, n2, d)  # 0 for a refused shape: the call below names what is wrong
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=a.device)
    _lib.check(lib.mstg_frechet_distance(_p(a), _p(b), int(a.dtype == torch.float64), n1, n2, d, _p(out), _p(info), _p(ws), ws.numel() * 8,
                                         _stream()), "mstg_frechet_distance")
    return out, info


def frechet_distance(real: torch.Tensor, fake: torch.Tensor, return_parts=False):
    """``calculate_fid`` of the reference's m_test.py (:37-50) for (n1, d) and (n2, d) float32 or float64 feature sets on the GPU,
    in float64 throughout: ``|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2)`` with the last trace taken as the nuclear norm of
    ``A B^T`` (A, B the centred features over sqrt(n - 1)), found by a one-sided Jacobi SVD (include/mstg_hip.h).  Returns the
    distance as a 0-dim float64 cuda tensor; with ``return_parts`` a dict of 0-dim tensors ``ssdiff``, ``tr1``, ``tr2``, ``nuclear``,
    ``fid`` and the int32 tensor ``info`` = (sweeps used, converged).  No host synchronisation: the caller reads ``info``.
    ``min(n1, n2)`` above ``MAX_SAMPLES`` is refused (the d x d form is not built)."""
    out, info = _frechet_launch(real, fake)
    if return_parts:
        return {"ssdiff": out[0], "tr1": out[1], "tr2": out[2], "nuclear": out[3], "fid": out[4], "info": info}
    return out[4]


def singular_values(M: torch.Tensor, return_info=False):
    """The singular values of a float64 (m, n) cuda matrix, descending, by the one-sided Jacobi of ``frechet_distance`` alone
    (``min(m, n)`` at most ``MAX_SAMPLES``); one launch, no host synchronisation.  ``return_info``: also the int32 tensor
    (sweeps used, converged)."""
    if not isinstance(M, torch.Tensor) or not M.is_cuda or M.dtype != torch.float64 or M.dim() != 2:
        raise RuntimeError("mstg_hip metrics: singular_values takes a float64 (m, n) matrix on the GPU")
    x = M.contiguous()
    lib = _lib.load()
    m, n = x.shape
    sigma = torch.empty(max(min(m, n), 1), dtype=torch.float64, device=x.device)
    info = torch.empty(2, dtype=torch.int32, device=x.device)
    nbytes = lib.mstg_singular_values_workspace_bytes(m, n)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=x.device)
    _lib.check(lib.mstg_singular_values(_p(x), m, n, _p(sigma), _p(info), _p(ws), ws.numel() * 8, _stream()), "mstg_singular_values")
    sigma = sigma[:min(m, n)]
    return (sigma, info) if return_info else sigma


def calculate_fid(real_features, fake_features) -> float:
    """``calculate_fid`` of m_test.py as the reference calls it: numpy arrays or cuda tensors in, a Python float out after ONE
    device-to-host copy.  Raises if the Jacobi did not converge within ``MAX_SWEEPS`` sweeps."""
    def stage(x):
        if isinstance(x, np.ndarray):
            if x.dtype not in (np.float32, np.float64):
                x = x.astype(np.float64)
            x = np.ascontiguousarray(x)
            return torch.from_numpy(x if x.flags.writeable else x.copy()).cuda()
        return x
    out, info = _frechet_launch(stage(real_features), stage(fake_features))
    host = torch.cat([out, info.to(torch.float64)]).cpu().tolist()  # the one device-to-host copy
    if int(host[6]) != 1:
        raise RuntimeError(f"mstg_hip metrics: the Jacobi SVD did not converge within {int(host[5])} sweeps (non-finite features?)")
    return host[4]
