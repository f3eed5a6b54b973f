"""Image-quality metrics of the reference's evaluation scripts on the device (csrc/metrics.hip): MSE, PSNR and SSIM of uint8 HWC
image pairs as compare_image_quality.py:14-33, image_quality_comparison.py:11-34, complete_comparison.py:13-32 and
improved_image_compare.py:8-27 compute them (images / 255, ``np.mean((a - b) ** 2)``, skimage ``peak_signal_noise_ratio`` and
``structural_similarity(channel_axis=2)`` with ``data_range=1.0``).  The images stay on the GPU, e.g. straight from
``image.process_cyclegan``; only ``calculate_metrics`` and ``evaluate_pairs`` bring numbers to the host, once per call.
Below them the Frechet distance of two feature sets as the reference's m_test.py:37-50 computes it (csrc/frechet.hip):
``frechet_distance``, its Jacobi SVD alone (``singular_values``) and ``calculate_fid`` with the reference's signature.
"""
from __future__ import annotations

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
    one with cv2.resize there, which this package does not restate -- resize with ``image.resize_u8`` first."""
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
    {'mse', 'psnr', 'ssim'} that the reference's folder comparison prints (None for an empty list)."""
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
