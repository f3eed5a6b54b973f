"""CPU restatement of the five settings of the reference's advanced_transform.py (:129-311) as include/mstg_hip.h defines them,
written independently of the kernels (csrc/advanced_transform.hip): the 8-bit RGB <-> Lab round trip, the 8-bit
``cv2.GaussianBlur(plane, (0, 0), sigma)`` in 8.8 fixed point, the HSV gains, this build's deterministic K-means, the region blend,
the fusion of scales, the three chains and ``process_advanced``.

OpenCV is not a dependency of this repository: like tests/color_blocks_ref.py this module RESTATES OpenCV 4.x as recalled and HAS
NOT BEEN COMPARED WITH AN OPENCV BINARY; the Lab -> RGB constants and the K-means are this build's own definitions
(include/mstg_hip.h says which parts are which).  tests/test_advanced_transform_cpu.py pins it with closed forms, float64 CIE Lab
and scikit-learn's Lloyd iteration.
"""
import math

import numpy as np

from app_local_style_ref import blur_u8_fixed, hsv_u8
from color_blocks_ref import WHITE, lab_tables
from enhanced_local_style_ref import clahe, hsv2rgb_u8
from local_style_ref import gray_u8

F32, F64 = np.float32, np.float64
XYZ_INV = ((3.240479, -1.53715, -0.498535), (-0.969256, 1.875991, 0.041556), (0.055648, -0.204043, 1.057311))
CUBE_N, ENC_N = 6720, 8193
MAX_KSIZE, MAX_K, MAX_ATTEMPTS = 31, 16, 16


# ---- 1, 2. Lab ----------------------------------------------------------------------------------------------------------------------
def lab_u8(rgb, tables=None):
    """(..., 3) uint8 RGB -> (..., 3) uint8 (L, a, b) of the 8-bit COLOR_RGB2LAB"""
    gamma, cbrt, C = tables or lab_tables()
    lin = gamma[rgb.astype(np.int64)]
    f = [cbrt[(lin[..., 0] * C[r, 0] + lin[..., 1] * C[r, 1] + lin[..., 2] * C[r, 2] + 2048) >> 12] for r in range(3)]
    L = (296 * f[1] - 1336934 + 16384) >> 15
    a = (500 * (f[0] - f[1]) + 128 * 32768 + 16384) >> 15
    b = (200 * (f[1] - f[2]) + 128 * 32768 + 16384) >> 15
    return np.clip(np.stack([L, a, b], axis=-1), 0, 255).astype(np.uint8)


def _fy(L):
    ls = np.asarray(L, dtype=F64) * 100.0 / 255.0
    return np.where(ls <= 8.0, 7.787 * (ls / 903.3) + 16.0 / 116.0, (ls + 16.0) / 116.0)


def _g(t):
    t = np.asarray(t, dtype=F64)
    return np.where(t > 6.0 / 29.0, t * t * t, (t - 16.0 / 116.0) / 7.787)


def _enc(x):
    x = np.asarray(x, dtype=F64)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0), 1.0 / 2.4) - 0.055)


def lab_inverse_tables_unrounded():
    v = np.arange(256, dtype=F64)
    fy = 32768.0 * _fy(v)
    da, db = 32768.0 * (v - 128) / 500.0, 32768.0 * (v - 128) / 200.0
    cube = 8192.0 * np.maximum(_g(np.arange(CUBE_N, dtype=F64) * 8.0 / 32768.0), 0.0)
    D = np.array([[4096.0 * XYZ_INV[r][k] * WHITE[k] for k in range(3)] for r in range(3)])
    enc = 255.0 * _enc(np.arange(ENC_N, dtype=F64) / 8192.0)
    return fy, da, db, cube, D, enc


def lab_inverse_tables():
    """(fy[256], da[256], db[256], cube[6720], D[3][3], enc[8193]) as int64"""
    return tuple(np.rint(t).astype(np.int64) for t in lab_inverse_tables_unrounded())


def lab_inverse_flat(tables=None):
    """the layout of mstg_lab_inverse_tables, as int64 (signed entries not yet wrapped to 16 bits)"""
    fy, da, db, cube, D, enc = tables or lab_inverse_tables()
    return np.concatenate([fy, da, db, cube, D.reshape(-1), enc])


def lab2rgb_u8(lab, tables=None):
    """(..., 3) uint8 (L, a, b) -> (..., 3) uint8 RGB: this build's integer path, defined for every byte triple"""
    fy_t, da, db, cube, D, enc = tables or lab_inverse_tables()
    q = lab.astype(np.int64)
    fy = fy_t[q[..., 0]]
    fx, fz = fy + da[q[..., 1]], fy - db[q[..., 2]]
    g = []
    for f in (fx, fy, fz):
        f = np.clip(f, 0, 8 * (CUBE_N - 1) - 1)
        i, frac = f >> 3, f & 7
        g.append(cube[i] + (((cube[i + 1] - cube[i]) * frac + 4) >> 3))  # linear interpolation between two entries
    out = [enc[np.clip((D[c, 0] * g[0] + D[c, 1] * g[1] + D[c, 2] * g[2] + 2048) >> 12, 0, ENC_N - 1)] for c in range(3)]
    return np.stack(out, axis=-1).astype(np.uint8)


def lab2rgb_float64(lab):
    """the CIE inverse of Lab BYTES in float64 -> RGB in [0, 255], clipped, unrounded: what the integer path approximates"""
    q = lab.astype(F64)
    fy = _fy(q[..., 0])
    fx, fz = fy + (q[..., 1] - 128.0) / 500.0, fy - (q[..., 2] - 128.0) / 200.0
    xyz = [np.maximum(_g(f), 0.0) * w for f, w in zip((fx, fy, fz), WHITE)]
    out = [255.0 * _enc(np.clip(XYZ_INV[c][0] * xyz[0] + XYZ_INV[c][1] * xyz[1] + XYZ_INV[c][2] * xyz[2], 0.0, 1.0)) for c in range(3)]
    return np.stack(out, axis=-1)


# ---- 3. the 8-bit Gaussian ----------------------------------------------------------------------------------------------------------
def sigma_ksize(sigma):
    """cv2.GaussianBlur's size for ksize = (0, 0) on 8 bits: cvRound(sigma * 6 + 1) | 1"""
    return int(np.rint(sigma * 6 + 1)) | 1


def sigma_taps(sigma):
    """(taps, the smallest distance of a rounded quantity from a tie): the generator of app_local_style_ref.fixed_point_taps at a
    given sigma"""
    ksize = sigma_ksize(sigma)
    if ksize > MAX_KSIZE:
        raise NotImplementedError(f"ksize = {ksize}")
    r = ksize // 2
    t = [math.exp(-0.5 * float((i - r) * (i - r)) / (sigma * sigma)) for i in range(ksize)]
    total = 0.0
    for v in t:
        total += v
    taps, err, margin = [], 0.0, 1.0
    for i in range(r):
        a = t[i] / total * 256 + err
        q = round(a)  # half to even
        margin = min(margin, abs(abs(a - math.floor(a)) - 0.5))
        err = a - q
        taps.append(int(q))
    return taps + [256 - 2 * sum(taps)] + taps[::-1], margin


def gaussian_sigma_u8(plane, sigma=3.0):
    return blur_u8_fixed(plane, sigma_taps(sigma)[0])


# ---- 4. the HSV gains ---------------------------------------------------------------------------------------------------------------
def gain_u8(v, gain, dtype=F32):
    return np.clip(np.rint(np.asarray(v).astype(dtype) * dtype(gain)), 0, 255).astype(np.int64)


def hsv_gain_u8(rgb, s_gain=1.2, v_gain=1.0):
    h, s, v = hsv_u8(rgb)
    return np.ascontiguousarray(hsv2rgb_u8(h, gain_u8(s, s_gain), gain_u8(v, v_gain)))


# ---- 5. K-means ---------------------------------------------------------------------------------------------------------------------
def uniforms(seed, attempts, K):
    return np.random.RandomState(seed).random_sample(attempts * K * 3).astype(F32).reshape(attempts, K, 3)


def km_assign(px, cen):
    """px (P, 3) uint8, cen (K, 3) float32 -> labels: the nearest centre in float32, the lowest index wins a tie"""
    d = px.astype(F32)[:, None, :] - cen[None, :, :]
    d2 = d * d
    dist = (d2[..., 0] + d2[..., 1]) + d2[..., 2]
    assert dist.dtype == F32
    return np.argmin(dist, axis=1)  # the first minimum


def km_sums(px, labels, K):
    p = px.astype(np.int64)  # the float64 weights of bincount are exact: every sum stays below 2^53
    n = np.bincount(labels, minlength=K).astype(np.int64)
    s1 = np.stack([np.bincount(labels, weights=p[:, c], minlength=K) for c in range(3)], axis=1).astype(np.int64)
    s2 = np.stack([np.bincount(labels, weights=p[:, c] * p[:, c], minlength=K) for c in range(3)], axis=1).astype(np.int64)
    return n, s1, s2


def km_attempt(px, cen, iters, eps):
    """one problem -> (centres float32 (K, 3), compactness float64, rounds used)"""
    cen = cen.astype(F32).copy()
    K = cen.shape[0]
    used = 0
    for _ in range(iters):
        n, s1, _ = km_sums(px, km_assign(px, cen), K)
        used += 1
        new = cen.copy()
        for k in range(K):
            if n[k]:
                new[k] = (s1[k].astype(F64) / F64(n[k])).astype(F32)
        e = new.astype(F64) - cen.astype(F64)
        e2 = e * e
        shift = ((e2[:, 0] + e2[:, 1]) + e2[:, 2]).max()
        cen = new
        if shift <= eps * eps:
            break
    n, s1, s2 = km_sums(px, km_assign(px, cen), K)
    comp = F64(0)
    for k in range(K):
        for ch in range(3):
            c = F64(cen[k, ch])
            comp = comp + ((F64(s2[k, ch]) - (F64(2.0) * c) * F64(s1[k, ch])) + (F64(n[k]) * c) * c)
    return cen, float(comp), used


def kmeans_u8(img, K=5, attempts=10, iters=10, eps=1.0, seed=0, centers0=None):
    """(H, W, 3) uint8 -> (labels int32 (H, W), centres float32 (K, 3), compactness, winning attempt)"""
    if not 1 <= K <= MAX_K:
        raise NotImplementedError(f"K = {K}")
    if not 1 <= attempts <= MAX_ATTEMPTS:
        raise NotImplementedError(f"attempts = {attempts}")
    H, W = img.shape[:2]
    px = img.reshape(-1, 3)
    if centers0 is not None:
        assert attempts == 1
        starts = [np.asarray(centers0, dtype=F32).reshape(K, 3)]
    else:
        lo, hi = px.min(axis=0).astype(F32), px.max(axis=0).astype(F32)
        starts = [lo[None, :] + u * (hi - lo)[None, :] for u in uniforms(seed, attempts, K)]
        assert all(s.dtype == F32 for s in starts)
    best = None
    for a, start in enumerate(starts):
        cen, comp, _ = km_attempt(px, start, iters, eps)
        if best is None or comp < best[1]:
            best = (cen, comp, a)
    cen, comp, a = best
    return km_assign(px, cen).astype(np.int32).reshape(H, W), cen, comp, a


# ---- 6, 7. the region blend and the fusion ------------------------------------------------------------------------------------------
def region_blend_u8(styled, orig, labels, ratios=(0.8, 0.4, 0.6)):
    r = np.asarray(ratios, dtype=F64)[np.clip(labels, 0, len(ratios) - 1)][..., None]
    x = styled.astype(F64) * r + orig.astype(F64) * (1 - r)
    out = np.clip(x, 0, 255).astype(np.uint8)
    out[labels < 0] = 0
    return out


def fuse_scales_u8(outputs, weights=(0.2, 0.3, 0.5), gain=1.1):
    fused = np.zeros(outputs[0].shape, dtype=F32)
    for o, w in zip(outputs, weights):
        fused = fused + (o.astype(F32) / F32(255.0)) * F32(w)
    fused = np.clip(fused * F32(gain), 0, 1)
    assert fused.dtype == F32
    return (fused * F32(255.0)).astype(np.uint8)


# ---- the chains ---------------------------------------------------------------------------------------------------------------------
def contrast_enhanced_finish(styled):
    lab = lab_u8(styled)
    lab[..., 0] = clahe(np.ascontiguousarray(lab[..., 0]))
    return hsv_gain_u8(lab2rgb_u8(lab), 1.2, 1.0)


def detail_enhanced_finish(styled, orig):
    grey = gray_u8(orig).astype(np.uint8)
    detail = grey - gaussian_sigma_u8(grey, 3.0)  # uint8 arithmetic wraps
    assert detail.dtype == np.uint8
    lab = lab_u8(styled)
    lab[..., 0] = np.clip(lab[..., 0].astype(F32) + detail.astype(F32) * F32(0.5), 0, 255).astype(np.uint8)
    return hsv_gain_u8(lab2rgb_u8(lab), 1.2, 1.1)


def local_regions_finish(styled, orig, seed=0):
    labels = kmeans_u8(orig, seed=seed)[0]
    return hsv_gain_u8(region_blend_u8(styled, orig, labels), 1.2, 1.0)


# ---- test inputs --------------------------------------------------------------------------------------------------------------------
def noise(h, w, seed, n=None):
    rng = np.random.RandomState(seed)
    shape = (h, w, 3) if n is None else (n, h, w, 3)
    return rng.randint(0, 256, size=shape).astype(np.uint8)


def smooth(h, w, seed):
    """a smooth colour field with a few flat patches: clusters with interiors, CLAHE tiles with structure"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([127 + 120 * np.sin(x / (3.0 + c) + rng.rand() * 6) * np.cos(y / (5.0 - c) + rng.rand() * 6) for c in range(3)], axis=-1)
    img = np.clip(img + rng.randint(-6, 7, size=img.shape), 0, 255).astype(np.uint8)
    img[: h // 3, : w // 4] = rng.randint(0, 256, size=3)
    return np.ascontiguousarray(img)
