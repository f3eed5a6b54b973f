"""CPU restatement of the reference's colour-block repair (improved_smooth.py: detect_color_blocks :53-95,
adaptive_color_correction :10-51, edge_preserving_smoothing :97-112, detail_enhancing_blend :114-135 and the chain
fix_color_blocks_improved :137-164), written from the definitions in include/mstg_hip.h independently of the kernels
(csrc/color_blocks.hip): a and b of the 8-bit ``COLOR_RGB2LAB`` in OpenCV's integer path, ``cv2.Sobel(ksize=3)`` on float32, the
box dilation, the correction towards the window mean, ``cv2.bilateralFilter(img, 0, 0.4 * 255, 60)`` (radius 90) and the float64
``cv2.GaussianBlur(orig, (0, 0), 3)`` of the detail blend.

OpenCV is not a dependency of this repository: like tests/standard_mode_ref.py this module RESTATES OpenCV 4.x and HAS NOT BEEN
COMPARED WITH AN OPENCV BINARY.  tests/test_color_blocks_cpu.py pins it with closed forms and CIE Lab in float64 and measures how
far other plausible evaluations lie from the definition.
"""
import math

import numpy as np

from app_local_style_ref import blur_f64, gaussian_kernel_f64
from standard_mode_ref import fma_f32, reflect101, _padded

F32, F64 = np.float32, np.float64
XYZ = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
WHITE = (0.950456, 1.0, 1.088754)
MAX_RADIUS = 90


# ---- 1. the block mask --------------------------------------------------------------------------------------------------------------
def _lin(x, dt=F64):
    x = np.asarray(x, dtype=dt)
    return np.where(x <= dt(0.04045), x / dt(12.92), np.power((x + dt(0.055)) / dt(1.055), dt(2.4)))


def _f(x, dt=F64):
    x = np.asarray(x, dtype=dt)
    return np.where(x < dt(0.008856), dt(7.787) * x + dt(16.0) / dt(116.0), np.cbrt(x))


def lab_tables_unrounded(dt=F64):
    """(gamma, cbrt) before rounding, evaluated in ``dt`` (float64: the definition; float32: measured only)"""
    gamma = dt(2040) * _lin(np.arange(256, dtype=dt) / dt(255), dt)
    cbrt = dt(32768) * _f(np.arange(3072, dtype=dt) / dt(2040), dt)
    return gamma, cbrt


def lab_tables(dt=F64):
    """(gamma[256], cbrt[3072], C[3][3]) as int64"""
    gamma, cbrt = lab_tables_unrounded(dt)
    C = np.array([[round(4096 * XYZ[r][k] / WHITE[r]) for k in range(3)] for r in range(3)], dtype=np.int64)
    return np.rint(gamma).astype(np.int64), np.rint(cbrt).astype(np.int64), C


def lab_ab(rgb, tables=None):
    """(..., 3) uint8 RGB -> (a, b) of the 8-bit COLOR_RGB2LAB, int64"""
    gamma, cbrt, C = tables or lab_tables()
    lin = gamma[rgb.astype(np.int64)]
    f = [cbrt[(lin[..., 0] * C[r, 0] + lin[..., 1] * C[r, 1] + lin[..., 2] * C[r, 2] + 2048) >> 12] for r in range(3)]
    a = (500 * (f[0] - f[1]) + 128 * 32768 + 16384) >> 15  # numpy's >> on signed integers is arithmetic
    b = (200 * (f[1] - f[2]) + 128 * 32768 + 16384) >> 15
    return np.clip(a, 0, 255), np.clip(b, 0, 255)


def lab_ab_float64(rgb):
    """a, b of CIE Lab in float64, unrounded, with the offset of 128: what the integer path approximates"""
    lin = _lin(np.arange(256, dtype=F64) / 255.0)[rgb]  # a function of the byte alone
    m = np.array(XYZ, dtype=F64) / np.array(WHITE, dtype=F64)[:, None]
    f = [_f(lin[..., 0] * m[r, 0] + lin[..., 1] * m[r, 1] + lin[..., 2] * m[r, 2]) for r in range(3)]
    return 500.0 * (f[0] - f[1]) + 128.0, 200.0 * (f[1] - f[2]) + 128.0


def sobel3(plane):
    """cv2.Sobel(plane, CV_32F, 1, 0, ksize=3) and (0, 1) of a float32 plane, BORDER_REFLECT_101 -> (gx, gy) float32"""
    H, W = plane.shape
    p = _padded(plane.astype(F32), 1, reflect101)

    def at(dy, dx):
        return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (at(-1, 1) + F32(2) * at(0, 1) + at(1, 1)) - (at(-1, -1) + F32(2) * at(0, -1) + at(1, -1))
    gy = (at(1, -1) + F32(2) * at(1, 0) + at(1, 1)) - (at(-1, -1) + F32(2) * at(-1, 0) + at(-1, 1))
    return gx, gy


def block_edges(img, threshold=30):
    a, b = lab_ab(img)
    mags = []
    for plane in (a, b):
        gx, gy = sobel3(plane.astype(F32))
        mags.append(np.sqrt(gx * gx + gy * gy))  # float32, correctly rounded
    assert mags[0].dtype == F32
    c = (mags[0] + mags[1]) * F32(0.5)
    return c > F32(threshold)


def dilate_box(mask, k):
    """any() over the k x k window clipped to the image (cv2.dilate with a box, default border: neutral); k odd"""
    if k < 1 or k % 2 == 0:
        raise NotImplementedError(f"kernel_size = {k}")
    r = k // 2
    H, W = mask.shape
    p = np.zeros((H + 2 * r, W + 2 * r), dtype=bool)
    p[r:r + H, r:r + W] = mask
    rows = np.zeros((H + 2 * r, W), dtype=bool)
    for j in range(k):
        rows |= p[:, j:j + W]
    out = np.zeros((H, W), dtype=bool)
    for i in range(k):
        out |= rows[i:i + H]
    return out


def block_mask(img, threshold=30, kernel_size=11):
    """:53-95 -> bool (H, W)"""
    return dilate_box(block_edges(img, threshold), kernel_size)


# ---- 2. the correction --------------------------------------------------------------------------------------------------------------
def correct(img, mask, radius=50):
    """:10-51: a flagged pixel becomes 0.5 * px + 0.5 * mean of its window of the INPUT clipped to the image, truncated"""
    H, W = img.shape[:2]
    sat = np.zeros((H + 1, W + 1, 3), dtype=np.int64)
    sat[1:, 1:] = img.astype(np.int64).cumsum(axis=0).cumsum(axis=1)
    y, x = np.mgrid[0:H, 0:W]
    y0, y1 = np.maximum(y - radius, 0), np.minimum(y + radius + 1, H)
    x0, x1 = np.maximum(x - radius, 0), np.minimum(x + radius + 1, W)
    total = sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0]
    count = ((y1 - y0) * (x1 - x0))[..., None]
    mean = total.astype(F64) / count.astype(F64)
    v = 0.5 * img.astype(F64) + 0.5 * mean
    out = img.copy()
    out[mask] = v.astype(np.uint8)[mask]
    return out


# ---- 3. the wide bilateral filter ---------------------------------------------------------------------------------------------------
def bilateral_radius(d, sigma_space):
    """OpenCV's rule: d <= 0 derives the radius from sigmaSpace with cvRound (round half to even)"""
    sigma_space = sigma_space if sigma_space > 0 else 1
    radius = int(np.rint(sigma_space * 1.5)) if d <= 0 else d // 2
    return max(radius, 1)


def bilateral_taps(radius):
    return [(i, j) for i in range(-radius, radius + 1) for j in range(-radius, radius + 1) if math.sqrt(i * i + j * j) <= radius]


_TIE_MASK, _TIE = np.int64((1 << 29) - 1), np.int64(1 << 28)


def _fma_bytes(q64, w, acc):
    """fmaf(q, w, acc) for byte-valued q (float64, (..., C)), float32 w (...) and float32 acc (..., C).  The product is exact in
    float64 (8 + 24 bits); the float64 sum is rounded once more to float32, which is the rounding of the exact value unless the
    float64 sum is exactly halfway between two float32 values (float32 midpoints are float64 numbers and rounding is monotonic).
    Only then the slow, always exact emulation of tests/standard_mode_ref.py decides."""
    s = q64 * w.astype(F64)[..., None] + acc
    r = s.astype(F32)
    tie = (s.view(np.int64) & _TIE_MASK) == _TIE
    if tie.any():
        at = np.nonzero(tie)
        r[at] = fma_f32(q64[at].astype(F32), w[at[:-1]], acc[at])
    return r


def bilateral_wide_all(imgs, d=0, sigma_color=0.4 * 255, sigma_space=60, coords=None, others=False):
    """cv2.bilateralFilter of every image of an (N, H, W, 3) uint8 batch at any radius up to 90, by the definition of
    include/mstg_hip.h.  ``coords`` = a list of (y, x): only these pixels are evaluated, -> (N, len(coords), 3); None: all pixels,
    -> (N, H, W, 3).  Returns a dict: 'definition' and, with ``others``, three evaluations that are NOT the definition ('unfused',
    'divide', 'float64', as tests/standard_mode_ref.py names them)."""
    imgs = np.asarray(imgs)
    N, H, W = imgs.shape[:3]
    radius = bilateral_radius(d, sigma_space)
    if radius > MAX_RADIUS:
        raise NotImplementedError(f"radius = {radius}")
    sigma_color = sigma_color if sigma_color > 0 else 1
    sigma_space = sigma_space if sigma_space > 0 else 1
    gc, gs = -0.5 / (sigma_color * sigma_color), -0.5 / (sigma_space * sigma_space)
    color64 = np.array([math.exp(t * t * gc) for t in range(768)], dtype=F64)
    color = color64.astype(F32)
    if coords is None:
        yy, xx = (a.reshape(-1) for a in np.mgrid[0:H, 0:W])
    else:
        yy, xx = np.array([c[0] for c in coords]), np.array([c[1] for c in coords])
    ry, rx = reflect101(np.arange(-radius, H + radius), H), reflect101(np.arange(-radius, W + radius), W)
    pad = np.ascontiguousarray(imgs.astype(np.int32)[:, ry][:, :, rx])  # BORDER_REFLECT_101, as often as the radius needs
    PW = W + 2 * radius
    flat, at = pad.reshape(N, -1, 3), (yy + radius) * PW + xx + radius
    c0 = flat[:, at]  # (N, P, 3)
    P = len(yy)
    acc = np.zeros((N, P, 4), F32)  # the three channel sums and wsum: wsum + w is fmaf(1, w, wsum)
    q4 = np.ones((N, P, 4), F64)
    su, wsum64, s64 = np.zeros((N, P, 3), F32), np.zeros((N, P), F64), np.zeros((N, P, 3), F64)
    for i, j in bilateral_taps(radius):
        sp64 = math.exp((i * i + j * j) * gs)
        if coords is None:
            q = pad[:, radius + i:radius + i + H, radius + j:radius + j + W].reshape(N, P, 3)
        else:
            q = np.take(flat, at + (i * PW + j), axis=1)
        dist = np.abs(q - c0)
        t = dist[..., 0] + dist[..., 1] + dist[..., 2]
        w = F32(sp64) * color[t]  # float32 * float32: one rounded product
        q4[..., :3] = q
        acc = _fma_bytes(q4, w, acc)
        if others:
            su = su + q.astype(F32) * w[..., None]
            w64 = sp64 * color64[t]
            wsum64 += w64
            s64 += q * w64[..., None]
    s, wsum = acc[..., :3], acc[..., 3]

    def u8(x):
        return np.clip(np.rint(x), 0, 255).astype(np.uint8)
    inv = F32(1.0) / wsum  # IEEE division in float32
    out = {"definition": u8(s * inv[..., None])}
    if others:
        out["unfused"] = u8(su * inv[..., None])
        out["divide"] = u8(s / wsum[..., None])
        out["float64"] = u8(s64 / wsum64[..., None])
    if coords is None:
        out = {k: v.reshape(N, H, W, 3) for k, v in out.items()}
    return out


def bilateral_wide(imgs, d=0, sigma_color=0.4 * 255, sigma_space=60, coords=None):
    return bilateral_wide_all(imgs, d, sigma_color, sigma_space, coords)["definition"]


# ---- 4. the detail blend ------------------------------------------------------------------------------------------------------------
def detail_ksize(sigma):
    """cv2.GaussianBlur's size for ksize = (0, 0) and a depth other than 8 bits: cvRound(sigma * 4 * 2 + 1) | 1"""
    return int(np.rint(sigma * 4 * 2 + 1)) | 1


def detail_blend(img, orig, alpha=0.3, beta=1.5, sigma=3.0):
    """:114-135 on (H, W, 3) uint8 arrays of one size: the reference's own numpy expression around the float64 blur"""
    k = gaussian_kernel_f64(detail_ksize(sigma), sigma)
    img_np, orig_np = img.astype(float), orig.astype(float)
    blurred = np.stack([blur_f64(orig_np[..., c], k) for c in range(3)], axis=-1)
    detail = orig_np - blurred
    blended = img_np * (1 - alpha) + orig_np * alpha + detail * beta
    return np.clip(blended, 0, 255).astype(np.uint8)


# ---- the chain ----------------------------------------------------------------------------------------------------------------------
def fix_color_blocks(img, orig=None, coords=None):
    """:137-164 on (H, W, 3) uint8 arrays (``orig`` of the same size); ``coords``: evaluate the bilateral filter, and so the result,
    only at these pixels -> (len(coords), 3)"""
    corrected = correct(img, block_mask(img))
    smoothed = bilateral_wide(corrected[None], 0, 0.4 * 255, 60, coords)[0]
    if orig is None:
        return smoothed
    if coords is None:
        return detail_blend(smoothed, orig, alpha=0.1, beta=0.5)
    full = np.zeros_like(img)
    yy, xx = np.array([c[0] for c in coords]), np.array([c[1] for c in coords])
    full[yy, xx] = smoothed
    return detail_blend(full, orig, alpha=0.1, beta=0.5)[yy, xx]


# ---- test inputs --------------------------------------------------------------------------------------------------------------------
PALETTE = ((220, 20, 20), (20, 220, 20), (20, 20, 220), (220, 220, 20), (20, 220, 220), (220, 20, 220))


def blocks(h, w, seed, cell=32):
    """(h, w, 3) uint8: flat cells of saturated colours, neighbouring cells always of different colours: block edges between the
    cells and nothing inside them, so the mask flags a band around every cell border and leaves the interiors"""
    i, j = np.mgrid[0:h // cell + 1, 0:w // cell + 1]
    cells = np.array(PALETTE, dtype=np.uint8)[(2 * i + j + seed) % len(PALETTE)]
    return np.ascontiguousarray(np.kron(cells, np.ones((cell, cell, 1), dtype=np.uint8))[:h, :w])
