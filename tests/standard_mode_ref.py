"""CPU restatement of the finish of the standard mode of the reference's application (gan_login_gui.py:817-868,
standard_process_thread): the blend with the canvas, ``cv2.medianBlur(3)``, ``cv2.bilateralFilter(d, sigmaColor, sigmaSpace)``,
the colour step of the direction and ``cv2.GaussianBlur((k, k), 0)``, written from the definitions in include/mstg_hip.h
independently of the kernels (csrc/standard_mode.hip), and the mode's caller around it (:769-889).

OpenCV is not a dependency of this repository: like tests/local_style_finish_ref.py this module RESTATES OpenCV 4.x -- the median
with BORDER_REPLICATE, ``bilateralFilter_8u`` for three channels on a build with FMA lanes (float32 in tap order, one rounded weight
product, fused channel sums, one reciprocal, round half to even, BORDER_REFLECT_101), ``cvtabs`` on uint8 input and the bit-exact
8-bit blur for sizes 3, 5, 7 -- and HAS NOT BEEN COMPARED WITH AN OPENCV BINARY.  tests/test_standard_mode_cpu.py pins it against
scipy, the existing blur restatement and closed forms, and measures how far other plausible evaluations of the floating-point
steps lie from the definition.
"""
import math

import numpy as np

from oracle import image_ref as IR

F32, F64 = np.float32, np.float64
GAUSS_TAPS = {3: [64, 128, 64], 5: [16, 64, 96, 64, 16], 7: [8, 28, 56, 72, 56, 28, 8]}  # OpenCV's sigma <= 0 tables times 256
MODEL_TYPES = ("photo_to_monet", "monet_to_photo")


# ---- borders ------------------------------------------------------------------------------------------------------------------------
def reflect101(p, n):
    """cv2.borderInterpolate(p, n, BORDER_REFLECT_101) for an integer array: reflect about the first / last pixel without repeating
    it, again and again while the index is outside; n == 1 gives 0"""
    p = np.array(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * n - 2 - p, p)
    return p


def _padded(img, radius, index):
    H, W = img.shape[:2]
    return img[index(np.arange(-radius, H + radius), H)][:, index(np.arange(-radius, W + radius), W)]


# ---- the integer steps --------------------------------------------------------------------------------------------------------------
def blend(styled, canvas, ratio):
    """:820-828: the reference's own numpy expression; a ratio that is not > 0 skips the step"""
    if not ratio > 0:
        return styled.copy()
    return np.clip(styled * (1 - ratio) + canvas * ratio, 0, 255).astype(np.uint8)


def median3(img):
    """cv2.medianBlur(img, 3) of an (H, W, 3) uint8 array: the fifth of the nine sorted samples, coordinates clamped to the image"""
    H, W = img.shape[:2]
    pad = _padded(img, 1, lambda p, n: np.clip(p, 0, n - 1))
    nine = np.stack([pad[i:i + H, j:j + W] for i in range(3) for j in range(3)])
    return np.sort(nine, axis=0)[4]


def gaussian(img, ksize):
    """cv2.GaussianBlur(img, (ksize, ksize), 0) of an (H, W, 3) uint8 array in 8.8 fixed point: along x, then along y"""
    if ksize not in GAUSS_TAPS:
        raise NotImplementedError(f"ksize {ksize} (smooth_level {ksize // 2}) is not restated")
    taps, r = GAUSS_TAPS[ksize], ksize // 2
    H, W = img.shape[:2]
    v = img.astype(np.int64)
    px = v[:, reflect101(np.arange(-r, W + r), W)]
    h = sum(t * px[:, k:k + W] for k, t in enumerate(taps))
    assert h.max(initial=0) <= 65280  # the row sums fit 16 bits
    py = h[reflect101(np.arange(-r, H + r), H)]
    s = sum(t * py[k:k + H] for k, t in enumerate(taps))
    return ((s + 32768) >> 16).astype(np.uint8)


# ---- the colour step ----------------------------------------------------------------------------------------------------------------
def scale_abs_u8(v):
    """sat_u8(rint_half_even(|fmaf(float32(v), 1.1f, 5.0f)|)) for bytes: product and sum are exact in float64 (8 + 24 bits), so the
    one rounding to float32 is the rounding of the fused operation"""
    t = (np.asarray(v).astype(F32).astype(F64) * F64(F32(1.1)) + 5.0).astype(F32)
    return np.clip(np.rint(np.abs(t)), 0, 255).astype(np.uint8)


def scale_abs_u8_unfused(v):
    """float32 with a rounded product and a rounded sum: NOT the definition"""
    return np.clip(np.rint(np.abs(np.asarray(v).astype(F32) * F32(1.1) + F32(5.0))), 0, 255).astype(np.uint8)


def scale_abs_u8_float64(v):
    """plain float64: NOT the definition"""
    return np.clip(np.rint(np.abs(np.asarray(v).astype(F64) * 1.1 + 5.0)), 0, 255).astype(np.uint8)


def color_lut(model_type):
    """(3, 256) uint8: the table of channel c is row c (:848-854; the indices of the code, not of its comments)"""
    v = np.arange(256, dtype=np.uint8)
    if model_type == "photo_to_monet":
        return np.stack([np.clip(v * 1.1, 0, 255).astype(np.uint8), np.clip(v * 1.05, 0, 255).astype(np.uint8), v])
    if model_type == "monet_to_photo":
        return np.stack([scale_abs_u8(v)] * 3)
    raise ValueError(model_type)


def apply_lut(img, lut):
    return np.stack([lut[c][img[..., c]] for c in range(3)], axis=-1)


# ---- the bilateral filter -----------------------------------------------------------------------------------------------------------
def bilateral_tables(d, sigma_color, sigma_space, narrow=True):
    """(taps, space, color): the tap list (i, j) in the definition's order and the two weight tables, math.exp in double then
    narrowed to float32 (``narrow=False``: left in double, for the float64 evaluation)"""
    if d not in (3, 5, 7, 9):
        raise NotImplementedError(f"d = {d}")
    sigma_color = sigma_color if sigma_color > 0 else 1
    sigma_space = sigma_space if sigma_space > 0 else 1
    radius = max(d // 2, 1)
    gc, gs = -0.5 / (sigma_color * sigma_color), -0.5 / (sigma_space * sigma_space)
    taps = [(i, j) for i in range(-radius, radius + 1) for j in range(-radius, radius + 1) if math.sqrt(i * i + j * j) <= radius]
    dt = F32 if narrow else F64
    space = np.array([math.exp((i * i + j * j) * gs) for i, j in taps], dtype=F64).astype(dt)
    color = np.array([math.exp(t * t * gc) for t in range(768)], dtype=F64).astype(dt)
    return taps, space, color


def fma_f32(a, b, c, stats=None):
    """fmaf(a, b, c) on float32 arrays whose product a * b is exact in float64 (here: a byte times a float32), emulated in float64.
    The float64 sum product + c can be inexact (the weights reach exp(-52) and below), and rounding it twice could break a
    would-be float32 tie the wrong way: the sum's error term (TwoSum) turns the float64 sum into the round-to-odd one, whose
    rounding to float32 is the rounding of the exact value.  ``stats`` counts the operations, the inexact float64 sums and the
    results the correction changed."""
    p = np.asarray(a, dtype=F32).astype(F64) * np.asarray(b, dtype=F32).astype(F64)
    c64 = np.broadcast_to(np.asarray(c, dtype=F32).astype(F64), p.shape)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    bits = np.ascontiguousarray(s).view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0)  # inexact and even: step to the odd neighbour on the side of the exact value
    down = (err < 0) == (s > 0)           # towards zero in the bit pattern
    odd = np.where(fix, np.where(down, bits - 1, bits + 1), bits).view(F64)
    r = odd.astype(F32)
    if stats is not None:
        stats["fma"] = stats.get("fma", 0) + int(r.size)
        stats["inexact"] = stats.get("inexact", 0) + int((err != 0).sum())
        stats["fired"] = stats.get("fired", 0) + int((r != s.astype(F32)).sum())
    return r


def bilateral_all(img, d=9, sigma_color=75, sigma_space=75, stats=None, others=True):
    """cv2.bilateralFilter of an (H, W, 3) uint8 array -> dict: 'definition' (include/mstg_hip.h) and, with ``others``, three
    evaluations that are NOT the definition: 'unfused' (rounded product, rounded sum in float32), 'divide' (the definition's sums
    divided by wsum instead of multiplied by its reciprocal) and 'float64' (tables, sums and division in double)"""
    H, W = img.shape[:2]
    taps, space, color = bilateral_tables(d, sigma_color, sigma_space)
    _, space64, color64 = bilateral_tables(d, sigma_color, sigma_space, narrow=False)
    radius = max(d // 2, 1)
    pad = _padded(img, radius, reflect101).astype(np.int32)
    c0 = img.astype(np.int32)
    wsum, s = np.zeros((H, W), F32), np.zeros((H, W, 3), F32)
    su = np.zeros((H, W, 3), F32)
    wsum64, s64 = np.zeros((H, W), F64), np.zeros((H, W, 3), F64)
    for k, (i, j) in enumerate(taps):
        q = pad[radius + i:radius + i + H, radius + j:radius + j + W]
        t = np.abs(q - c0).sum(axis=2)
        w = space[k] * color[t]  # float32 * float32: one rounded product
        wsum = wsum + w
        qf = q.astype(F32)
        s = fma_f32(qf, w[..., None], s, stats)
        if others:
            su = su + qf * w[..., None]
            w64 = space64[k] * color64[t]
            wsum64 += w64
            s64 += q * w64[..., None]

    def u8(x):
        return np.clip(np.rint(x), 0, 255).astype(np.uint8)
    inv = F32(1.0) / wsum  # IEEE division in float32
    out = {"definition": u8(s * inv[..., None])}
    if others:
        out["unfused"] = u8(su * inv[..., None])
        out["divide"] = u8(s / wsum[..., None])
        out["float64"] = u8(s64 / wsum64[..., None])
    return out


def bilateral(img, d=9, sigma_color=75, sigma_space=75, stats=None):
    return bilateral_all(img, d, sigma_color, sigma_space, stats, others=False)["definition"]


# ---- the chain and its caller -------------------------------------------------------------------------------------------------------
def standard_finish(canvas, styled, model_type, blend_ratio=0.3, fix_blocks=True, enhance_colors=True, smooth_level=3, adaptive_smooth=True):
    """:817-868 on (H, W, 3) uint8 arrays"""
    if model_type not in MODEL_TYPES:
        raise ValueError(model_type)
    x = blend(styled, canvas, blend_ratio)
    if fix_blocks:
        x = bilateral(median3(x), 9, 75, 75)
    if enhance_colors:
        x = apply_lut(x, color_lut(model_type))
    if adaptive_smooth and smooth_level > 0:
        x = gaussian(x, 2 * smooth_level + 1)
    return x


def process_standard(model_fn, img, model_type, target=256, resize=IR.pil_resize, **options):
    """standard_process_thread (:769-889) without file I/O; ``model_fn``: (1, 3, T, T) float32 -> (1, 3, T, T) float32"""
    height, width = img.shape[:2]
    if width > height:
        new_width, new_height = target, int(height * (target / width))
    else:
        new_height, new_width = target, int(width * (target / height))
    canvas = np.full((target, target, 3), 255, dtype=np.uint8)
    off_x, off_y = (target - new_width) // 2, (target - new_height) // 2
    canvas[off_y:off_y + new_height, off_x:off_x + new_width] = resize(img, (new_width, new_height), IR.LANCZOS)
    styled = IR.output_to_u8(np.asarray(model_fn(IR.to_tensor_normalize(canvas)[None]))[0])
    out = standard_finish(canvas, styled, model_type, **options)
    if width != height:
        aspect = width / height
        if aspect > 1:
            crop_w, crop_h = target, int(target / aspect)
        else:
            crop_h, crop_w = target, int(target * aspect)
        left, top = (target - crop_w) // 2, (target - crop_h) // 2
        out = out[top:top + crop_h, left:left + crop_w]
    if width * height <= 1024 * 1024:
        out = resize(np.ascontiguousarray(out), (width, height), IR.LANCZOS)
    return out


# ---- test images --------------------------------------------------------------------------------------------------------------------
KINDS = ("noise", "blocky", "gradient", "constant", "step")


def image(kind, h, w, seed):
    """(h, w, 3) uint8: 'noise'; 'blocky' = 4 x 4 cells of few levels (rich in equal samples and exact ties); 'gradient' = smooth
    ramps with a different slope per channel; 'constant'; 'step' = 0 / 255 in all channels with an oblique edge, whose colour
    distances reach 765, the smallest colour weights"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    if kind == "blocky":
        cells = rs.randint(0, 8, size=(h // 4 + 1, w // 4 + 1, 3)) * 36
        return np.ascontiguousarray(np.kron(cells, np.ones((4, 4, 1), dtype=np.int64))[:h, :w].astype(np.uint8))
    if kind == "gradient":
        return np.stack([(yy * 2 + xx) % 256, (xx * 3) % 256, (255 - yy - xx // 2) % 256], axis=-1).astype(np.uint8)
    if kind == "constant":
        return np.full((h, w, 3), int(rs.randint(1, 255)), dtype=np.uint8)
    if kind == "step":
        return np.repeat((((xx + yy // 3 + seed) // 5) % 2 * 255).astype(np.uint8)[..., None], 3, axis=2)
    raise ValueError(kind)
