"""numpy restatement of the display finish (csrc/display_finish.hip) as include/mstg_hip.h defines it, written from the definition and
independently of the kernels: plain Python loops over the 256 bins, int64 numpy arithmetic with floor shifts for the colour
conversions, float32 numpy one operation at a time.  The OpenCV steps are restated as recalled: NOTHING HERE HAS BEEN COMPARED WITH AN
OPENCV BINARY.
"""
import numpy as np

F32, F64 = np.float32, np.float64


def gamma_inputs(y):
    """v of step 1: (float)y * 0.5f + 0.5f, clamped to [0, 1], a NaN to 0; float32, the shape of y"""
    v = np.asarray(y).astype(F32) * F32(0.5) + F32(0.5)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.minimum(v, F32(1.0)), F32(0.0)).astype(F32)


def gamma_margin_ulps(v, gamma=1.1):
    """the smallest distance, in ulps of the float64 power, of pow((double)v, gamma) from a midpoint of two neighbouring float32
    values: where it is large no correctly working pow can round the other way"""
    p = np.power(v.astype(F64), F64(gamma)).ravel()
    f = p.astype(F32)
    lo = np.where(f.astype(F64) <= p, f, np.nextafter(f, F32(-np.inf)))
    hi = np.nextafter(lo, F32(np.inf))
    mid = (lo.astype(F64) + hi.astype(F64)) * 0.5  # exact: two neighbouring float32 values
    ulp = np.spacing(np.maximum(p, np.finfo(F64).tiny))
    return float(np.min(np.abs(p - mid) / ulp))


def gamma_u8(y, gamma=1.1):
    """(N, 3, H, W) or (3, H, W) float32 / float16 -> (N, H, W, 3) uint8"""
    y = np.asarray(y)
    if y.ndim == 3:
        y = y[None]
    v = gamma_inputs(y)
    p = np.power(v.astype(F64), F64(gamma)).astype(F32)
    b = (p * F32(255.0)).astype(F32)
    return np.ascontiguousarray(np.transpose(b.astype(np.uint8), (0, 2, 3, 1)))


def _sat(x):
    return np.clip(x, 0, 255)


def rgb2yuv(img):
    """the 8-bit COLOR_RGB2YUV: (..., 3) uint8 -> (Y, U, V) int64 planes"""
    R, G, B = (img[..., k].astype(np.int64) for k in range(3))
    Y = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14
    U = _sat(((B - Y) * 8061 + (128 << 14) + 8192) >> 14)
    V = _sat(((R - Y) * 14369 + (128 << 14) + 8192) >> 14)
    return Y, U, V


def yuv2rgb(Y, U, V):
    """the 8-bit COLOR_YUV2RGB: int64 planes -> (..., 3) uint8"""
    u, v = U - 128, V - 128
    B = _sat(Y + ((u * 33292 + 8192) >> 14))
    G = _sat(Y + ((u * -6472 + v * -9519 + 8192) >> 14))
    R = _sat(Y + ((v * 18678 + 8192) >> 14))
    return np.stack([R, G, B], axis=-1).astype(np.uint8)


def _rint_sat(x):
    """cvRound (half to even) of a float32 and saturate_cast<uchar>"""
    return int(min(max(np.rint(F32(x)), 0), 255))


def equalize_lut(plane):
    """the 256-entry table of cv2.equalizeHist for one uint8 plane (identity for a constant plane)"""
    hist = np.bincount(np.asarray(plane).ravel().astype(np.int64), minlength=256)
    total = int(hist.sum())
    i0 = 0
    while hist[i0] == 0:
        i0 += 1
    if hist[i0] == total:
        return np.arange(256, dtype=np.uint8)
    scale = F32(255.0) / F32(total - int(hist[i0]))
    lut = np.zeros(256, np.uint8)
    s = 0
    for i in range(i0 + 1, 256):
        s += int(hist[i])
        lut[i] = _rint_sat(F32(s) * scale)
    return lut


def equalize_hist(plane):
    return equalize_lut(plane)[np.asarray(plane)]


def equalize_luma_u8(img):
    """(H, W, 3) or (N, H, W, 3) uint8 -> the same shape, each image with its own histogram"""
    img = np.asarray(img)
    if img.ndim == 3:
        return equalize_luma_u8(img[None])[0]
    out = np.empty_like(img)
    for n in range(img.shape[0]):
        Y, U, V = rgb2yuv(img[n])
        out[n] = yuv2rgb(equalize_lut(Y.astype(np.uint8)).astype(np.int64)[Y], U, V)
    return out


def display_finish(y, gamma=1.1):
    return equalize_luma_u8(gamma_u8(y, gamma))


def process_image(y):
    """m_test.py's process_image on ONE (3, H, W) tensor: float64 (H, W, 3) = bytes / 255.0 (the final clip changes nothing)"""
    return display_finish(y)[0].astype(F64) / 255.0
