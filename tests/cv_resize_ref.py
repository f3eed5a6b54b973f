"""CPU restatement of ``cv2.resize(src, (Wd, Hd))`` for 8-bit images (INTER_LINEAR), written from the definition in
include/mstg_hip.h ("Mixed-size image comparison") and independent of csrc/compare.hip.  OpenCV is not a dependency of this
repository and the restatement has NOT been compared with an OpenCV binary; tests/test_compare_cpu.py pins it with closed forms
(identity at equal size, the exact 2x reduction, constant images, ``w0 + w1 == 2048``).
"""
import numpy as np


def coeffs(s, d, horizontal):
    """(index int32 [d], weights int16 [d, 2]) of one axis: source extent ``s``, destination extent ``d``"""
    assert s >= 1 and d >= 1
    scale = 1.0 / (float(d) / float(s))                                   # both divisions in double
    i = np.arange(d, dtype=np.float64)
    f = ((i + 0.5) * scale - 0.5).astype(np.float32)                       # double arithmetic, one rounding to float
    p = np.floor(f)
    f = (f - p.astype(np.float32)).astype(np.float32)                      # a float subtraction
    p = p.astype(np.int64)
    if horizontal:
        low, high = p < 0, p >= s - 1
        p = np.where(low, 0, np.where(high, s - 1, p))
        f = np.where(low | high, np.float32(0), f).astype(np.float32)
    one, k = np.float32(1), np.float32(2048)
    w0 = np.rint(((one - f).astype(np.float32) * k).astype(np.float32))    # float operations, each rounded; rint: ties to even
    w1 = np.rint((f * k).astype(np.float32))
    w = np.clip(np.stack([w0, w1], axis=1), -32768, 32767).astype(np.int16)
    return p.astype(np.int32), w


def resize_wide(img, size):
    """the value BEFORE the byte cast, int64 (Hd, Wd, C); ``size`` = (width, height) as cv2.resize takes it"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    hs, ws = img.shape[:2]
    wd, hd = int(size[0]), int(size[1])
    px, wx = coeffs(ws, wd, True)
    py, wy = coeffs(hs, hd, False)
    qx = np.minimum(px + 1, ws - 1)
    src = img.astype(np.int64)
    t = src[:, px] * wx[:, 0].astype(np.int64)[None, :, None] + src[:, qx] * wx[:, 1].astype(np.int64)[None, :, None]  # horizontal pass
    r0, r1 = np.clip(py, 0, hs - 1), np.clip(py + 1, 0, hs - 1)             # rows clamped, weights from the unclamped fraction
    b0, b1 = wy[:, 0].astype(np.int64)[:, None, None], wy[:, 1].astype(np.int64)[:, None, None]
    return (((b0 * (t[r0] >> 4)) >> 16) + ((b1 * (t[r1] >> 4)) >> 16) + 2) >> 2


def resize(img, size):
    """uint8 (Hd, Wd, C): the cast keeps the low 8 bits, as C's (uchar) of an int does"""
    return (resize_wide(img, size) & 0xff).astype(np.uint8)
