"""CPU restatement of the end of the reference's ``process_local_style(mode='enhanced')`` (batch_process_images.py:342-352): the
float64 blend with the weight map, ``cv2.convertScaleAbs(result, alpha=1.1, beta=5)`` (``enhance_colors``, :346) and
``smooth_transitions(result, detail_mask, radius=3)`` (``smooth``, :152-174 and :350), written from the definition in
include/mstg_hip.h independently of the kernel (csrc/local_style.hip).

OpenCV is not a dependency of this repository: like tests/local_style_ref.py this module RESTATES OpenCV 4.x -- ``cvtabs`` for
CV_64F -> CV_8U on a build with FMA lanes (narrow to float32, one fused multiply-add, absolute value, round half to even,
saturate), ``dilate`` / ``erode`` with a 5 x 5 box, two iterations, default border, and the bit-exact 8-bit ``GaussianBlur``
(7 x 7, sigma 0, 8.8 fixed point, BORDER_REFLECT_101) -- and HAS NOT BEEN COMPARED WITH AN OPENCV BINARY.
tests/test_local_style_finish_cpu.py pins it with closed forms instead.  ``smooth`` without ``enhance_colors`` is not restated:
there ``GaussianBlur`` runs on the float64 blend and OpenCV's summation order decides bytes.
"""
import numpy as np
from scipy.ndimage import correlate1d, maximum_filter, minimum_filter

import local_style_ref as LR
from oracle import image_ref as IR

TAPS = np.array([8, 28, 56, 72, 56, 28, 8], dtype=np.int64)  # OpenCV's sigma <= 0 table for size 7, times 256
ALPHA32 = np.float32(1.1)


def blend_f64(orig, styled, weight):
    """orig * (1 - w) + styled * w as numpy evaluates it on uint8 (..., H, W, 3) arrays and a float64 (..., H, W) weight"""
    w = np.asarray(weight, dtype=np.float64)[..., np.newaxis]
    return orig * (1 - w) + styled * w


def enhance_u8(x):
    """sat_u8(rint_half_even(|fmaf(float32(x), 1.1f, 5.0f)|)): the fused multiply-add is emulated in float64, where the product
    of two float32 values is exact and so is its sum with 5.0 for every blend value this repository forms (x == 0 or
    |x| >= 1 / 16: at most 53 bits), so the one rounding to float32 is the rounding of the fused operation"""
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    t = (f.astype(np.float64) * np.float64(ALPHA32) + 5.0).astype(np.float32)
    return np.clip(np.rint(np.abs(t)), 0, 255).astype(np.uint8)


def enhance_u8_float64(x):
    """plain float64 evaluation, rint(|x * 1.1 + 5|): NOT the definition; what differs from it is measured in the CPU test"""
    return np.clip(np.rint(np.abs(np.asarray(x, dtype=np.float64) * 1.1 + 5.0)), 0, 255).astype(np.uint8)


def enhance_u8_unfused(x):
    """float32 with a rounded product and a rounded sum: NOT the definition either"""
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    return np.clip(np.rint(np.abs(f * ALPHA32 + np.float32(5.0))), 0, 255).astype(np.uint8)


def boundary(detail):
    """dilate != erode of the (H, W) mask over the 9 x 9 window clipped to the image: outside the image a pixel is neutral, 0 for
    the maximum and 1 for the minimum"""
    d = np.asarray(detail).astype(np.uint8)
    return maximum_filter(d, size=9, mode="constant", cval=0) != minimum_filter(d, size=9, mode="constant", cval=1)


def blur7(e):
    """cv2.GaussianBlur(e, (7, 7), 0) of a uint8 (H, W) or (H, W, C) array in 8.8 fixed point: along x, then along y, scipy's
    'mirror' = BORDER_REFLECT_101 (a length of 1 mirrors onto itself)"""
    v = np.asarray(e).astype(np.int64)
    h = correlate1d(v, TAPS, axis=1, mode="mirror")
    assert h.max(initial=0) <= 65280
    s = correlate1d(h, TAPS, axis=0, mode="mirror")
    return ((s + 32768) >> 16).astype(np.uint8)


def finish(orig, styled, weight, detail, enhance=True, smooth=True):
    """(H, W, 3) uint8 x 2, float64 (H, W), mask (H, W) -> uint8 (H, W, 3)"""
    if smooth and not enhance:
        raise NotImplementedError("smooth without enhance_colors is not restated")
    x = blend_f64(orig, styled, weight)
    if not enhance:
        return np.clip(x, 0, 255).astype(np.uint8)
    e = enhance_u8(x)
    if not smooth:
        return e
    out = e.copy()
    b = boundary(detail)
    out[b] = ((e[b].astype(np.int32) + blur7(e)[b].astype(np.int32)) >> 1).astype(np.uint8)
    return out


def enhanced_ref(canvas, styled, strength=0.8, detail=0.7, detail_coeff=0.3, enhance=True, smooth=True):
    """mode 'enhanced' from the canvas: tests/local_style_ref.py's map and detail mask, then ``finish``"""
    m = LR.enhanced_weight_map(canvas, strength, detail, detail_coeff)
    return finish(canvas, styled, m["weight"], m["detail"], enhance, smooth), m


def process_local_style_enhanced_ref(model_fn, img, strength=0.8, detail=0.7, detail_coeff=0.3, enhance=True, smooth=True, target=256,
                                     resize=IR.pil_resize):
    """process_local_style(mode='enhanced') (batch_process_images.py:255-441) without file I/O, composed from the public pieces of
    oracle/image_ref.py (letterbox geometry as in its process_local_style_ref), tests/local_style_ref.py and ``finish``;
    returns (image, the map dict)"""
    height, width = img.shape[:2]
    if width > height:
        new_width, new_height = target, int(height * (target / width))
    else:
        new_height, new_width = target, int(width * (target / height))
    canvas = np.full((target, target, 3), 255, dtype=np.uint8)
    off_x, off_y = (target - new_width) // 2, (target - new_height) // 2
    canvas[off_y:off_y + new_height, off_x:off_x + new_width] = resize(img, (new_width, new_height), IR.LANCZOS)
    styled = IR.output_to_u8(np.asarray(model_fn(IR.to_tensor_normalize(canvas)[None]))[0])
    out, m = enhanced_ref(canvas, styled, strength, detail, detail_coeff, enhance, smooth)
    aspect = width / height
    if aspect != 1.0:
        if aspect > 1:
            crop_w, crop_h = target, int(target / aspect)
        else:
            crop_h, crop_w = target, int(target * aspect)
        crop_w, crop_h = min(crop_w, target), min(crop_h, target)
        left, top = (target - crop_w) // 2, (target - crop_h) // 2
        out = out[top:top + crop_h, left:left + crop_w]
    if width * height <= 1024 * 1024:
        out = resize(np.ascontiguousarray(out), (width, height), IR.LANCZOS)
    return out, m
