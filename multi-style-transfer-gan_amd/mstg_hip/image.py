"""Device-side image pipeline around the generator: what PIL / torchvision / numpy do on the CPU in the
reference's dataset (pretrain.py:20-57) and in ``process_cyclegan`` (batch_process_images.py:176-245), on uint8 HWC tensors that
live on the GPU.  Resampling is Pillow's algorithm bit for bit (csrc/image.hip); decoding / encoding image FILES stays with PIL on
the host -- this module starts from and ends with uint8 arrays.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .ops import _p, _stream

BILINEAR, LANCZOS = 0, 1


@lru_cache(maxsize=256)
def _coeff_tables_host(in_size: int, out_size: int, filt: int):
    lib = _lib.load()
    ks = lib.mstg_resample_ksize(in_size, out_size, filt)
    if ks <= 0:
        raise RuntimeError(f"mstg_hip resample: bad sizes {in_size} -> {out_size}")
    kk = np.zeros((out_size, ks), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    _lib.check(lib.mstg_resample_coeffs(in_size, out_size, filt, kk.ctypes.data, bounds.ctypes.data), "mstg_resample_coeffs")
    return ks, kk, bounds


_dev_tables = {}


def _coeff_tables(in_size, out_size, filt, device):
    key = (in_size, out_size, filt, str(device))
    if key not in _dev_tables:
        ks, kk, bounds = _coeff_tables_host(in_size, out_size, filt)
        _dev_tables[key] = (ks, torch.from_numpy(kk).to(device), torch.from_numpy(bounds).to(device), bounds)
    return _dev_tables[key]


def _req_u8(img: torch.Tensor) -> torch.Tensor:
    if not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise RuntimeError("mstg_hip image: expected a uint8 (H, W, 3) tensor on the GPU")
    return img.contiguous()


def resize_u8(img: torch.Tensor, size, filt: int = BILINEAR) -> torch.Tensor:
    """``PIL.Image.resize((w, h), filter)`` of an (H, W, 3) uint8 image; ``size`` = (new_w, new_h) like PIL."""
    img = _req_u8(img)
    H, W = img.shape[:2]
    new_w, new_h = int(size[0]), int(size[1])
    lib = _lib.load()
    need_h, need_v = new_w != W, new_h != H
    if not need_h and not need_v:
        return img.clone()
    cur, y_first = img, 0
    if need_v:
        ksv, kkv, bv_dev, bv_host = _coeff_tables(H, new_h, filt, img.device)
        y_first = int(bv_host[0, 0])
        y_last = int(bv_host[new_h - 1, 0] + bv_host[new_h - 1, 1])
    else:
        y_last = H
    if need_h:
        ksh, kkh, bh_dev, _ = _coeff_tables(W, new_w, filt, img.device)
        rows = y_last - y_first if need_v else H
        tmp = torch.empty((rows, new_w, 3), dtype=torch.uint8, device=img.device)
        _lib.check(lib.mstg_resample_h_u8(_p(cur), _p(tmp), W, y_first if need_v else 0, rows, new_w, ksh, _p(kkh), _p(bh_dev), _stream()),
                   "mstg_resample_h_u8")
        cur = tmp
    if need_v:
        bounds = bv_dev
        if need_h and y_first:  # Pillow shifts the vertical bounds by the first row the horizontal pass kept
            bounds = bv_dev.clone()
            bounds[:, 0] -= y_first
        out = torch.empty((new_h, cur.shape[1], 3), dtype=torch.uint8, device=img.device)
        _lib.check(lib.mstg_resample_v_u8(_p(cur), _p(out), cur.shape[1], new_h, ksv, _p(kkv), _p(bounds), _stream()), "mstg_resample_v_u8")
        cur = out
    return cur


@lru_cache(maxsize=1024)
def _cv_table_host(src: int, dst: int, horizontal: bool) -> np.ndarray:
    """The device table of one axis of ``cv_resize_u8`` (include/mstg_hip.h): int32 [2 dst] = the index of each destination
    position, then its int16 weight pair as one int32.  Built by the host-only ``mstg_cv_resize_coeffs``."""
    index, weights = np.zeros(max(dst, 0), dtype=np.int32), np.zeros((max(dst, 0), 2), dtype=np.int16)
    _lib.check(_lib.load().mstg_cv_resize_coeffs(src, dst, int(horizontal), index.ctypes.data, weights.ctypes.data), "mstg_cv_resize_coeffs")
    return np.concatenate([index, weights.view(np.int32).reshape(-1)])


def cv_resize_u8(img: torch.Tensor, size) -> torch.Tensor:
    """``cv2.resize(img, (width, height))`` of 8-bit images, i.e. INTER_LINEAR, as the reference's folder comparisons call it
    (compare_image_quality.py:102, complete_comparison.py:17): ``size`` = (new_w, new_h) as ``resize_u8`` takes it, ``img`` an
    (H, W, 3) or (N, H, W, 3) uint8 tensor on the GPU; one launch for the whole batch.  This build's restatement of OpenCV's
    arithmetic (include/mstg_hip.h), not compared with an OpenCV binary -- and not Pillow's resampling, which ``resize_u8`` is.
    The coefficient tables are built on the host and cached on the device per (source extent, destination extent, axis)."""
    if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise RuntimeError("mstg_hip image: cv_resize_u8 expects a uint8 (H, W, 3) or (N, H, W, 3) tensor on the GPU")
    x = img.contiguous()
    batch = x if x.dim() == 4 else x.unsqueeze(0)
    N, H, W = batch.shape[:3]
    new_w, new_h = int(size[0]), int(size[1])
    if min(N, H, W, new_w, new_h) < 1:
        raise RuntimeError(f"mstg_hip image: cv_resize_u8 of {N} image(s) {H} x {W} to {new_h} x {new_w}: every extent must be at least 1")
    tv = _device_table(("cv_resize", H, new_h, 0), x.device, lambda: _cv_table_host(H, new_h, False))
    th = _device_table(("cv_resize", W, new_w, 1), x.device, lambda: _cv_table_host(W, new_w, True))
    out = torch.empty((N, new_h, new_w, 3), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().mstg_cv_resize_linear_u8(_p(batch), N, H, W, new_h, new_w, _p(tv), _p(th), _p(out), _stream()),
               "mstg_cv_resize_linear_u8")
    return out if x.dim() == 4 else out[0]


def paste_u8(src, window, dst_hw, at, fill=255) -> torch.Tensor:
    """New (dh, dw) canvas filled with ``fill`` with ``src[window]`` pasted at ``at`` = (y, x); window = (y0, x0, h, w)."""
    src = _req_u8(src)
    y0, x0, h, w = window
    dst = torch.empty((dst_hw[0], dst_hw[1], 3), dtype=torch.uint8, device=src.device)
    _lib.check(_lib.load().mstg_paste_u8(_p(src), src.shape[0], src.shape[1], y0, x0, h, w, _p(dst), dst_hw[0], dst_hw[1], at[0], at[1],
                                         fill, _stream()), "mstg_paste_u8")
    return dst


def crop_u8(src, left, top, right, bottom) -> torch.Tensor:
    """``Image.crop((left, top, right, bottom))`` for a box inside the image."""
    return paste_u8(src, (top, left, bottom - top, right - left), (bottom - top, right - left), (0, 0), fill=0)


def to_tensor(img, window=None, grid_mask=None):
    """ToTensor + Normalize(0.5, 0.5) -> (3, H, W) fp32 in [-1, 1].  With ``grid_mask`` (64-bit int, bit i*8+j = keep cell (i, j))
    returns (masked_image, image, mask) like MonetPhotoDataset.__getitem__ (pretrain.py:56-57)."""
    img = _req_u8(img)
    y0, x0, H, W = window if window is not None else (0, 0, img.shape[0], img.shape[1])
    out = torch.empty((3, H, W), dtype=torch.float32, device=img.device)
    lib = _lib.load()
    if grid_mask is None:
        _lib.check(lib.mstg_u8_to_tensor(_p(img), img.shape[0], img.shape[1], y0, x0, H, W, _p(out), None, None, 0, 0, _stream()),
                   "mstg_u8_to_tensor")
        return out
    image, mask = torch.empty_like(out), torch.empty_like(out)
    _lib.check(lib.mstg_u8_to_tensor(_p(img), img.shape[0], img.shape[1], y0, x0, H, W, _p(out), _p(image), _p(mask),
                                     int(grid_mask) & (2 ** 64 - 1), 1, _stream()), "mstg_u8_to_tensor")
    return out, image, mask


def to_u8(y: torch.Tensor) -> torch.Tensor:
    """(3, H, W) generator output -> (H, W, 3) uint8: (y + 1) / 2, clamp, * 255, astype(uint8) (batch_process_images.py:213-217)."""
    if not y.is_cuda or y.dim() != 3 or y.shape[0] != 3:
        raise RuntimeError("mstg_hip image: expected a (3, H, W) tensor on the GPU")
    y = y.float().contiguous()
    out = torch.empty((y.shape[1], y.shape[2], 3), dtype=torch.uint8, device=y.device)
    _lib.check(_lib.load().mstg_tensor_to_u8(_p(y), y.shape[1], y.shape[2], _p(out), _stream()), "mstg_tensor_to_u8")
    return out


def blend_u8(orig: torch.Tensor, styled: torch.Tensor, strength=None, weight_map=None) -> torch.Tensor:
    """``np.clip(orig * (1 - w) + styled * w, 0, 255).astype(np.uint8)`` on two (H, W, 3) uint8 images, bit for bit as numpy
    evaluates it in float64: w = the scalar ``strength`` (process_local_style mode 'simple', batch_process_images.py:304-312) or a
    float64 (H, W) ``weight_map`` (the 'enhanced' / 'advanced' blend of :340-342, :386-387; ``enhanced_weight_map`` builds the
    'enhanced' map on the device)."""
    orig, styled = _req_u8(orig), _req_u8(styled)
    if orig.shape != styled.shape:
        raise RuntimeError(f"mstg_hip blend: shapes differ {tuple(orig.shape)} vs {tuple(styled.shape)}")
    if (strength is None) == (weight_map is None):
        raise RuntimeError("mstg_hip blend: give either strength or weight_map")
    H, W = orig.shape[:2]
    out = torch.empty_like(orig)
    if weight_map is not None:
        wm = torch.as_tensor(weight_map)
        if tuple(wm.shape) != (H, W):
            raise RuntimeError(f"mstg_hip blend: weight map {tuple(wm.shape)} does not match the image {H}x{W}")
        wm = wm.to(device=orig.device, dtype=torch.float64).contiguous()
        w0 = w1 = 0.0
    else:
        wm, w1 = None, float(strength)
        w0 = 1 - w1  # Python's double subtraction, as in the reference's expression
    _lib.check(_lib.load().mstg_blend_u8(_p(orig), _p(styled), w0, w1, _p(wm), _p(out), H, W, _stream()), "mstg_blend_u8")
    return out


def local_style_weights(strength, detail, detail_coeff=0.3):
    """(w_base, w_sky, w_detail) in Python's own doubles, as the reference forms them (batch_process_images.py:330, :334, :337;
    ``detail_coeff`` is 0.3 in mode 'enhanced' and 0.4 in mode 'advanced', :383)."""
    return float(strength), min(strength + 0.2, 1.0), max(strength - detail_coeff * detail, 0.0)


def enhanced_weight_map(canvas_u8: torch.Tensor, strength=0.8, detail=0.7, detail_coeff=0.3, return_masks=False):
    """The float64 weight map of ``process_local_style(mode='enhanced', enhance_colors=False, smooth=False)``
    (batch_process_images.py:312-338) of an (H, W, 3) or (N, H, W, 3) uint8 canvas on the GPU, built there in three launches
    whatever N (csrc/local_style.hip): ``detect_sky``'s HSV mask and its 70 % rule, ``cv2.Canny(gray, 50, 150)``,
    ``scipy.ndimage.gaussian_filter(edges, sigma=2) > 0.1`` and the three weight levels; H * W <= 147456 per image.  OpenCV's
    integer steps are restated from their definitions (include/mstg_hip.h), not compared with an OpenCV binary.  Returns the
    (H, W) / (N, H, W) map; with ``return_masks`` also the sky, edge and detail masks (bool) and the ``has_sky`` flag(s), all on
    the device.  ``local_style_finish`` applies the map with the mode's ``enhance_colors`` and ``smooth`` steps; not built:
    ``smooth`` without ``enhance_colors``, mode 'advanced', and a comparison with an OpenCV binary."""
    single = canvas_u8.dim() == 3
    c = canvas_u8.unsqueeze(0) if single else canvas_u8
    if not c.is_cuda or c.dtype != torch.uint8 or c.dim() != 4 or c.shape[3] != 3 or c.shape[0] < 1:
        raise RuntimeError("mstg_hip image: expected a uint8 (H, W, 3) or (N, H, W, 3) canvas on the GPU")
    c = c.contiguous()
    N, H, W = c.shape[:3]
    w_base, w_sky, w_detail = local_style_weights(strength, detail, detail_coeff)
    lib = _lib.load()
    wm = torch.empty((N, H, W), dtype=torch.float64, device=c.device)
    if not return_masks:
        need = lib.mstg_local_style_workspace_bytes(N, H, W)  # 0: the call below names what is wrong with the shape
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=c.device)
        _lib.check(lib.mstg_local_style_weight_map(_p(c), N, H, W, w_base, w_sky, w_detail, _p(wm), _p(ws), need, _stream()),
                   "mstg_local_style_weight_map")
        return wm[0] if single else wm
    state, sky, edge, det = (torch.empty((N, H, W), dtype=torch.uint8, device=c.device) for _ in range(4))
    count = torch.empty(N, dtype=torch.int32, device=c.device)
    _lib.check(lib.mstg_local_style_prepare(_p(c), N, H, W, _p(state), _p(sky), _p(count), None, _stream()), "mstg_local_style_prepare")
    _lib.check(lib.mstg_local_style_hysteresis(_p(state), N, H, W, _p(edge), _stream()), "mstg_local_style_hysteresis")
    _lib.check(lib.mstg_local_style_weights(_p(edge), _p(sky), _p(count), N, H, W, w_base, w_sky, w_detail, _p(wm), _p(det), _stream()),
               "mstg_local_style_weights")
    # count / (H * W) > 0.7 in doubles, as the kernel and the reference evaluate it, is 10 * count > 7 * H * W: the quotient of an
    # exact 7 / 10 rounds to the double 0.7 itself, and the next possible ratio lies 1 / (10 H W) above it, far more than an ulp.
    # (A torch division by a Python scalar multiplies by the reciprocal on the device and calls 7000 / 10000 greater than 0.7.)
    has_sky = count.long() * 10 > 7 * H * W
    out = (wm, sky.view(torch.bool), edge.view(torch.bool), det.view(torch.bool), has_sky)
    return tuple(t[0] for t in out) if single else out


def _req_canvases(t, what):
    if not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or t.shape[0] < 1:
        raise RuntimeError(f"mstg_hip image: expected a uint8 (H, W, 3) or (N, H, W, 3) {what} on the GPU")
    return t.contiguous()


def local_style_finish(canvas_u8, styled_u8, weight_map, detail_mask, enhance_colors=True, smooth=True) -> torch.Tensor:
    """The end of ``process_local_style(mode='enhanced')`` (batch_process_images.py:342-352) for an (H, W, 3) or (N, H, W, 3)
    uint8 canvas and styled image, the float64 ``weight_map`` and the ``detail_mask`` (bool or 0 / 1 bytes; may be None without
    ``smooth``) of ``enhanced_weight_map``, in one launch whatever N: the float64 blend of ``blend_u8``, ``enhance_colors`` =
    ``cv2.convertScaleAbs(alpha=1.1, beta=5)`` and ``smooth`` = ``smooth_transitions(radius=3)``, restated from their
    definitions (include/mstg_hip.h; not compared with an OpenCV binary).  Both flags off equals ``blend_u8`` byte for byte;
    ``smooth`` without ``enhance_colors`` is not built and raises."""
    single = canvas_u8.dim() == 3
    c = _req_canvases(canvas_u8.unsqueeze(0) if single else canvas_u8, "canvas")
    st = _req_canvases(styled_u8.unsqueeze(0) if single else styled_u8, "styled image")
    if c.shape != st.shape:
        raise RuntimeError(f"mstg_hip local style: shapes differ {tuple(c.shape)} vs {tuple(st.shape)}")
    N, H, W = c.shape[:3]
    wm = torch.as_tensor(weight_map).to(device=c.device, dtype=torch.float64)
    if single:
        wm = wm.unsqueeze(0)
    if tuple(wm.shape) != (N, H, W):
        raise RuntimeError(f"mstg_hip local style: weight map {tuple(wm.shape)} does not match the canvases {(N, H, W)}")
    wm = wm.contiguous()
    det = None
    if detail_mask is not None:
        det = torch.as_tensor(detail_mask).to(device=c.device)
        if det.numel() != N * H * W:
            raise RuntimeError(f"mstg_hip local style: detail mask {tuple(det.shape)} does not match the canvases {(N, H, W)}")
        det = (det if det.dtype == torch.uint8 else det.to(torch.uint8)).contiguous()
    out = torch.empty_like(c)
    _lib.check(_lib.load().mstg_local_style_finish(_p(c), _p(st), _p(wm), _p(det), N, H, W, int(bool(enhance_colors)), int(bool(smooth)),
                                                   _p(out), _stream()), "mstg_local_style_finish")
    return out[0] if single else out


def _local_style_enhanced(canvas, styled, strength, detail, detail_coeff, enhance_colors, smooth, out=None):
    """mode 'enhanced' for (N, H, W, 3) canvases that are already checked: four launches on one workspace"""
    N, H, W = canvas.shape[:3]
    w_base, w_sky, w_detail = local_style_weights(strength, detail, detail_coeff)
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(canvas)
    need = lib.mstg_local_style_enhanced_workspace_bytes(N, H, W)  # 0: the call below names what is wrong with the shape
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=canvas.device)
    _lib.check(lib.mstg_local_style_enhanced(_p(canvas), _p(styled), N, H, W, w_base, w_sky, w_detail, int(bool(enhance_colors)),
                                             int(bool(smooth)), _p(out), _p(ws), need, _stream()), "mstg_local_style_enhanced")
    return out


# ---- the standard mode's finish (csrc/standard_mode.hip) -------------------------------------------------------------------
_std_tables = {}


def _device_table(key, device, build):
    """what ``build()`` returns, with its numpy table on ``device``: built on the host and uploaded once per ``key`` and device.
    ``build`` returns the table, or (value, table) where a value goes with it."""
    key = key + (str(device),)
    if key not in _std_tables:
        built = build()
        if isinstance(built, tuple):
            _std_tables[key] = (built[0], torch.from_numpy(built[1]).to(device))
        else:
            _std_tables[key] = torch.from_numpy(built).to(device)
    return _std_tables[key]


def _host_fill(entry, size, dtype, *args, counts=False):
    """(return value, table): ``size`` zeros of ``dtype`` filled by the host-only C entry ``entry(*args, pointer)``.  An error code
    raises; with ``counts`` the entry returns a positive count, and 0 is an error as well."""
    table = np.zeros(size, dtype=dtype)
    rc = getattr(_lib.load(), entry)(*args, table.ctypes.data)
    if rc <= 0 or not counts:
        _lib.check((rc or -1) if counts else rc, entry)
    return rc, table


def _bilateral_table(d, sigma_color, sigma_space, device):
    """the host-built weight tables of ``mstg_bilateral_tables`` on ``device`` (built and uploaded once per parameter set)"""
    args, size = (int(d), float(sigma_color), float(sigma_space)), _lib.BILATERAL_COLOR_WEIGHTS + _lib.BILATERAL_MAX_TAPS
    return _device_table(("bilateral",) + args, device,
                         lambda: _host_fill("mstg_bilateral_tables", size, np.float32, *args, counts=True)[1])


def _standard_model_type(model_type):
    if model_type not in _lib.STANDARD_MODEL_TYPES:
        raise ValueError(f"mstg_hip image: model_type {model_type!r} is neither 'photo_to_monet' nor 'monet_to_photo'")
    return _lib.STANDARD_MODEL_TYPES[model_type]


def _color_lut(model_type, device):
    """the colour step's three 256-entry tables of ``mstg_standard_color_lut`` on ``device``"""
    mt = _standard_model_type(model_type)
    return _device_table(("lut", mt), device, lambda: _host_fill("mstg_standard_color_lut", 768, np.uint8, mt)[1])


def _stage_u8(img, what):
    single = img.dim() == 3
    return single, _req_canvases(img.unsqueeze(0) if single else img, what)


def median3_u8(img: torch.Tensor) -> torch.Tensor:
    """``cv2.medianBlur(img, 3)`` of an (H, W, 3) or (N, H, W, 3) uint8 image on the GPU (gan_login_gui.py:835): per channel the
    median of the 3 x 3 window with replicated borders, one launch whatever N.  Restated from the definition
    (include/mstg_hip.h), not compared with an OpenCV binary."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    out = torch.empty_like(x)
    _lib.check(_lib.load().mstg_median3_u8(_p(x), N, H, W, _p(out), _stream()), "mstg_median3_u8")
    return out[0] if single else out


def bilateral_u8(img: torch.Tensor, d=9, sigma_color=75, sigma_space=75) -> torch.Tensor:
    """``cv2.bilateralFilter(img, d, sigma_color, sigma_space)`` of an (H, W, 3) or (N, H, W, 3) uint8 image on the GPU
    (gan_login_gui.py:838, :1423, :2560): OpenCV 4.x's 8-bit three-channel filter as include/mstg_hip.h defines it (float32 in tap
    order, fused channel sums, one reciprocal, BORDER_REFLECT_101; the weight tables are built on the host), one launch whatever
    N.  ``d`` must be 3, 5, 7 or 9; anything else raises, naming d.  Not compared with an OpenCV binary."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    table = _bilateral_table(d, sigma_color, sigma_space, x.device)
    out = torch.empty_like(x)
    _lib.check(_lib.load().mstg_bilateral_u8(_p(x), N, H, W, int(d), _p(table), _p(out), _stream()), "mstg_bilateral_u8")
    return out[0] if single else out


def gaussian_u8(img: torch.Tensor, ksize) -> torch.Tensor:
    """``cv2.GaussianBlur(img, (ksize, ksize), 0)`` of an (H, W, 3) or (N, H, W, 3) uint8 image on the GPU (gan_login_gui.py:865)
    in OpenCV's bit-exact 8.8 fixed point, for ksize 3, 5 and 7; 9 to 15 (smooth_level 4 to 7) raise, naming the level: their
    taps are not restated and the blur is never approximated.  Not compared with an OpenCV binary."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    out = torch.empty_like(x)
    _lib.check(_lib.load().mstg_gaussian_u8(_p(x), N, H, W, int(ksize), _p(out), _stream()), "mstg_gaussian_u8")
    return out[0] if single else out


def _standard_finish(canvas, styled, model_type, blend_ratio, fix_blocks, enhance_colors, smooth_level, adaptive_smooth, out=None):
    """the standard mode's finish for (N, H, W, 3) batches that are already checked: at most three launches on one workspace"""
    N, H, W = styled.shape[:3]
    lib = _lib.load()
    _standard_model_type(model_type)  # a bad name raises whatever the flags
    lut = _color_lut(model_type, styled.device) if enhance_colors else None
    table = _bilateral_table(9, 75, 75, styled.device) if fix_blocks else None
    level = int(smooth_level) if adaptive_smooth and smooth_level > 0 else 0
    w1 = float(blend_ratio) if blend_ratio > 0 else 0.0
    w0 = 1 - w1  # Python's double subtraction, as in the reference's expression
    if out is None:
        out = torch.empty_like(styled)
    need = lib.mstg_standard_finish_workspace_bytes(N, H, W)  # 0: the call below names what is wrong with the shape
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=styled.device)
    _lib.check(lib.mstg_standard_finish(_p(canvas), _p(styled), N, H, W, w0, w1, int(bool(fix_blocks)), 9, _p(table), _p(lut), level,
                                        _p(out), _p(ws), need, _stream()), "mstg_standard_finish")
    return out


def standard_finish(canvas_u8, styled_u8, model_type, blend_ratio=0.3, fix_blocks=True, enhance_colors=True, smooth_level=3,
                    adaptive_smooth=True) -> torch.Tensor:
    """Everything the standard mode of the reference's application does between the forward pass and the crop
    (gan_login_gui.py:817-868) for an (H, W, 3) or (N, H, W, 3) uint8 canvas and styled image on the GPU, with that tab's options
    and defaults: the ``blend_ratio`` blend with the canvas (0 skips it), ``fix_blocks`` = ``cv2.medianBlur(3)`` then
    ``cv2.bilateralFilter(d=9, 75, 75)``, ``enhance_colors`` = the colour step of ``model_type`` ('photo_to_monet' or
    'monet_to_photo'; anything else raises ValueError), and ``cv2.GaussianBlur`` of size ``2 * smooth_level + 1`` (level 0 or
    ``adaptive_smooth=False`` skips it; levels above 3 raise, naming the level).  At most three launches whatever N, byte for byte
    the composition of ``blend_u8``, ``median3_u8``, ``bilateral_u8``, the table lookup and ``gaussian_u8``.  The OpenCV steps are
    restated from their definitions (include/mstg_hip.h), not compared with an OpenCV binary."""
    _standard_model_type(model_type)
    single, st = _stage_u8(styled_u8, "styled image")
    _, c = _stage_u8(canvas_u8, "canvas")
    if c.shape != st.shape:
        raise RuntimeError(f"mstg_hip standard mode: shapes differ {tuple(c.shape)} vs {tuple(st.shape)}")
    out = _standard_finish(c, st, model_type, blend_ratio, fix_blocks, enhance_colors, smooth_level, adaptive_smooth)
    return out[0] if single else out


_STANDARD = object()  # the mode of the batched pipeline that runs _standard_finish (not reachable through a mode name)


# ---- the callers, restated on the device ----------------------------------------------------------------------------------
def dataset_item(img_u8: torch.Tensor, grid_mask: int, img_size: int = 256):
    """MonetPhotoDataset.__getitem__ (pretrain.py:41-57) from a decoded uint8 image on the GPU: Resize(img_size) (shorter side,
    bilinear) -> CenterCrop -> ToTensor -> Normalize -> 8x8-grid mask.  Returns (masked_image, image, mask)."""
    H, W = img_u8.shape[:2]
    if W <= H:  # torchvision Resize(int): the smaller edge becomes img_size, the other int(size * long / short)
        new_w, new_h = img_size, int(img_size * H / W)
    else:
        new_h, new_w = img_size, int(img_size * W / H)
    r = resize_u8(img_u8, (new_w, new_h), BILINEAR) if (new_w, new_h) != (W, H) else img_u8
    top, left = int(round((new_h - img_size) / 2.0)), int(round((new_w - img_size) / 2.0))  # torchvision center_crop
    return to_tensor(r, (top, left, img_size, img_size), grid_mask)


def letterbox(img_u8: torch.Tensor, target=256):
    """batch_process_images.py:183-199: aspect-preserving LANCZOS resize onto a white target x target canvas -> (canvas, geometry)."""
    height, width = img_u8.shape[:2]
    if width > height:
        new_width, new_height = target, int(height * (target / width))
    else:
        new_height, new_width = target, int(width * (target / height))
    resized = resize_u8(img_u8, (new_width, new_height), LANCZOS)
    off_x, off_y = (target - new_width) // 2, (target - new_height) // 2
    canvas = paste_u8(resized, (0, 0, new_height, new_width), (target, target), (off_y, off_x), fill=255)
    return canvas, (width, height)


def process_cyclegan(model, img_u8: torch.Tensor, target=256) -> torch.Tensor:
    """``process_cyclegan`` of the reference (batch_process_images.py:176-236) without the file I/O: decoded uint8 image in, uint8
    image out, everything in between on the GPU (letterbox, forward, output conversion, crop back, resize back)."""
    canvas, (width, height) = letterbox(img_u8, target)
    x = to_tensor(canvas).unsqueeze(0)
    with torch.no_grad():
        y = model(x)
    out = to_u8(y[0])
    if width != height:
        aspect = width / height
        if aspect > 1:
            crop_w, crop_h = target, int(target / aspect)
        else:
            crop_h, crop_w = target, int(target * aspect)
        left, top = (target - crop_w) // 2, (target - crop_h) // 2
        out = crop_u8(out, left, top, left + crop_w, top + crop_h)
    if width * height <= 1024 * 1024:
        out = resize_u8(out, (width, height), LANCZOS)
    return out


def process_local_style(model, img_u8: torch.Tensor, mode="simple", strength=0.8, weight_map=None, target=256, detail=0.7,
                        detail_coeff=0.3, enhance_colors=True, smooth=True) -> torch.Tensor:
    """``process_local_style`` of the reference (batch_process_images.py:255-441) without the file I/O, on the GPU end to end:
    'simple' (strength blend of the letterboxed original with the styled image, :304-312), 'weight_map' (the per-pixel blend of
    the 'enhanced' mode, :340-342 + :352: with the caller's (target, target) float64 ``weight_map``, or, when it is None, with the
    map ``enhanced_weight_map`` builds from the letterboxed canvas, ``strength``, ``detail`` and ``detail_coeff`` -- the
    reference's mode='enhanced', enhance_colors=False, smooth=False), 'enhanced' (the reference's default mode, :312-353, with
    its keywords ``enhance_colors`` and ``smooth``, both on by default as there: the device map, then ``local_style_finish`` in
    place of the blend, so as many launches as 'weight_map' without a map; ``smooth`` without ``enhance_colors`` is not built and
    raises; the two keywords matter in this mode only), and any other mode name, 'advanced' included = the reference's default
    branch (the styled image itself, :399-401).  Crop back to the aspect ratio and LANCZOS resize back as :403-429."""
    canvas, (width, height) = letterbox(img_u8, target)
    x = to_tensor(canvas).unsqueeze(0)
    with torch.no_grad():
        y = model(x)
    styled = to_u8(y[0])
    if mode == "simple":
        out = blend_u8(canvas, styled, strength=strength)
    elif mode == "weight_map":
        if weight_map is None:
            weight_map = enhanced_weight_map(canvas, strength, detail, detail_coeff)
        out = blend_u8(canvas, styled, weight_map=weight_map)
    elif mode == "enhanced":
        out = _local_style_enhanced(canvas.unsqueeze(0), styled.unsqueeze(0), strength, detail, detail_coeff, enhance_colors, smooth)[0]
    else:
        out = styled
    aspect = width / height
    if aspect != 1.0:
        if aspect > 1:
            crop_w, crop_h = target, int(target / aspect)
        else:
            crop_h, crop_w = target, int(target * aspect)
        crop_w, crop_h = min(crop_w, target), min(crop_h, target)
        left, top = (target - crop_w) // 2, (target - crop_h) // 2
        out = crop_u8(out, left, top, left + crop_w, top + crop_h)
    if width * height <= 1024 * 1024:
        out = resize_u8(out, (width, height), LANCZOS)
    return out


def process_standard(model, img_u8: torch.Tensor, model_type, blend_ratio=0.3, fix_blocks=True, enhance_colors=True, smooth_level=3,
                     adaptive_smooth=True, target=256) -> torch.Tensor:
    """The standard mode of the reference's application (gan_login_gui.py:769-889, standard_process_thread) without the file I/O,
    on the GPU end to end: the letterbox and forward pass of ``process_cyclegan``, ``standard_finish`` with the tab's options (its
    defaults: every step on), then the crop back to the aspect ratio and the LANCZOS resize back of :870-889.  The reference's
    ``strength`` argument is never read there and is not taken."""
    _standard_model_type(model_type)
    canvas, (width, height) = letterbox(img_u8, target)
    x = to_tensor(canvas).unsqueeze(0)
    with torch.no_grad():
        y = model(x)
    styled = to_u8(y[0])
    out = _standard_finish(canvas.unsqueeze(0), styled.unsqueeze(0), model_type, blend_ratio, fix_blocks, enhance_colors, smooth_level,
                           adaptive_smooth)[0]
    if width != height:
        aspect = width / height
        if aspect > 1:
            crop_w, crop_h = target, int(target / aspect)
        else:
            crop_h, crop_w = target, int(target * aspect)
        left, top = (target - crop_w) // 2, (target - crop_h) // 2
        out = crop_u8(out, left, top, left + crop_w, top + crop_h)
    if width * height <= 1024 * 1024:
        out = resize_u8(out, (width, height), LANCZOS)
    return out


# ---- the batched pipeline (csrc/image_batch.hip) ---------------------------------------------------------------------------
# N images of different sizes per call; the number of library launches does not depend on N and every byte equals the one-image
# functions above.  Geometry is planned in pure Python with the expressions of letterbox / process_cyclegan /
# process_local_style / dataset_item, turned into one descriptor per image and direction, and uploaded -- descriptors, tile
# lists and the coefficient tables of the whole chunk -- in one pinned host-to-device copy.
class LetterboxGeom(NamedTuple):
    """Geometry of one image through process_cyclegan / process_local_style: the LANCZOS resize to (new_h, new_w), its offset
    on the canvas, the crop box (left, top, crop_w, crop_h) of the output canvas, whether that crop is resized back, and the
    size of the result."""
    height: int
    width: int
    new_h: int
    new_w: int
    off_y: int
    off_x: int
    crop: tuple
    resize_back: bool
    out_h: int
    out_w: int


class DatasetGeom(NamedTuple):
    """Geometry of one MonetPhotoDataset item: the BILINEAR shorter-side resize to (new_h, new_w) and the centre-crop origin."""
    height: int
    width: int
    new_h: int
    new_w: int
    top: int
    left: int


def _sizes(sizes):
    out = []
    for i, s in enumerate(sizes):
        h, w = int(s[0]), int(s[1])
        if h < 1 or w < 1:
            raise ValueError(f"mstg_hip image: image {i} has size {h}x{w}")
        out.append((h, w))
    return out


@lru_cache(maxsize=4096)
def _letterbox_geom(height, width, target, local_style):
    if width > height:
        new_width, new_height = target, int(height * (target / width))
    else:
        new_height, new_width = target, int(width * (target / height))
    if new_width < 1 or new_height < 1:
        return None
    off_x, off_y = (target - new_width) // 2, (target - new_height) // 2
    crop_w = crop_h = target
    aspect = width / height
    if (aspect != 1.0) if local_style else (width != height):
        if aspect > 1:
            crop_w, crop_h = target, int(target / aspect)
        else:
            crop_h, crop_w = target, int(target * aspect)
        if local_style:
            crop_w, crop_h = min(crop_w, target), min(crop_h, target)
    if crop_w < 1 or crop_h < 1:
        return None
    left, top = (target - crop_w) // 2, (target - crop_h) // 2
    back = width * height <= 1024 * 1024
    return LetterboxGeom(height, width, new_height, new_width, off_y, off_x, (left, top, crop_w, crop_h), back,
                         height if back else crop_h, width if back else crop_w)


def letterbox_plan(sizes, target=256, local_style=False):
    """Geometry of ``process_cyclegan`` (``local_style``: of ``process_local_style``) for images of ``sizes`` = (height, width)
    pairs.  Pure Python.  Raises, naming the image, for a size whose resized or cropped side would be 0 (Pillow refuses it)."""
    target = int(target)
    if target < 1:
        raise ValueError(f"mstg_hip image: target {target}")
    plan = []
    for i, (h, w) in enumerate(_sizes(sizes)):
        g = _letterbox_geom(h, w, target, bool(local_style))
        if g is None:
            raise ValueError(f"mstg_hip image: image {i} ({h}x{w}) would be resized to a side of 0 on a {target} canvas")
        plan.append(g)
    return plan


@lru_cache(maxsize=4096)
def _dataset_geom(H, W, img_size):
    if W <= H:  # torchvision Resize(int): the smaller edge becomes img_size, the other int(size * long / short)
        new_w, new_h = img_size, int(img_size * H / W)
    else:
        new_h, new_w = img_size, int(img_size * W / H)
    top, left = int(round((new_h - img_size) / 2.0)), int(round((new_w - img_size) / 2.0))  # torchvision center_crop
    return DatasetGeom(H, W, new_h, new_w, top, left)


def dataset_plan(sizes, img_size=256):
    """Geometry of ``dataset_item`` for images of ``sizes`` = (height, width) pairs.  Pure Python."""
    img_size = int(img_size)
    if img_size < 1:
        raise ValueError(f"mstg_hip image: img_size {img_size}")
    return [_dataset_geom(h, w, img_size) for h, w in _sizes(sizes)]


_DESC = np.dtype([("src", "<u8")] + [(n, "<i4") for n in (
    "src_h", "src_w", "box_y", "box_x", "box_h", "box_w", "rs_h", "rs_w", "filter", "win_y", "win_x", "win_h", "win_w", "dst_y", "dst_x",
    "fill", "ks_h", "ks_v", "y_first", "irows", "ipitch")] + [(n, "<i8") for n in (
        "kk_h", "bounds_h", "kk_v", "bounds_v", "inter_off", "out_off")] + [("grid", "<u8")], align=True)
assert _DESC.itemsize == C.sizeof(_lib.ImgDesc)


@lru_cache(maxsize=4096)
def _axes(bh, bw, rh, rw, filt, wy, wh):
    """(ks_h, ks_v, y_first, irows): tap counts (0: the pass copies) and the box rows the vertical pass reads for window rows
    [wy, wy + wh) -- what Pillow's horizontal pass computes."""
    ks_h = 0 if rw == bw else _coeff_tables_host(bw, rw, filt)[0]
    if rh == bh:
        return ks_h, 0, wy, wh
    ks_v, _, b = _coeff_tables_host(bh, rh, filt)
    y_first = int(b[wy, 0])
    return ks_h, ks_v, y_first, int(b[wy + wh - 1, 0] + b[wy + wh - 1, 1]) - y_first


class _Direction:
    """Descriptors of one direction (image -> canvas or canvas -> image) of one chunk."""

    def __init__(self, plan, canvas):
        self.plan, self.canvas, self.rows, self.inter_bytes, self.out_bytes, self.out_offs = plan, canvas, [], 0, 0, []

    def add(self, src_ptr, src_h, src_w, box, rs, filt, win, dst=(0, 0), fill=0, grid=0):
        (by, bx, bh, bw), (rh, rw), (wy, wx, wh, ww) = box, rs, win
        ks_h, ks_v, y_first, irows = _axes(bh, bw, rh, rw, filt, wy, wh)
        kk_h, bo_h = self.plan.table(bw, rw, filt) if ks_h else (0, 0)
        kk_v, bo_v = self.plan.table(bh, rh, filt) if ks_v else (0, 0)
        ipitch = (3 * ww + 3) & ~3
        self.rows.append((src_ptr, src_h, src_w, by, bx, bh, bw, rh, rw, filt, wy, wx, wh, ww, dst[0], dst[1], fill, ks_h, ks_v, y_first,
                          irows, ipitch, kk_h, bo_h, kk_v, bo_v, self.inter_bytes, self.out_bytes, grid))
        self.out_offs.append(self.out_bytes)
        self.inter_bytes += irows * ipitch
        self.out_bytes += (3 * wh * ww + 15) & ~15

    def _args(self, k):
        p = self.plan
        return (p.host + self.off_descs, len(self.rows), p.host + p.off_table, p.table_len, p.dev + self.off_descs, p.dev + self.off_tiles[k],
                self.ntiles[k], p.dev + p.off_table)

    def run_h(self, inter):
        _lib.check(_lib.load().mstg_img_batch_resample_h(*self._args(0), _p(inter), inter.numel(), _stream()), "mstg_img_batch_resample_h")

    def run_v_tensor(self, inter, out, image_out=None, mask_out=None, canvas_u8=None, use_mask=0):
        _lib.check(_lib.load().mstg_img_batch_resample_v_tensor(*self._args(1), _p(inter), inter.numel(), self.canvas, _p(out), _p(image_out),
                                                                _p(mask_out), _p(canvas_u8), use_mask, _stream()),
                   "mstg_img_batch_resample_v_tensor")

    def run_v_u8(self, inter, out):
        _lib.check(_lib.load().mstg_img_batch_resample_v_u8(*self._args(1), _p(inter), inter.numel(), _p(out), out.numel(), _stream()),
                   "mstg_img_batch_resample_v_u8")


class _BatchPlan:
    """Everything the kernels of one chunk read besides pixels: descriptors and tile lists per direction, and the coefficient
    tables (each (in, out, filter) once), laid out in one pinned buffer and copied to the device in one transfer."""

    def __init__(self, device):
        self.device, self.dirs, self._parts, self._index, self.table_len = device, [], [], {}, 0

    def direction(self, canvas=0):
        self.dirs.append(_Direction(self, canvas))
        return self.dirs[-1]

    def table(self, in_size, out_size, filt):
        key = (in_size, out_size, filt)
        if key not in self._index:
            _, kk, bounds = _coeff_tables_host(in_size, out_size, filt)
            self._index[key] = (self.table_len, self.table_len + kk.size)
            self._parts += [kk.reshape(-1), bounds.reshape(-1)]
            self.table_len += kk.size + bounds.size
        return self._index[key]

    def upload(self):
        lib = _lib.load()
        table = np.concatenate(self._parts) if self._parts else np.zeros(4, dtype=np.int32)
        self.table_len = int(table.size)
        total = 0

        def take(nbytes):
            nonlocal total
            off, total = total, total + ((nbytes + 15) & ~15)
            return off

        for d in self.dirs:
            d.descs = np.array(d.rows, dtype=_DESC)
            d.passes = (_lib.IMG_PASS_H, _lib.IMG_PASS_V_TENSOR if d.canvas else _lib.IMG_PASS_V_U8)
            d.ntiles = []
            for p in d.passes:
                cnt = lib.mstg_img_batch_tiles(d.descs.ctypes.data, len(d.rows), table.ctypes.data, self.table_len, p,
                                               d.canvas if p == _lib.IMG_PASS_V_TENSOR else 0, None, 0)
                if cnt <= 0:
                    _lib.check(cnt or -1, "mstg_img_batch_tiles")
                d.ntiles.append(cnt)
            d.off_descs = take(d.descs.nbytes)
            d.off_tiles = [take(16 * c) for c in d.ntiles]
        self.off_table = take(table.nbytes)
        self._host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        hb = self._host.numpy()
        self.host = hb.ctypes.data
        hb[self.off_table:self.off_table + table.nbytes] = table.view(np.uint8)
        for d in self.dirs:
            hb[d.off_descs:d.off_descs + d.descs.nbytes] = d.descs.view(np.uint8)
            for p, off, c in zip(d.passes, d.off_tiles, d.ntiles):
                got = lib.mstg_img_batch_tiles(self.host + d.off_descs, len(d.rows), self.host + self.off_table, self.table_len, p,
                                               d.canvas if p == _lib.IMG_PASS_V_TENSOR else 0, self.host + off, c)
                if got != c:
                    _lib.check(got if got < 0 else -1, "mstg_img_batch_tiles")
        self._dev = self._host.to(self.device, non_blocking=True)
        self.dev = self._dev.data_ptr()


def upload_u8(arrays, device=None):
    """Decoded (H, W, 3) uint8 numpy images -> GPU tensors through ONE pinned buffer and ONE host-to-device copy; the results
    are views of one device buffer (each starts on a 16-byte boundary)."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    arrays = [np.ascontiguousarray(a, dtype=np.uint8) for a in arrays]
    offs, total = [], 0
    for i, a in enumerate(arrays):
        if a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
            raise RuntimeError(f"mstg_hip image: image {i} is not a non-empty (H, W, 3) array")
        offs.append(total)
        total += (a.size + 15) & ~15
    host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
    hb = host.numpy()
    for a, o in zip(arrays, offs):
        hb[o:o + a.size] = a.reshape(-1)
    dev = host.to(device, non_blocking=True)
    return [dev[o:o + a.size].view(a.shape) for a, o in zip(arrays, offs)]


def _req_batch(images):
    images = [_req_u8(im) for im in images]
    if any(im.device != images[0].device for im in images):
        raise RuntimeError("mstg_hip image: the images of a batch must live on one device")
    return images


def _process_chunk(model, images, geoms, target, mode, strength, weight_maps, detail, detail_coeff, enhance_colors, smooth, standard=None):
    n, T, dev = len(images), target, images[0].device
    blend = mode in ("simple", "weight_map", "enhanced") or mode is _STANDARD
    plan = _BatchPlan(dev)
    pre, post = plan.direction(canvas=T), plan.direction()
    x = torch.empty((n, 3, T, T), dtype=torch.float32, device=dev)
    styled = torch.empty((n, T, T, 3), dtype=torch.uint8, device=dev)
    canvas = torch.empty_like(styled) if blend else None
    final = torch.empty_like(styled) if blend else styled
    for im, g in zip(images, geoms):
        pre.add(im.data_ptr(), g.height, g.width, (0, 0, g.height, g.width), (g.new_h, g.new_w), LANCZOS, (0, 0, g.new_h, g.new_w),
                (g.off_y, g.off_x), 255)
    for i, g in enumerate(geoms):
        left, top, crop_w, crop_h = g.crop
        post.add(final.data_ptr() + i * T * T * 3, T, T, (top, left, crop_h, crop_w), (g.out_h, g.out_w), LANCZOS, (0, 0, g.out_h, g.out_w))
    plan.upload()
    inter = torch.empty(max(pre.inter_bytes, post.inter_bytes), dtype=torch.uint8, device=dev)
    pre.run_h(inter)
    pre.run_v_tensor(inter, x, canvas_u8=canvas)
    with torch.no_grad():
        y = model(x)
    if not y.is_cuda or tuple(y.shape) != (n, 3, T, T):
        raise RuntimeError(f"mstg_hip image: the model returned {tuple(y.shape)} for an input of {tuple(x.shape)}")
    if y.dtype not in (torch.float32, torch.float16):
        y = y.float()
    y = y.contiguous()
    lib = _lib.load()
    _lib.check(lib.mstg_img_batch_tensor_to_u8(_p(y), int(y.dtype == torch.float16), n, T, T, _p(styled), _stream()),
               "mstg_img_batch_tensor_to_u8")
    if mode is _STANDARD:  # the standard mode's finish on the canvas batch the chunk already has: at most three launches
        _standard_finish(canvas, styled, out=final, **standard)
    elif mode == "enhanced":  # stages A-C and the finish on the canvas batch the chunk already has: four launches
        _local_style_enhanced(canvas, styled, strength, detail, detail_coeff, enhance_colors, smooth, out=final)
    elif blend:  # the (n * T, T, 3) view of the batch is one tall image to the blend kernel
        if mode == "weight_map":
            if weight_maps is None:  # three launches on the canvas batch the chunk already has
                wm = enhanced_weight_map(canvas, strength, detail, detail_coeff)
            else:
                wm = torch.stack([torch.as_tensor(m) for m in weight_maps]).to(device=dev, dtype=torch.float64).contiguous()
            w0 = w1 = 0.0
        else:
            wm, w1 = None, float(strength)
            w0 = 1 - w1
        _lib.check(lib.mstg_blend_u8(_p(canvas), _p(styled), w0, w1, _p(wm), _p(final), n * T, T, _stream()), "mstg_blend_u8")
    out = torch.empty(post.out_bytes, dtype=torch.uint8, device=dev)
    post.run_h(inter)
    post.run_v_u8(inter, out)
    return [out[o:o + g.out_h * g.out_w * 3].view(g.out_h, g.out_w, 3) for o, g in zip(post.out_offs, geoms)]


def _process_batch(model, images, target, batch_size, mode, strength, weight_maps, local_style, detail=0.7, detail_coeff=0.3,
                   enhance_colors=True, smooth=True, standard=None):
    images = _req_batch(images)
    target, batch_size = int(target), int(batch_size)
    if batch_size < 1:
        raise RuntimeError(f"mstg_hip image: batch_size {batch_size}")
    geoms = letterbox_plan([im.shape[:2] for im in images], target, local_style=local_style)
    device_map = mode == "enhanced" or (mode == "weight_map" and weight_maps is None)
    if device_map and target * target > _lib.LOCAL_STYLE_MAX_PIXELS:
        raise RuntimeError(f"mstg_hip image: the device weight map takes canvases of at most {_lib.LOCAL_STYLE_MAX_PIXELS} pixels, "
                           f"not {target}x{target}")
    if mode == "weight_map" and weight_maps is not None:
        if len(weight_maps) != len(images):
            raise RuntimeError("mstg_hip blend: mode 'weight_map' needs one weight map per image")
        for i, m in enumerate(weight_maps):
            if tuple(m.shape) != (target, target):
                raise RuntimeError(f"mstg_hip blend: weight map {i} {tuple(m.shape)} does not match the canvas {target}x{target}")
    outs = []
    for s in range(0, len(images), batch_size):
        e = s + batch_size
        outs += _process_chunk(model, images[s:e], geoms[s:e], target, mode, strength, None if weight_maps is None else weight_maps[s:e],
                               detail, detail_coeff, enhance_colors, smooth, standard)
    return outs


def process_cyclegan_batch(model, images, target=256, batch_size=64):
    """``process_cyclegan`` for a sequence of uint8 (H, W, 3) GPU images of any sizes: byte-identical results, ``model`` called
    once per chunk of ``batch_size`` images on the (n, 3, target, target) batch under ``torch.no_grad()`` (fp32 or fp16 output),
    five library launches per chunk whatever n.  Returns uint8 tensors (views of one buffer per chunk)."""
    return _process_batch(model, images, target, batch_size, None, None, None, False)


def process_local_style_batch(model, images, mode="simple", strength=0.8, weight_maps=None, target=256, batch_size=64, detail=0.7,
                              detail_coeff=0.3, enhance_colors=True, smooth=True):
    """``process_local_style`` for a sequence of images, same modes: 'simple' (``strength``), 'weight_map' (``weight_maps``: one
    (target, target) float64 map per image, or None: the 'enhanced' map is built on the device from the chunk's canvas batch with
    ``strength``, ``detail`` and ``detail_coeff``, three more launches whatever the chunk size), 'enhanced' (the reference's
    default mode with its ``enhance_colors`` and ``smooth`` keywords: the device map and the finish launch in place of the
    blend), anything else = the styled image.  Six library launches per chunk at most, nine with the device-built map."""
    return _process_batch(model, images, target, batch_size, mode, strength, weight_maps, True, detail, detail_coeff, enhance_colors,
                          smooth)


def process_standard_batch(model, images, model_type, blend_ratio=0.3, fix_blocks=True, enhance_colors=True, smooth_level=3,
                           adaptive_smooth=True, target=256, batch_size=64):
    """``process_standard`` for a sequence of uint8 (H, W, 3) GPU images of any sizes: byte-identical results, ``model`` called
    once per chunk of ``batch_size`` images, the five launches of ``process_cyclegan_batch`` plus at most three for the finish
    per chunk, whatever the chunk size."""
    _standard_model_type(model_type)
    standard = dict(model_type=model_type, blend_ratio=blend_ratio, fix_blocks=fix_blocks, enhance_colors=enhance_colors,
                    smooth_level=smooth_level, adaptive_smooth=adaptive_smooth)
    return _process_batch(model, images, target, batch_size, _STANDARD, None, None, False, standard=standard)


def dataset_batch(images, grid_masks, img_size=256):
    """``dataset_item`` for a sequence of decoded images and their grid masks in two launches:
    (masked_images, images, masks), each (N, 3, img_size, img_size) fp32."""
    images = _req_batch(images)
    if len(grid_masks) != len(images):
        raise RuntimeError("mstg_hip image: one grid mask per image")
    S, n, dev = int(img_size), len(images), images[0].device
    plan = _BatchPlan(dev)
    pre = plan.direction(canvas=S)
    for im, g, grid in zip(images, dataset_plan([im.shape[:2] for im in images], S), grid_masks):
        pre.add(im.data_ptr(), g.height, g.width, (0, 0, g.height, g.width), (g.new_h, g.new_w), BILINEAR, (g.top, g.left, S, S),
                grid=int(grid) & (2 ** 64 - 1))
    plan.upload()
    inter = torch.empty(pre.inter_bytes, dtype=torch.uint8, device=dev)
    masked, image, mask = (torch.empty((n, 3, S, S), dtype=torch.float32, device=dev) for _ in range(3))
    pre.run_h(inter)
    pre.run_v_tensor(inter, masked, image, mask, use_mask=1)
    return masked, image, mask


# ---- the application's local-style and compare tabs (csrc/app_local_style.hip) -----------------------------------------------
APP_MODES = ("simple", "enhanced", "advanced")  # the tab's three modes in its order (gan_login_gui.py:1315, :1328, :1428)


def _edge_kernel(device):
    """the 21 float64 taps of ``mstg_gaussian_kernel_f64(21, 0)`` on ``device`` (built on the host and uploaded once)"""
    n = _lib.APP_EDGE_KSIZE
    return _device_table(("edge_kernel",), device, lambda: _host_fill("mstg_gaussian_kernel_f64", n, np.float64, n, 0.0)[1])


def app_sky_mask(canvas_u8: torch.Tensor) -> torch.Tensor:
    """The sky mask of the application's local-style tab (gan_login_gui.py:1337-1355) of an (H, W, 3) or (N, H, W, 3) uint8 canvas
    on the GPU -> uint8 (H, W) / (N, H, W): the 8-bit ``COLOR_RGB2HSV``, ``cv2.inRange([90, 30, 140], [130, 255, 255])`` on the
    upper half, two ``cv2.dilate`` with a 5 x 5 box and ``cv2.GaussianBlur((15, 15), 0)`` in OpenCV's 8.8 fixed point, one launch
    whatever N.  Restated from the definitions (include/mstg_hip.h), not compared with an OpenCV binary."""
    single, c = _stage_u8(canvas_u8, "canvas")
    N, H, W = c.shape[:3]
    mask = torch.empty((N, H, W), dtype=torch.uint8, device=c.device)
    _lib.check(_lib.load().mstg_app_sky_mask(_p(c), N, H, W, _p(mask), _stream()), "mstg_app_sky_mask")
    return mask[0] if single else mask


def app_edge_weight(canvas_u8: torch.Tensor, detail=0.6) -> torch.Tensor:
    """The edge weight of the application's local-style tab (gan_login_gui.py:1375-1391) of an (H, W, 3) or (N, H, W, 3) uint8 canvas
    on the GPU -> float64 (H, W) / (N, H, W): ``cv2.Canny(gray, 50, 150)`` (the two launches of ``enhanced_weight_map``, so H * W
    <= 147456), ``cv2.dilate`` with a 3 x 3 box, ``cv2.GaussianBlur((21, 21), 0)`` in float64 in OpenCV's summation order, times
    ``detail``; three launches whatever N.  Restated from the definitions (include/mstg_hip.h), not compared with an OpenCV
    binary."""
    single, c = _stage_u8(canvas_u8, "canvas")
    N, H, W = c.shape[:3]
    lib = _lib.load()
    state, sky, edge = (torch.empty((N, H, W), dtype=torch.uint8, device=c.device) for _ in range(3))
    count = torch.empty(N, dtype=torch.int32, device=c.device)
    weight = torch.empty((N, H, W), dtype=torch.float64, device=c.device)
    _lib.check(lib.mstg_local_style_prepare(_p(c), N, H, W, _p(state), _p(sky), _p(count), None, _stream()), "mstg_local_style_prepare")
    _lib.check(lib.mstg_local_style_hysteresis(_p(state), N, H, W, _p(edge), _stream()), "mstg_local_style_hysteresis")
    _lib.check(lib.mstg_app_edge_weight(_p(edge), N, H, W, _p(_edge_kernel(c.device)), float(detail), _p(weight), _stream()),
               "mstg_app_edge_weight")
    return weight[0] if single else weight


def _app_plan(model_type, mode, strength, detail, auto_select, ignore_sky, enhance_colors, smooth_transitions):
    """the switches and doubles of ``mstg_app_local_style_finish`` for a mode of the tab, or None for the styled image itself; the
    doubles are formed with Python's own double arithmetic, as the reference's expressions"""
    mt = _standard_model_type(model_type)  # a bad name raises whatever the mode
    if mode not in APP_MODES:
        return None
    strength, detail = float(strength), float(detail)
    if mode == "simple":
        r = max(0.05, min(1.0 - strength, 0.95))
        return dict(sky=False, auto=False, use_strength=True, w_styled=1 - r, w_canvas=r, colors=False, smooth=False, detail=detail)
    low = strength < 0.3
    bf = strength / 0.3 if low else 1.0
    plan = dict(sky=False, auto=False, use_strength=low, w_styled=bf, w_canvas=1 - bf, colors=False, smooth=False, detail=detail)
    if mode == "enhanced":
        plan.update(sky=bool(ignore_sky) and mt == _lib.STANDARD_MODEL_TYPES["photo_to_monet"], auto=bool(auto_select),
                    colors=bool(enhance_colors), smooth=bool(smooth_transitions))
    return plan


def _app_finish(canvas, styled, model_type, plan, out=None):
    """``mstg_app_local_style_finish`` for (N, H, W, 3) batches that are already checked: at most six launches on one workspace"""
    N, H, W = styled.shape[:3]
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(styled)
    dev = styled.device
    kern = _edge_kernel(dev) if plan["auto"] else None
    lut = _color_lut(model_type, dev) if plan["colors"] else None
    table = _bilateral_table(9, 75, 75, dev) if plan["smooth"] else None
    need = lib.mstg_app_local_style_workspace_bytes(N, H, W)  # 0: the call below names what is wrong with the shape
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _lib.check(lib.mstg_app_local_style_finish(_p(canvas), _p(styled), N, H, W, int(plan["sky"]), int(plan["auto"]), int(plan["use_strength"]),
                                               int(plan["smooth"]), plan["detail"], plan["w_styled"], plan["w_canvas"], _p(kern), _p(lut),
                                               _p(table), _p(out), _p(ws), need, _stream()), "mstg_app_local_style_finish")
    return out


def app_local_style_finish(canvas_u8, styled_u8, model_type, mode="enhanced", strength=0.5, detail=0.6, auto_select=True, ignore_sky=True,
                           enhance_colors=True, smooth_transitions=True) -> torch.Tensor:
    """Everything the local-style tab of the reference's application does between the forward pass and the crop
    (gan_login_gui.py:1315-1478) for an (H, W, 3) or (N, H, W, 3) uint8 canvas and styled image on the GPU, with that tab's
    options and defaults (:1051-1116).  ``mode`` names the tab's three modes in English:

    'simple'    ``styled * (1 - r) + canvas * r`` with ``r = max(0.05, min(1.0 - strength, 0.95))``;
    'enhanced'  the sky blend (``ignore_sky`` and 'photo_to_monet': ``app_sky_mask``), the edge blend (``auto_select``:
                ``app_edge_weight``; then H * W <= 147456, a larger canvas raises, naming the size), the strength blend (only for
                ``strength < 0.3``), the colour step of ``model_type`` (``enhance_colors``) and ``cv2.bilateralFilter(9, 75, 75)``
                (``smooth_transitions``); every blend is float64, clipped and truncated before the next;
    'advanced'  the strength blend alone: every helper the reference calls in this mode is guarded by ``hasattr(self, ...)`` and
                its class defines none of them;
    any other name: the styled image.

    At most six launches whatever N, byte for byte the composition of the stage functions.  ``model_type`` other than
    'photo_to_monet' / 'monet_to_photo' raises ValueError.  This is not ``process_local_style``'s chain, which restates
    batch_process_images.py.  Restated from the definitions (include/mstg_hip.h), not compared with an OpenCV binary."""
    plan = _app_plan(model_type, mode, strength, detail, auto_select, ignore_sky, enhance_colors, smooth_transitions)
    single, st = _stage_u8(styled_u8, "styled image")
    _, c = _stage_u8(canvas_u8, "canvas")
    if c.shape != st.shape:
        raise RuntimeError(f"mstg_hip app local style: shapes differ {tuple(c.shape)} vs {tuple(st.shape)}")
    out = st.clone() if plan is None else _app_finish(c, st, model_type, plan)
    return out[0] if single else out


def _app_chunk(models, images, geoms, target, model_type, plan):
    """one chunk of the two tabs: the launches of ``_process_chunk`` with every model of ``models`` called on the same input batch;
    the first model's output goes through ``_app_finish`` (``plan`` None: it stays as it is), the others are converted only; every
    output is cropped and resized back alike.  Returns one list of images per model."""
    n, T, dev = len(images), target, images[0].device
    plan_b = _BatchPlan(dev)
    pre = plan_b.direction(canvas=T)
    posts = [plan_b.direction() for _ in models]
    x = torch.empty((n, 3, T, T), dtype=torch.float32, device=dev)
    canvas = torch.empty((n, T, T, 3), dtype=torch.uint8, device=dev)
    finals = [torch.empty_like(canvas) for _ in models]
    for im, g in zip(images, geoms):
        pre.add(im.data_ptr(), g.height, g.width, (0, 0, g.height, g.width), (g.new_h, g.new_w), LANCZOS, (0, 0, g.new_h, g.new_w),
                (g.off_y, g.off_x), 255)
    for post, final in zip(posts, finals):
        for i, g in enumerate(geoms):
            left, top, crop_w, crop_h = g.crop
            post.add(final.data_ptr() + i * T * T * 3, T, T, (top, left, crop_h, crop_w), (g.out_h, g.out_w), LANCZOS,
                     (0, 0, g.out_h, g.out_w))
    plan_b.upload()
    inter = torch.empty(max([pre.inter_bytes] + [p.inter_bytes for p in posts]), dtype=torch.uint8, device=dev)
    pre.run_h(inter)
    pre.run_v_tensor(inter, x, canvas_u8=canvas)
    lib = _lib.load()
    for k, (model, final) in enumerate(zip(models, finals)):
        with torch.no_grad():
            y = model(x)
        if not y.is_cuda or tuple(y.shape) != (n, 3, T, T):
            raise RuntimeError(f"mstg_hip image: the model returned {tuple(y.shape)} for an input of {tuple(x.shape)}")
        if y.dtype not in (torch.float32, torch.float16):
            y = y.float()
        y = y.contiguous()
        styled = torch.empty_like(canvas) if k == 0 and plan is not None else final
        _lib.check(lib.mstg_img_batch_tensor_to_u8(_p(y), int(y.dtype == torch.float16), n, T, T, _p(styled), _stream()),
                   "mstg_img_batch_tensor_to_u8")
        if styled is not final:
            _app_finish(canvas, styled, model_type, plan, out=final)
    results = []
    for post in posts:
        out = torch.empty(post.out_bytes, dtype=torch.uint8, device=dev)
        post.run_h(inter)
        post.run_v_u8(inter, out)
        results.append([out[o:o + g.out_h * g.out_w * 3].view(g.out_h, g.out_w, 3) for o, g in zip(post.out_offs, geoms)])
    return results


def _app_batch(models, images, model_type, plan, target, batch_size):
    images = _req_batch(images)
    target, batch_size = int(target), int(batch_size)
    if batch_size < 1:
        raise RuntimeError(f"mstg_hip image: batch_size {batch_size}")
    geoms = letterbox_plan([im.shape[:2] for im in images], target, local_style=True)
    if plan is not None and plan["auto"] and target * target > _lib.LOCAL_STYLE_MAX_PIXELS:
        raise RuntimeError(f"mstg_hip image: with auto_select the edge weight takes canvases of at most {_lib.LOCAL_STYLE_MAX_PIXELS} "
                           f"pixels, not {target}x{target}")
    outs = [[] for _ in models]
    for s in range(0, len(images), batch_size):
        for acc, part in zip(outs, _app_chunk(models, images[s:s + batch_size], geoms[s:s + batch_size], target, model_type, plan)):
            acc += part
    return outs


def process_app_local_style_batch(model, images, model_type, mode="enhanced", strength=0.5, detail=0.6, auto_select=True, ignore_sky=True,
                                  enhance_colors=True, smooth_transitions=True, target=256, batch_size=64):
    """The local-style tab of the reference's application (gan_login_gui.py:1259-1530, local_style_process_thread) without the file
    I/O for a sequence of uint8 (H, W, 3) GPU images of any sizes, on the GPU end to end: the letterbox on white and the forward
    pass of ``process_cyclegan_batch`` (``model`` called once per chunk of ``batch_size`` images), ``app_local_style_finish`` with
    the tab's options, then the crop back to the aspect ratio (with the tab's ``min`` clamps) and the LANCZOS resize back.  The
    five launches of ``process_cyclegan_batch`` plus at most six per chunk, whatever the chunk size."""
    plan = _app_plan(model_type, mode, strength, detail, auto_select, ignore_sky, enhance_colors, smooth_transitions)
    return _app_batch([model], images, model_type, plan, target, batch_size)[0]


def process_app_local_style(model, img_u8: torch.Tensor, model_type, mode="enhanced", strength=0.5, detail=0.6, auto_select=True,
                            ignore_sky=True, enhance_colors=True, smooth_transitions=True, target=256) -> torch.Tensor:
    """``process_app_local_style_batch`` for one image."""
    return process_app_local_style_batch(model, [img_u8], model_type, mode, strength, detail, auto_select, ignore_sky, enhance_colors,
                                         smooth_transitions, target, 1)[0]


def process_compare_batch(enhanced_model, cyclegan_model, images, model_type, blend_strength=0.5, sky_handling=True, target=256,
                          batch_size=64):
    """The compare tab of the reference's application (gan_login_gui.py:2423-2638, compare_process_thread) without the file I/O
    for a sequence of images: both models are called on the same letterboxed input batch; the first output goes through the
    'enhanced' chain of ``app_local_style_finish`` with ``auto_select``, ``enhance_colors`` and ``smooth_transitions`` on,
    ``detail = 0.6``, ``strength = blend_strength`` and ``ignore_sky = sky_handling``, the second is the plain generator's
    ``to_u8`` output; both are cropped and resized back alike.  The reference's ``smooth_level`` and ``fix_blocks`` arguments are
    never read there and are not taken.  Returns (local_style, cyclegan), two lists."""
    plan = _app_plan(model_type, "enhanced", blend_strength, 0.6, True, sky_handling, True, True)
    local, plain = _app_batch([enhanced_model, cyclegan_model], images, model_type, plan, target, batch_size)
    return local, plain


def process_compare(enhanced_model, cyclegan_model, img_u8: torch.Tensor, model_type, blend_strength=0.5, sky_handling=True, target=256):
    """``process_compare_batch`` for one image -> (local_style, cyclegan)."""
    local, plain = process_compare_batch(enhanced_model, cyclegan_model, [img_u8], model_type, blend_strength, sky_handling, target, 1)
    return local[0], plain[0]


# ---- the colour-block repair of improved_smooth.py (csrc/color_blocks.hip) --------------------------------------------------
def _lab_table(device):
    """the 16-bit gamma, cube-root and coefficient tables of ``mstg_lab_tables`` on ``device`` (built on the host, uploaded once)"""
    # uploaded as int16, the same bits: torch has no uint16 on every build
    return _device_table(("lab",), device, lambda: _host_fill("mstg_lab_tables", _lib.LAB_TABLE_U16, np.uint16)[1].view(np.int16))


def _bilateral_wide_table(d, sigma_color, sigma_space, device):
    """(radius, table): the host-built weight tables of ``mstg_bilateral_wide_tables`` on ``device`` (once per parameter set); a
    radius above 90 raises, naming it"""
    args, size = (int(d), float(sigma_color), float(sigma_space)), _lib.BILATERAL_WIDE_TABLE_FLOATS
    return _device_table(("bilateral_wide",) + args, device,
                         lambda: _host_fill("mstg_bilateral_wide_tables", size, np.float32, *args, counts=True))


def _detail_ksize(sigma):
    """cv2.GaussianBlur's size for ksize = (0, 0) on float64: cvRound(sigma * 4 * 2 + 1) | 1 (round half to even)"""
    return int(round(float(sigma) * 4 * 2 + 1)) | 1


def _detail_kernel(ksize, sigma, device):
    """the float64 taps of ``mstg_gaussian_kernel_f64(ksize, sigma)`` on ``device`` (built on the host and uploaded once)"""
    args = (int(ksize), float(sigma))
    return _device_table(("detail_kernel",) + args, device, lambda: _host_fill("mstg_gaussian_kernel_f64", args[0], np.float64, *args)[1])


def detect_color_blocks(img: torch.Tensor, threshold=30, kernel_size=11) -> torch.Tensor:
    """``detect_color_blocks`` of the reference (improved_smooth.py:53-95) for an (H, W, 3) or (N, H, W, 3) uint8 RGB image on the
    GPU -> bool (H, W) / (N, H, W): a and b of the 8-bit ``COLOR_RGB2LAB``, ``cv2.Sobel(ksize=3)`` on both, the mean of the two
    magnitudes ``> threshold``, ``cv2.dilate`` with a ``kernel_size`` box (odd, at most 31; anything else raises, naming
    kernel_size); two launches whatever N.  Restated from the definitions (include/mstg_hip.h), not compared with an OpenCV
    binary."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    mask = torch.empty((N, H, W), dtype=torch.uint8, device=x.device)
    ws = torch.empty((N, H, W), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().mstg_color_block_mask(_p(x), N, H, W, _p(_lab_table(x.device)), float(threshold), int(kernel_size), _p(mask),
                                                 _p(ws), ws.numel(), _stream()), "mstg_color_block_mask")
    mask = mask != 0
    return mask[0] if single else mask


def adaptive_color_correction(img: torch.Tensor, blocks_detected=None, radius=50) -> torch.Tensor:
    """``adaptive_color_correction`` of the reference (improved_smooth.py:10-51) for an (H, W, 3) or (N, H, W, 3) uint8 image on the
    GPU: every pixel flagged in ``blocks_detected`` (bool or bytes, (H, W) / (N, H, W); None: ``detect_color_blocks(img)``) becomes
    ``0.5 * px + 0.5 * mean`` of its ``(2 radius + 1)^2`` window of the input clipped to the image, in float64, truncated; the
    others are copied.  Two launches whatever N and no host synchronisation: with nothing flagged the result is the input."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    if blocks_detected is None:
        m = detect_color_blocks(x)
    else:
        m = blocks_detected.unsqueeze(0) if blocks_detected.dim() == 2 else blocks_detected
        if not m.is_cuda or tuple(m.shape) != (N, H, W):
            raise RuntimeError(f"mstg_hip colour blocks: expected a mask of shape {(N, H, W)} on the GPU, got {tuple(m.shape)}")
    m = m.to(torch.uint8).contiguous()
    out = torch.empty_like(x)
    ws = torch.empty(N * H * W * 3, dtype=torch.int32, device=x.device)
    _lib.check(_lib.load().mstg_color_correct_u8(_p(x), _p(m), N, H, W, int(radius), _p(out), _p(ws), ws.numel() * 4, _stream()),
               "mstg_color_correct_u8")
    return out[0] if single else out


def edge_preserving_smoothing(img: torch.Tensor, sigma_s=60, sigma_r=0.4) -> torch.Tensor:
    """``edge_preserving_smoothing`` of the reference (improved_smooth.py:97-112) for an (H, W, 3) or (N, H, W, 3) uint8 image on
    the GPU: ``cv2.bilateralFilter(img, 0, sigma_r * 255, sigma_s)`` as include/mstg_hip.h defines it, the radius derived from
    ``sigma_s`` (90 and 25 445 taps at the default; above 90, sigma_s >= 61, raises, naming the radius); one launch whatever N.  Not
    compared with an OpenCV binary."""
    return bilateral_wide_u8(img, 0, sigma_r * 255, sigma_s)


def bilateral_wide_u8(img: torch.Tensor, d=0, sigma_color=102.0, sigma_space=60) -> torch.Tensor:
    """``cv2.bilateralFilter(img, d, sigma_color, sigma_space)`` for any ``d`` (``d <= 0``: the radius is ``cvRound(sigma_space *
    1.5)``) up to radius 90, the definition of ``bilateral_u8`` through ``mstg_bilateral_wide_u8``; at d = 3, 5, 7, 9 the same
    bytes as ``bilateral_u8``."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    radius, table = _bilateral_wide_table(d, sigma_color, sigma_space, x.device)
    out = torch.empty_like(x)
    _lib.check(_lib.load().mstg_bilateral_wide_u8(_p(x), N, H, W, radius, _p(table), _p(out), _stream()), "mstg_bilateral_wide_u8")
    return out[0] if single else out


def _same_size(original, x):
    """``original`` as an (N, H, W, 3) batch of the size of ``x``: an original of another size goes through the Lanczos resize"""
    o = original.unsqueeze(0) if original.dim() == 3 else original
    H, W = x.shape[1:3]
    if tuple(o.shape[1:3]) != (H, W):
        o = torch.stack([resize_u8(im, (W, H), LANCZOS) for im in o])
    o = _req_canvases(o, "original")
    if o.shape != x.shape:
        raise RuntimeError(f"mstg_hip colour blocks: shapes differ {tuple(o.shape)} vs {tuple(x.shape)}")
    return o


def detail_enhancing_blend(img: torch.Tensor, original: torch.Tensor, alpha=0.3, beta=1.5, sigma=3.0) -> torch.Tensor:
    """``detail_enhancing_blend`` of the reference (improved_smooth.py:114-135) for (H, W, 3) or (N, H, W, 3) uint8 images on the
    GPU: ``img * (1 - alpha) + original * alpha + (original - GaussianBlur(original, (0, 0), sigma)) * beta`` in float64 in
    OpenCV's summation order, clipped and truncated; an ``original`` of another size is resized first (Lanczos).  ``sigma`` is 3
    in the reference (25 taps); a size above 31 (sigma above 3.81) raises, naming ksize.  Two launches whatever N."""
    single, x = _stage_u8(img, "image")
    o = _same_size(original, x)
    N, H, W = x.shape[:3]
    ksize = _detail_ksize(sigma)
    lib = _lib.load()
    if ksize > 31:  # before the taps are built: the refusal names the size
        _lib.check(lib.mstg_detail_blend_u8(None, None, N, H, W, None, ksize, 0.0, 0.0, 0.0, None, None, 0, None), "mstg_detail_blend_u8")
    kern = _detail_kernel(ksize, sigma, x.device)
    out = torch.empty_like(x)
    ws = torch.empty(N * H * W * 3, dtype=torch.float64, device=x.device)
    alpha, beta = float(alpha), float(beta)
    _lib.check(lib.mstg_detail_blend_u8(_p(x), _p(o), N, H, W, _p(kern), ksize, 1 - alpha, alpha, beta, _p(out), _p(ws), ws.numel() * 8,
                                        _stream()), "mstg_detail_blend_u8")
    return out[0] if single else out


def fix_color_blocks(img: torch.Tensor, original=None) -> torch.Tensor:
    """``fix_color_blocks_improved`` of the reference (improved_smooth.py:137-164) between decoding and encoding, for an (H, W, 3)
    or (N, H, W, 3) uint8 image on the GPU with the reference's constants: ``detect_color_blocks`` (30, 11),
    ``adaptive_color_correction`` (radius 50), ``edge_preserving_smoothing`` (60, 0.4) and, with an ``original``,
    ``detail_enhancing_blend`` (alpha 0.1, beta 0.5).  Five launches on one workspace (seven with an original) whatever N, byte
    for byte the composition of the four stage functions.  Restated from the definitions (include/mstg_hip.h), not compared with
    an OpenCV binary."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    lib = _lib.load()
    dev = x.device
    o = _same_size(original, x) if original is not None else None
    radius, table = _bilateral_wide_table(0, 0.4 * 255, 60, dev)
    ksize, alpha, beta = _detail_ksize(3.0), 0.1, 0.5
    kern = _detail_kernel(ksize, 3.0, dev) if o is not None else None
    out = torch.empty_like(x)
    need = lib.mstg_color_block_fix_workspace_bytes(N, H, W, int(o is not None))  # 0: the call below names what is wrong
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    _lib.check(lib.mstg_color_block_fix(_p(x), _p(o), N, H, W, _p(_lab_table(dev)), 30.0, 11, 50, radius, _p(table), _p(kern), ksize,
                                        1 - alpha, alpha, beta, _p(out), _p(ws), need, _stream()), "mstg_color_block_fix")
    return out[0] if single else out


# ---- the segmentation-driven local style of enhanced_local_style.py (csrc/segment_style.hip) -------------------------------
def felzenszwalb_labels(img, scale=100, sigma=0.5, min_size=50) -> np.ndarray:
    """``skimage.segmentation.felzenszwalb(img, scale, sigma, min_size)`` of an (H, W, 3) uint8 image (numpy, or a tensor that is
    copied to the host) on the HOST, as include/mstg_hip.h defines it -> int32 numpy (H, W), labels 0 .. count - 1.  Equal edge
    costs keep their order (a stable sort): this build's definition, where scikit-image leaves them as numpy's unstable sort does.
    Only ``sigma=0.5`` is built; another value raises, naming it.  Not compared with scikit-image."""
    a = img.detach().cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise RuntimeError(f"mstg_hip segmentation: expected an (H, W, 3) uint8 image, got {a.dtype} {tuple(a.shape)}")
    a = np.ascontiguousarray(a)
    H, W = a.shape[:2]
    labels = np.zeros((H, W), dtype=np.int32)
    rc = _lib.load().mstg_felzenszwalb_u8(a.ctypes.data, H, W, float(scale), float(sigma), int(min_size), labels.ctypes.data)
    if rc <= 0:
        _lib.check(rc or -1, "mstg_felzenszwalb_u8")
    return labels


SEGMENTATIONS = ("felzenszwalb", "slic")


def slic_grid(H, W, n_segments=100):
    """(step, ny, nx) of the SLIC grid of an (H, W) image as include/mstg_hip.h defines it (K = ny * nx centres), from the host
    entry ``mstg_slic_grid``; a shape that is not built raises, naming the value."""
    out = np.zeros(3, dtype=np.int32)
    at = out.ctypes.data
    _lib.check(_lib.load().mstg_slic_grid(int(H), int(W), int(n_segments), at, at + 4, at + 8), "mstg_slic_grid")
    return int(out[0]), int(out[1]), int(out[2])


def slic_min_size(H, W, n_segments=100):
    """the connectivity step's ``min_size`` for the SLIC grid of (H, W): ``int(0.5 * (H * W / K))``"""
    _, ny, nx = slic_grid(H, W, n_segments)
    return int(0.5 * (float(H * W) / float(ny * nx)))


def slic_segment_bound(H, W, n_segments=100):
    """The most segments ``slic_labels`` can return for an (H, W) image: ``H * W // max(min_size, 1) + 1`` (every segment but the
    first pixel's has at least ``min_size`` pixels).  Computed on the host, so a caller sizes per-segment buffers without reading
    the count back; the labels are 1 .. count, so ``segment_blend_map`` takes ``num_segments = bound + 1``."""
    return int(H) * int(W) // max(slic_min_size(H, W, n_segments), 1) + 1


def _slic_call(entry, img_u8, n_segments, compactness, extra):
    single, x = _stage_u8(img_u8, "image")
    N, H, W = x.shape[:3]
    lib = _lib.load()
    labels = torch.empty((N, H, W), dtype=torch.int32, device=x.device)
    need = lib.mstg_slic_workspace_bytes(N, H, W, int(n_segments))  # 0: the call below names what is wrong
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    out = extra(N, H, W, x.device)
    _lib.check(getattr(lib, entry)(_p(x), N, H, W, int(n_segments), float(compactness), _p(_lab_table(x.device)), _p(labels), _p(out), _p(ws),
                                   need, _stream()), entry)
    return single, labels, out


def slic_labels(img_u8, n_segments=100, compactness=10.0, return_count=False):
    """``skimage.segmentation.slic(img, n_segments, compactness)`` of an (H, W, 3) or (N, H, W, 3) uint8 image on the GPU as
    include/mstg_hip.h defines it -> int32 (H, W) / (N, H, W) on the device, labels 1 .. count; with ``return_count`` also the
    count, an int32 tensor () / (N,) on the device.  The features are this build's 8-bit Lab and the connectivity step is this
    build's own (see the header); ten rounds, no host step and no host synchronisation; bit-reproducible.  A shape that is not
    built raises, naming the value.  Not compared with scikit-image."""
    single, labels, count = _slic_call("mstg_slic_u8", img_u8, n_segments, compactness,
                                       lambda N, H, W, dev: torch.empty((N,), dtype=torch.int32, device=dev))
    if single:
        labels, count = labels[0], count[0]
    return (labels, count) if return_count else labels


def slic_assign(img_u8, n_segments=100, compactness=10.0):
    """The ten rounds of assignment and update alone (steps 1 to 3 of the header) -> (raw labels int32 (H, W) / (N, H, W) in
    0 .. K - 1, centres float32 (K, 5) / (N, K, 5): y, x, L, a, b after the last update), on the device."""
    def centres_of(N, H, W, dev):
        _, ny, nx = slic_grid(H, W, n_segments)
        return torch.empty((N, ny * nx, 5), dtype=torch.float32, device=dev)

    single, labels, centres = _slic_call("mstg_slic_assign_u8", img_u8, n_segments, compactness, centres_of)
    return (labels[0], centres[0]) if single else (labels, centres)


def connect_labels(labels, min_size, return_count=False):
    """The connectivity step alone (step 4 of the header) on any integer labels (H, W) / (N, H, W) (numpy or tensor) on ``cuda`` ->
    int32 labels 1 .. count of the same shape on the device: 4-connected components, every component smaller than ``min_size``
    joined to the component of the pixel before its first pixel, the rest numbered in raster order of their first pixels."""
    lab = torch.from_numpy(np.ascontiguousarray(labels)) if isinstance(labels, np.ndarray) else labels
    lab = lab.to(device=lab.device if lab.is_cuda else "cuda", dtype=torch.int32).contiguous()
    single = lab.dim() == 2
    if single:
        lab = lab.unsqueeze(0)
    if lab.dim() != 3:
        raise RuntimeError(f"mstg_hip segmentation: expected labels of shape (H, W) or (N, H, W), got {tuple(lab.shape)}")
    N, H, W = lab.shape
    lib = _lib.load()
    out, count = torch.empty_like(lab), torch.empty((N,), dtype=torch.int32, device=lab.device)
    need = lib.mstg_connect_labels_workspace_bytes(N, H, W)  # 0: the call below names what is wrong
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=lab.device)
    _lib.check(lib.mstg_connect_labels(_p(lab), N, H, W, int(min_size), _p(out), _p(count), _p(ws), need, _stream()), "mstg_connect_labels")
    if single:
        out, count = out[0], count[0]
    return (out, count) if return_count else out


def _quickshift_args(ratio, kernel_size, max_dist=None):
    return (float(ratio), float(kernel_size)) + (() if max_dist is None else (float(max_dist),))


def quickshift_density(img_u8, ratio=1.0, kernel_size=5):
    """The density of ``skimage.segmentation.quickshift(img, ratio, kernel_size)`` (steps 1 to 3 of the header's definition) of an
    (H, W, 3) or (N, H, W, 3) uint8 image on the GPU -> int64 (H, W) / (N, H, W) on the device: per pixel the sum over its window
    of ``rint(exp(-D / (2 kernel_size^2)) * 2^32)``, an exact integer (this build's own form: bit-reproducible however the window
    is split).  One launch.  A parameter that is not built raises, naming the value.  Not compared with scikit-image."""
    single, x = _stage_u8(img_u8, "image")
    N, H, W = x.shape[:3]
    dens = torch.empty((N, H, W), dtype=torch.int64, device=x.device)
    _lib.check(_lib.load().mstg_quickshift_density_u8(_p(x), N, H, W, *_quickshift_args(ratio, kernel_size), _p(_lab_table(x.device)), _p(dens),
                                                      _stream()), "mstg_quickshift_density_u8")
    return dens[0] if single else dens


def quickshift_parents(img_u8, density, ratio=1.0, kernel_size=5, max_dist=10):
    """Step 4 of the header's definition on a GIVEN int64 density (H, W) / (N, H, W) (numpy or tensor) -> int32 of the same shape on
    the device: every pixel's parent as a raster index inside its image, a root its own parent.  Among equal densities the lower
    raster index is the higher pixel (this build's tie rule).  One launch."""
    single, x = _stage_u8(img_u8, "image")
    N, H, W = x.shape[:3]
    d = torch.from_numpy(np.ascontiguousarray(density)) if isinstance(density, np.ndarray) else density
    d = d.to(device=x.device, dtype=torch.int64).contiguous()
    if d.dim() == 2:
        d = d.unsqueeze(0)
    if tuple(d.shape) != (N, H, W):
        raise RuntimeError(f"mstg_hip segmentation: expected a density of shape {(N, H, W)}, got {tuple(d.shape)}")
    parent = torch.empty((N, H, W), dtype=torch.int32, device=x.device)
    _lib.check(_lib.load().mstg_quickshift_parents_u8(_p(x), _p(d), N, H, W, *_quickshift_args(ratio, kernel_size, max_dist),
                                                      _p(_lab_table(x.device)), _p(parent), _stream()), "mstg_quickshift_parents_u8")
    return parent[0] if single else parent


def quickshift_labels(img_u8, ratio=1.0, kernel_size=5, max_dist=10, return_count=False):
    """``skimage.segmentation.quickshift(img, ratio, kernel_size, max_dist)`` of an (H, W, 3) or (N, H, W, 3) uint8 image on the GPU
    as include/mstg_hip.h defines it -> int32 (H, W) / (N, H, W) on the device, labels 0 .. count - 1 numbered by ascending root;
    with ``return_count`` also the count, an int32 tensor () / (N,) on the device.  The 8-bit Lab features, the fixed-point density
    and the tie rule by raster index are this build's own (see the header); no host step and no host synchronisation;
    bit-reproducible.  The defaults are scikit-image's; the reference calls it with (0.5, 3, 6): ``quickshift_segmenter``.  A
    parameter that is not built raises, naming the value.  Not compared with scikit-image."""
    single, x = _stage_u8(img_u8, "image")
    N, H, W = x.shape[:3]
    lib = _lib.load()
    labels = torch.empty((N, H, W), dtype=torch.int32, device=x.device)
    count = torch.empty((N,), dtype=torch.int32, device=x.device)
    need = lib.mstg_quickshift_workspace_bytes(N, H, W, float(kernel_size))  # 0: the call below names what is wrong
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    _lib.check(lib.mstg_quickshift_u8(_p(x), N, H, W, *_quickshift_args(ratio, kernel_size, max_dist), _p(_lab_table(x.device)), _p(labels),
                                      _p(count), _p(ws), need, _stream()), "mstg_quickshift_u8")
    if single:
        labels, count = labels[0], count[0]
    return (labels, count) if return_count else labels


def quickshift_segmenter(ratio=0.5, kernel_size=3, max_dist=6):
    """A callable for ``process_enhanced_local_style(segments=...)``: canvas -> (``quickshift_labels(canvas, ...)``, H * W).  The
    defaults are the reference's call (enhanced_local_style.py:70).  H * W is the only bound on the count the host can know, so
    the map is sized by it and nothing synchronises."""
    def segment(canvas):
        return quickshift_labels(canvas, ratio, kernel_size, max_dist), int(canvas.shape[-3]) * int(canvas.shape[-2])
    return segment


def slic_segmenter(n_segments=100, compactness=10.0):
    """A callable for ``process_enhanced_local_style(segments=...)``: canvas -> (``slic_labels(canvas, ...)``, bound + 1); with the
    defaults what ``segmentation="slic"`` does."""
    def segment(canvas):
        H, W = int(canvas.shape[-3]), int(canvas.shape[-2])
        return slic_labels(canvas, n_segments, compactness), slic_segment_bound(H, W, n_segments) + 1  # labels 1 .. count <= bound
    return segment


def _req_labels(labels, shape, device):
    lab = torch.from_numpy(np.ascontiguousarray(labels)) if isinstance(labels, np.ndarray) else labels
    lab = lab.to(device=device, dtype=torch.int32).contiguous()
    if lab.dim() == 2:
        lab = lab.unsqueeze(0)
    if tuple(lab.shape) != tuple(shape):
        raise RuntimeError(f"mstg_hip segment style: expected labels of shape {tuple(shape)}, got {tuple(lab.shape)}")
    return lab


def segment_blend_map(canvas_u8, labels, num_segments=None, smooth=True, return_stats=False):
    """``determine_blend_ratios(analyze_segments(canvas, labels), labels, shape)`` of the reference (enhanced_local_style.py:76-176)
    for an (H, W, 3) or (N, H, W, 3) uint8 canvas on the GPU and integer labels (H, W) / (N, H, W) (numpy or tensor) -> float32
    (H, W) / (N, H, W): the per-segment sums in one pass over the image (a segmented reduction keyed by label), the ratio of every
    label, the map, and with ``smooth`` ``scipy.ndimage.gaussian_filter(map, sigma=3)``.  ``num_segments`` None: the largest label
    + 1 (one host synchronisation); a label outside ``[0, num_segments)`` belongs to no segment and gets 0.  With ``return_stats``
    also (sums int64 (N, S, 11): n, sum R, G, B, R^2, G^2, B^2, S, y, x and the 2^32 fixed-point edge sum; ratio float32 (N, S)).
    Four launches, six with ``smooth``, whatever N and the number of segments; bit-reproducible."""
    single, c = _stage_u8(canvas_u8, "canvas")
    N, H, W = c.shape[:3]
    lab = _req_labels(labels, (N, H, W), c.device)
    S = int(lab.max().item()) + 1 if num_segments is None else int(num_segments)
    lib = _lib.load()
    out = torch.empty((N, H, W), dtype=torch.float32, device=c.device)
    sums = torch.empty((N, max(S, 1), _lib.SEGMENT_SUMS), dtype=torch.int64, device=c.device)
    ratio = torch.empty((N, max(S, 1)), dtype=torch.float32, device=c.device)
    need = lib.mstg_segment_blend_map_workspace_bytes(N, H, W, S, int(bool(smooth)))  # 0: the call below names what is wrong
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=c.device)
    _lib.check(lib.mstg_segment_blend_map(_p(c), _p(lab), N, H, W, S, int(bool(smooth)), _p(out), _p(sums), _p(ratio), _p(ws), need, _stream()),
               "mstg_segment_blend_map")
    if single:
        out, sums, ratio = out[0], sums[0], ratio[0]
    return (out, sums, ratio) if return_stats else out


def gaussian_reflect_f32(plane: torch.Tensor) -> torch.Tensor:
    """``scipy.ndimage.gaussian_filter(plane, sigma=3)`` of a float32 (H, W) or (N, H, W) tensor on the GPU, bit for bit (radius 12,
    float64 weights and accumulation, mode 'reflect', float32 between the two passes); two launches."""
    single = plane.dim() == 2
    x = (plane.unsqueeze(0) if single else plane).contiguous()
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 3:
        raise RuntimeError(f"mstg_hip segment style: expected a float32 (H, W) or (N, H, W) tensor on the GPU, got {x.dtype} {tuple(x.shape)}")
    N, H, W = x.shape
    out, ws = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.load().mstg_gaussian_reflect_f32(_p(x), N, H, W, _p(out), _p(ws), ws.numel() * 4, _stream()), "mstg_gaussian_reflect_f32")
    return out[0] if single else out


def _clahe_ws(lib, N, H, W, device):
    need = lib.mstg_clahe_workspace_bytes(N, H, W)  # 0: the call names what is wrong with the shape
    return need, torch.empty(max(need, 16), dtype=torch.uint8, device=device)


def clahe_u8(plane: torch.Tensor) -> torch.Tensor:
    """``cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)).apply(plane)`` of a uint8 (H, W) or (N, H, W) plane on the GPU as
    include/mstg_hip.h defines it; H and W must be multiples of 8 (OpenCV pads other sizes: raises, naming them).  Two launches.
    Not compared with an OpenCV binary."""
    single = plane.dim() == 2
    x = (plane.unsqueeze(0) if single else plane).contiguous()
    if not x.is_cuda or x.dtype != torch.uint8 or x.dim() != 3:
        raise RuntimeError(f"mstg_hip segment style: expected a uint8 (H, W) or (N, H, W) plane on the GPU, got {x.dtype} {tuple(x.shape)}")
    N, H, W = x.shape
    lib = _lib.load()
    need, ws = _clahe_ws(lib, N, H, W, x.device)
    out = torch.empty_like(x)
    _lib.check(lib.mstg_clahe_u8(_p(x), N, H, W, _p(out), _p(ws), need, _stream()), "mstg_clahe_u8")
    return out[0] if single else out


def hsv_enhance_u8(img: torch.Tensor) -> torch.Tensor:
    """The colour step of the reference (enhanced_local_style.py:243-257) for an (H, W, 3) or (N, H, W, 3) uint8 image on the GPU:
    8-bit ``COLOR_RGB2HSV``, s * 1.2 saturated, CLAHE(2.0, 8 x 8) of v, ``COLOR_HSV2RGB``; H and W multiples of 8.  Two launches.
    Not compared with an OpenCV binary."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    lib = _lib.load()
    need, ws = _clahe_ws(lib, N, H, W, x.device)
    out = torch.empty_like(x)
    _lib.check(lib.mstg_hsv_enhance_u8(_p(x), N, H, W, _p(out), _p(ws), need, _stream()), "mstg_hsv_enhance_u8")
    return out[0] if single else out


def sharpen3_u8(img: torch.Tensor) -> torch.Tensor:
    """``cv2.filter2D(img, -1, [[-1,-1,-1],[-1,9,-1],[-1,-1,-1]])`` of an (H, W, 3) or (N, H, W, 3) uint8 image on the GPU
    (enhanced_local_style.py:260-261): exact integers, BORDER_REFLECT_101, saturated; one launch."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    out = torch.empty_like(x)
    _lib.check(_lib.load().mstg_sharpen3_u8(_p(x), N, H, W, _p(out), _stream()), "mstg_sharpen3_u8")
    return out[0] if single else out


def _req_map(blend_map, shape, device):
    m = torch.from_numpy(np.ascontiguousarray(blend_map)) if isinstance(blend_map, np.ndarray) else blend_map
    m = m.to(device=device, dtype=torch.float32).contiguous()
    if m.dim() == 2:
        m = m.unsqueeze(0)
    if tuple(m.shape) != tuple(shape):
        raise RuntimeError(f"mstg_hip segment style: expected a blend map of shape {tuple(shape)}, got {tuple(m.shape)}")
    return m


def blend_map_u8(canvas_u8, styled_u8, blend_map) -> torch.Tensor:
    """``styled * map + canvas * (1 - map)`` in float32 as numpy forms it from uint8 and float32 arrays, clipped and truncated
    (enhanced_local_style.py:232-240); not ``blend_u8``, which is float64.  One launch."""
    single, st = _stage_u8(styled_u8, "styled image")
    _, c = _stage_u8(canvas_u8, "canvas")
    if c.shape != st.shape:
        raise RuntimeError(f"mstg_hip segment style: shapes differ {tuple(c.shape)} vs {tuple(st.shape)}")
    N, H, W = st.shape[:3]
    m = _req_map(blend_map, (N, H, W), st.device)
    out = torch.empty_like(st)
    _lib.check(_lib.load().mstg_blend_map_f32_u8(_p(c), _p(st), _p(m), N, H, W, _p(out), _stream()), "mstg_blend_map_f32_u8")
    return out[0] if single else out


def enhanced_style_finish(canvas_u8, styled_u8, blend_map) -> torch.Tensor:
    """Everything ``enhanced_local_style_transfer`` of the reference does between the blend map and the crop
    (enhanced_local_style.py:232-264) for (H, W, 3) or (N, H, W, 3) uint8 images and a float32 map on the GPU: the float32 blend,
    the colour step (``hsv_enhance_u8``), ``sharpen3_u8`` and ``cv2.bilateralFilter(5, 50, 50)``; H and W multiples of 8.  Five
    launches on one workspace whatever N, byte for byte the composition of ``blend_map_u8``, ``hsv_enhance_u8``, ``sharpen3_u8``
    and ``bilateral_u8(d=5, 50, 50)``.  Not compared with an OpenCV binary."""
    single, st = _stage_u8(styled_u8, "styled image")
    _, c = _stage_u8(canvas_u8, "canvas")
    if c.shape != st.shape:
        raise RuntimeError(f"mstg_hip segment style: shapes differ {tuple(c.shape)} vs {tuple(st.shape)}")
    N, H, W = st.shape[:3]
    m = _req_map(blend_map, (N, H, W), st.device)
    lib = _lib.load()
    table = _bilateral_table(5, 50, 50, st.device)
    out = torch.empty_like(st)
    need = lib.mstg_enhanced_style_finish_workspace_bytes(N, H, W)  # 0: the call below names what is wrong with the shape
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=st.device)
    _lib.check(lib.mstg_enhanced_style_finish(_p(c), _p(st), _p(m), N, H, W, _p(table), _p(out), _p(ws), need, _stream()),
               "mstg_enhanced_style_finish")
    return out[0] if single else out


def letterbox_black(img_u8: torch.Tensor, target=256):
    """enhanced_local_style.py:184-203: ``letterbox`` on a BLACK canvas -> (canvas, (width, height))"""
    height, width = img_u8.shape[:2]
    if width > height:
        new_width, new_height = target, int(height * (target / width))
    else:
        new_height, new_width = target, int(width * (target / height))
    resized = resize_u8(img_u8, (new_width, new_height), LANCZOS)
    off_x, off_y = (target - new_width) // 2, (target - new_height) // 2
    return paste_u8(resized, (0, 0, new_height, new_width), (target, target), (off_y, off_x), fill=0), (width, height)


def process_enhanced_local_style(model, img_u8: torch.Tensor, segments=None, target=256, segmentation="felzenszwalb") -> torch.Tensor:
    """``enhanced_local_style_transfer`` of the reference (enhanced_local_style.py:178-292) without the file I/O and the chart:
    decoded uint8 image in, uint8 image out.  The letterbox on black, the forward pass, ``segment_blend_map`` of the canvas with
    ``segments`` (integer labels (target, target); None: ``felzenszwalb_labels(canvas)``, the one host step), ``enhanced_style_finish``,
    the crop of :270-277 exactly as written (its ``min(target, int(...))`` sizes leave an image larger than the canvas in both
    directions uncropped) and the LANCZOS resize back under the condition of :280.  ``segmentation="slic"``: ``slic_labels(canvas)``
    in the place of the host step; the labels stay on the device and the map gets ``slic_segment_bound`` for its size, so nothing
    leaves the device and nothing synchronises.  ``segments``, when given, wins; it may also be a CALLABLE that takes the device
    canvas and returns labels or ``(labels, num_segments)`` (``quickshift_segmenter()``, ``slic_segmenter()``): the labels then never
    leave the device, and with a ``num_segments`` nothing synchronises.  Quickshift is reached this way and not through
    ``segmentation``, whose values stay ``SEGMENTATIONS``."""
    if segmentation not in SEGMENTATIONS:
        raise ValueError(f"mstg_hip image: segmentation {segmentation!r} is none of {SEGMENTATIONS}")
    canvas, (width, height) = letterbox_black(img_u8, target)
    x = to_tensor(canvas).unsqueeze(0)
    with torch.no_grad():
        y = model(x)
    styled = to_u8(y[0])
    num_segments = None
    if callable(segments):
        segments = segments(canvas)
        if isinstance(segments, tuple):
            segments, num_segments = segments
    elif segments is None and segmentation == "slic":
        segments, num_segments = slic_segmenter()(canvas)
    elif segments is None:
        segments = felzenszwalb_labels(canvas)
    blend_map = segment_blend_map(canvas, segments, num_segments)
    out = enhanced_style_finish(canvas, styled, blend_map)
    if width != height:
        new_width = min(target, int(height * (width / height)))
        new_height = min(target, int(width * (height / width)))
        left, top = (target - new_width) // 2, (target - new_height) // 2
        out = crop_u8(out, left, top, left + new_width, top + new_height)
    if (width > target or height > target) and width * height <= 1024 * 1024:
        out = resize_u8(out, (width, height), LANCZOS)
    return out


# ---- the five settings of advanced_transform.py (csrc/advanced_transform.hip) ------------------------------------------------
ADVANCED_SETTINGS = ("standard", "contrast", "multi_scale", "detail", "regions")


def _lab_inverse_table(device):
    """the 16-bit tables of ``mstg_lab_inverse_tables`` on ``device`` (built on the host, uploaded once; int16 holds the same bits)"""
    return _device_table(("lab_inverse",), device,
                         lambda: _host_fill("mstg_lab_inverse_tables", _lib.LAB_INV_TABLE_U16, np.uint16)[1].view(np.int16))


@lru_cache(maxsize=32)
def gaussian_sigma_taps(sigma: float):
    """(ksize, taps, margin) of ``cv2.GaussianBlur(u8, (0, 0), sigma)``: ``ksize = cvRound(sigma * 6 + 1) | 1``, the 8.8 fixed-point
    taps (int32 numpy, ``ksize`` of them) and the smallest distance of a rounded quantity from a tie, from the host entry
    ``mstg_gaussian_sigma_taps``; a size above 31 (sigma above 5) raises, naming ksize."""
    taps, margin = np.zeros(_lib.GAUSSIAN_SIGMA_MAX_KSIZE, dtype=np.int32), np.zeros(1, dtype=np.float64)
    ksize = _lib.load().mstg_gaussian_sigma_taps(float(sigma), taps.ctypes.data, margin.ctypes.data)
    if ksize <= 0:
        _lib.check(ksize or -1, "mstg_gaussian_sigma_taps")
    return ksize, taps, float(margin[0])


def lab_u8(img: torch.Tensor) -> torch.Tensor:
    """``cv2.cvtColor(img, cv2.COLOR_RGB2LAB)`` of an (H, W, 3) or (N, H, W, 3) uint8 image on the GPU -> (L, a, b) bytes of the same
    shape: OpenCV's integer path as include/mstg_hip.h defines it (a and b are those of ``detect_color_blocks``); one launch.  Not
    compared with an OpenCV binary."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    out = torch.empty_like(x)
    _lib.check(_lib.load().mstg_lab_u8(_p(x), N, H, W, _p(_lab_table(x.device)), _p(out), _stream()), "mstg_lab_u8")
    return out[0] if single else out


def lab2rgb_u8(lab: torch.Tensor) -> torch.Tensor:
    """``cv2.cvtColor(lab, cv2.COLOR_LAB2RGB)`` of (L, a, b) bytes, (H, W, 3) or (N, H, W, 3), on the GPU: an integer path from
    host-built tables whose structure is OpenCV's and whose constants are this build's (include/mstg_hip.h states the measured
    distance from a float64 CIE inverse); every byte triple has a result, out-of-gamut ones clamp.  One launch."""
    single, x = _stage_u8(lab, "Lab image")
    N, H, W = x.shape[:3]
    out = torch.empty_like(x)
    _lib.check(_lib.load().mstg_lab2rgb_u8(_p(x), N, H, W, _p(_lab_inverse_table(x.device)), _p(out), _stream()), "mstg_lab2rgb_u8")
    return out[0] if single else out


def _req_plane(plane, what):
    single = plane.dim() == 2
    x = (plane.unsqueeze(0) if single else plane).contiguous()
    if not x.is_cuda or x.dtype != torch.uint8 or x.dim() != 3:
        raise RuntimeError(f"mstg_hip advanced transform: expected a uint8 (H, W) or (N, H, W) {what} on the GPU, got {x.dtype} {tuple(x.shape)}")
    return single, x


def gaussian_sigma_u8(plane: torch.Tensor, sigma=3.0) -> torch.Tensor:
    """``cv2.GaussianBlur(plane, (0, 0), sigma)`` of a uint8 (H, W) or (N, H, W) plane on the GPU: OpenCV's bit-exact 8.8
    fixed-point path with the taps of ``gaussian_sigma_taps`` (19 at sigma 3), BORDER_REFLECT_101 for any side; two launches.  Not
    compared with an OpenCV binary."""
    single, x = _req_plane(plane, "plane")
    N, H, W = x.shape
    ksize, taps, _ = gaussian_sigma_taps(float(sigma))
    out = torch.empty_like(x)
    ws = torch.empty(N * H * W, dtype=torch.int16, device=x.device)
    _lib.check(_lib.load().mstg_gaussian_sigma_u8(_p(x), N, H, W, taps.ctypes.data, ksize, _p(out), _p(ws), ws.numel() * 2, _stream()),
               "mstg_gaussian_sigma_u8")
    return out[0] if single else out


def hsv_gain_u8(img: torch.Tensor, s_gain=1.2, v_gain=1.0) -> torch.Tensor:
    """8-bit ``COLOR_RGB2HSV``, ``cv2.multiply(s, s_gain)`` and ``cv2.multiply(v, v_gain)`` (float32, rounded half to even,
    saturated), ``COLOR_HSV2RGB`` of an (H, W, 3) or (N, H, W, 3) uint8 image on the GPU: the colour step of ``hsv_enhance_u8``
    without its CLAHE; one launch."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    out = torch.empty_like(x)
    _lib.check(_lib.load().mstg_hsv_gain_u8(_p(x), N, H, W, float(s_gain), float(v_gain), _p(out), _stream()), "mstg_hsv_gain_u8")
    return out[0] if single else out


def kmeans_u8(img: torch.Tensor, K=5, attempts=10, iters=10, eps=1.0, seed=0, centers0=None, return_attempt=False):
    """This build's deterministic stand-in for ``cv2.kmeans(pixels, K, None, (EPS + MAX_ITER, iters, eps), attempts,
    KMEANS_RANDOM_CENTERS)`` on the pixels of an (H, W, 3) or (N, H, W, 3) uint8 image on the GPU (OpenCV draws its centres from its
    own generator, which cannot be pinned): initial centres ``lo + u * (hi - lo)`` per channel with ``u`` drawn from
    ``numpy.random.RandomState(seed)`` (the same table for every image) or ``centers0`` ((K, 3) / (N, K, 3), ``attempts = 1``),
    float32 distances with the lowest index winning a tie, exact integer sums, a freeze flag per attempt on the device, and the
    attempt of the smallest float64 compactness (include/mstg_hip.h).  All attempts of all images run as parallel problems in
    ``6 + 2 * iters`` launches, without a host synchronisation.  Returns (labels int32 (H, W) / (N, H, W) in the order of the
    initial centres, centres float32 (K, 3) / (N, K, 3), compactness float64 () / (N,)), and with ``return_attempt`` the winning
    attempt.  K and attempts outside 1 .. 16 raise, naming the parameter."""
    single, x = _stage_u8(img, "image")
    N, H, W = x.shape[:3]
    K, attempts, iters = int(K), int(attempts), int(iters)
    lib, dev = _lib.load(), x.device
    need = lib.mstg_kmeans_workspace_bytes(N, K, attempts)
    if need == 0:  # the refusal names the parameter
        _lib.check(lib.mstg_kmeans_u8(None, N, H, W, K, attempts, iters, float(eps), None, None, None, None, None, None, None, 0, None) or -1,
                   "mstg_kmeans_u8")
    u = c0 = None
    if centers0 is not None:
        c0 = torch.as_tensor(centers0).to(device=dev, dtype=torch.float32)
        c0 = (c0.unsqueeze(0) if c0.dim() == 2 else c0).contiguous()
        if tuple(c0.shape) != (N, K, 3):
            raise RuntimeError(f"mstg_hip kmeans: expected centers0 of shape {(N, K, 3)}, got {tuple(c0.shape)}")
    else:
        table = np.random.RandomState(int(seed)).random_sample(attempts * K * 3).astype(np.float32)
        u = torch.from_numpy(table).to(dev)
    labels = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    centers = torch.empty((N, K, 3), dtype=torch.float32, device=dev)
    comp = torch.empty(N, dtype=torch.float64, device=dev)
    best = torch.empty(N, dtype=torch.int32, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.check(lib.mstg_kmeans_u8(_p(x), N, H, W, K, attempts, iters, float(eps), _p(u), _p(c0), _p(labels), _p(centers), _p(comp), _p(best),
                                  _p(ws), need, _stream()), "mstg_kmeans_u8")
    out = (labels, centers, comp, best) if return_attempt else (labels, centers, comp)
    return tuple(t[0] for t in out) if single else out


def _region_args(styled_u8, orig_u8, labels, ratios):
    single, st = _stage_u8(styled_u8, "styled image")
    o = _same_size(orig_u8, st)
    N, H, W = st.shape[:3]
    lab = _req_labels(labels, (N, H, W), st.device)
    r = np.ascontiguousarray(np.asarray(ratios, dtype=np.float64).reshape(-1))
    return single, st, o, lab, r


def region_blend_u8(styled_u8, orig_u8, labels, ratios=(0.8, 0.4, 0.6)) -> torch.Tensor:
    """The region loop of ``local_style_transfer`` (advanced_transform.py:281-301) for (H, W, 3) or (N, H, W, 3) uint8 images and
    integer labels on the GPU: ``styled * r + orig * (1 - r)`` in float64 with ``r = ratios[min(label, len(ratios) - 1)]`` (the
    reference: 0.8, 0.4, then 0.6), clipped and truncated; a negative label gives 0.  One launch."""
    single, st, o, lab, r = _region_args(styled_u8, orig_u8, labels, ratios)
    N, H, W = st.shape[:3]
    out = torch.empty_like(st)
    _lib.check(_lib.load().mstg_region_blend_u8(_p(st), _p(o), _p(lab), N, H, W, r.ctypes.data, len(r), _p(out), _stream()), "mstg_region_blend_u8")
    return out[0] if single else out


def fuse_scales_u8(outputs: torch.Tensor, weights=(0.2, 0.3, 0.5), gain=1.1) -> torch.Tensor:
    """The fusion of ``multi_scale_fusion`` (advanced_transform.py:206-215) for uint8 ``outputs`` (S, H, W, 3) or (S, N, H, W, 3)
    on the GPU, in float32 as numpy forms it: ``x / 255``, the weighted sum in the order given, ``* gain``, clip, ``* 255``,
    truncate; up to 8 scales.  One launch."""
    single = outputs.dim() == 4
    x = outputs.unsqueeze(1) if single else outputs
    if not x.is_cuda or x.dtype != torch.uint8 or x.dim() != 5 or x.shape[4] != 3 or x.shape[1] < 1:
        raise RuntimeError("mstg_hip advanced transform: expected uint8 (S, H, W, 3) or (S, N, H, W, 3) outputs on the GPU")
    x = x.contiguous()
    S, N, H, W = x.shape[:4]
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
    if len(w) != S:
        raise RuntimeError(f"mstg_hip advanced transform: {S} scales but {len(w)} weights")
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().mstg_fuse_scales_u8(_p(x), S, N, H, W, w.ctypes.data, float(gain), _p(out), _stream()), "mstg_fuse_scales_u8")
    return out[0] if single else out


def contrast_enhanced_finish(styled_u8: torch.Tensor, s_gain=1.2) -> torch.Tensor:
    """``contrast_enhanced_postprocess`` of the reference (advanced_transform.py:137-166) after the plain post-process, for an
    (H, W, 3) or (N, H, W, 3) uint8 image on the GPU: Lab, CLAHE(2.0, 8 x 8) of L, Lab -> RGB, saturation * 1.2; byte for byte
    ``hsv_gain_u8(lab2rgb_u8(lab with clahe_u8(L))))`` in TWO launches whatever N; H and W multiples of 8."""
    single, x = _stage_u8(styled_u8, "styled image")
    N, H, W = x.shape[:3]
    lib, dev = _lib.load(), x.device
    need = lib.mstg_contrast_enhanced_finish_workspace_bytes(N, H, W)  # 0: the call below names what is wrong with the shape
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    out = torch.empty_like(x)
    _lib.check(lib.mstg_contrast_enhanced_finish(_p(x), N, H, W, _p(_lab_table(dev)), _p(_lab_inverse_table(dev)), float(s_gain), 1.0, _p(out),
                                                 _p(ws), need, _stream()), "mstg_contrast_enhanced_finish")
    return out[0] if single else out


def detail_enhanced_finish(styled_u8, orig_u8, sigma=3.0, s_gain=1.2, v_gain=1.1) -> torch.Tensor:
    """``detail_enhanced_postprocess`` of the reference (advanced_transform.py:218-258) after the plain post-process, for (H, W, 3)
    or (N, H, W, 3) uint8 images on the GPU (an original of another size is resized first, Lanczos): the 8-bit grey of the
    original minus its ``GaussianBlur((0, 0), 3)`` in wrapping uint8 arithmetic, half of it added to L in float32, Lab -> RGB,
    saturation * 1.2 and value * 1.1; byte for byte the composition of the stage functions in TWO launches whatever N."""
    single, x = _stage_u8(styled_u8, "styled image")
    o = _same_size(orig_u8, x)
    N, H, W = x.shape[:3]
    lib, dev = _lib.load(), x.device
    ksize, taps, _ = gaussian_sigma_taps(float(sigma))
    ws = torch.empty(N * H * W, dtype=torch.int16, device=dev)
    out = torch.empty_like(x)
    _lib.check(lib.mstg_detail_enhanced_finish(_p(x), _p(o), N, H, W, _p(_lab_table(dev)), _p(_lab_inverse_table(dev)), taps.ctypes.data, ksize,
                                               float(s_gain), float(v_gain), _p(out), _p(ws), ws.numel() * 2, _stream()),
               "mstg_detail_enhanced_finish")
    return out[0] if single else out


def local_regions_finish(styled_u8, orig_u8, seed=0, ratios=(0.8, 0.4, 0.6), s_gain=1.2) -> torch.Tensor:
    """``local_style_transfer`` of the reference (advanced_transform.py:261-311) after the plain post-process, for (H, W, 3) or
    (N, H, W, 3) uint8 images on the GPU: ``kmeans_u8(orig)`` with the reference's K = 5, 10 attempts, 10 iterations and eps 1.0
    (this build's deterministic centres from ``seed``, not OpenCV's), then the region blend and saturation * 1.2 in one launch:
    27 launches whatever N, byte for byte ``hsv_gain_u8(region_blend_u8(styled, orig, labels))``."""
    single, st = _stage_u8(styled_u8, "styled image")
    o = _same_size(orig_u8, st)
    lab = kmeans_u8(o, seed=seed)[0]
    r = np.ascontiguousarray(np.asarray(ratios, dtype=np.float64).reshape(-1))
    N, H, W = st.shape[:3]
    out = torch.empty_like(st)
    _lib.check(_lib.load().mstg_region_blend_gain_u8(_p(st), _p(o), _p(lab), N, H, W, r.ctypes.data, len(r), float(s_gain), 1.0, _p(out),
                                                     _stream()), "mstg_region_blend_gain_u8")
    return out[0] if single else out


def process_advanced(model, img_u8: torch.Tensor, setting, seed=0) -> torch.Tensor:
    """``generate_with_different_settings`` of the reference (advanced_transform.py:38-107) for ONE setting without the file I/O:
    decoded uint8 (H, W, 3) image in, (256, 256, 3) uint8 image out.  ``setting``: 'standard' (the plain post-process), 'contrast'
    (``contrast_enhanced_finish``), 'multi_scale' (the original at 0.5, 0.75 and 1.0 of its size by LANCZOS, each resized to
    256 x 256, three forward passes of one image each, ``fuse_scales_u8``; a batch of three does not give the bytes of three single
    passes (measured in tests/test_gpu_advanced_transform.py), so the three run singly as in the reference), 'detail' (``detail_enhanced_finish`` with the original
    resized by LANCZOS) and 'regions' (``local_regions_finish``, ``seed`` for the K-means).  ``Resize((256, 256))`` is
    ``resize_u8(..., BILINEAR)``.  Not built: the random ``ColorJitter(brightness=0.1, contrast=0.2)`` on the input of the
    'contrast' setting (a caller passes a jittered image if it wants one) and the matplotlib comparison chart."""
    if setting not in ADVANCED_SETTINGS:
        raise ValueError(f"mstg_hip advanced transform: setting {setting!r} is none of {ADVANCED_SETTINGS}")
    img = _req_u8(img_u8)
    height, width = img.shape[:2]
    if setting == "multi_scale":
        inputs = [resize_u8(resize_u8(img, (int(width * s), int(height * s)), LANCZOS), (256, 256), BILINEAR) for s in (0.5, 0.75, 1.0)]
    else:
        inputs = [resize_u8(img, (256, 256), BILINEAR)]
    with torch.no_grad():
        outs = [to_u8(model(to_tensor(i).unsqueeze(0))[0]) for i in inputs]
    if setting == "multi_scale":
        return fuse_scales_u8(torch.stack(outs))
    styled = outs[0]
    if setting == "standard":
        return styled
    if setting == "contrast":
        return contrast_enhanced_finish(styled)
    orig = resize_u8(img, (256, 256), LANCZOS)
    return detail_enhanced_finish(styled, orig) if setting == "detail" else local_regions_finish(styled, orig, seed)


# ---- the display finish of the reference's m_test.py (csrc/display_finish.hip) -------------------------------------------------------
def gamma_u8(y: torch.Tensor, gamma=1.1) -> torch.Tensor:
    """The head of ``process_image`` (m_test.py:58-71) on the GPU: (3, H, W) or (N, 3, H, W) float32 / float16 generator output ->
    (N, H, W, 3) uint8: ``v = y * 0.5 + 0.5`` in float32, clamped to [0, 1] (this build's: the reference raises a negative value to
    the power and casts the NaN; here a NaN gives 0), ``(float)pow((double)v, gamma)``, ``* 255`` in float32, truncated.  One launch."""
    if not isinstance(y, torch.Tensor) or not y.is_cuda or y.dim() not in (3, 4) or y.shape[-3] != 3:
        raise RuntimeError("mstg_hip image: expected a (3, H, W) or (N, 3, H, W) tensor on the GPU")
    if y.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f"mstg_hip image: gamma_u8 takes float32 or float16, got {y.dtype}")
    x = (y.unsqueeze(0) if y.dim() == 3 else y).contiguous()
    if x.shape[0] < 1:
        raise RuntimeError("mstg_hip image: gamma_u8 needs at least one image")
    N, _, H, W = x.shape
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().mstg_gamma_u8(_p(x), int(x.dtype == torch.float16), N, H, W, float(gamma), _p(out), _stream()), "mstg_gamma_u8")
    return out


def equalize_luma_u8(img_u8: torch.Tensor) -> torch.Tensor:
    """``cv2.cvtColor(img, COLOR_RGB2YUV)``, ``cv2.equalizeHist`` of Y, ``cv2.cvtColor(..., COLOR_YUV2RGB)`` (m_test.py:71-73) of an
    (H, W, 3) or (N, H, W, 3) uint8 image on the GPU, each image with its own histogram: OpenCV's 8-bit integer paths as
    include/mstg_hip.h defines them; three launches whatever N.  Restated as recalled, not compared with an OpenCV binary."""
    single, x = _stage_u8(img_u8, "image")
    N, H, W = x.shape[:3]
    lib = _lib.load()
    out = torch.empty_like(x)
    nbytes = lib.mstg_equalize_luma_workspace_bytes(N, H, W)  # 0 for a bad shape: the call below names what is wrong
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.int32, device=x.device)  # the query counts whole ints: not a byte of slack
    _lib.check(lib.mstg_equalize_luma_u8(_p(x), N, H, W, _p(out), _p(ws), ws.numel() * 4, _stream()), "mstg_equalize_luma_u8")
    return out[0] if single else out


def display_finish(y: torch.Tensor, gamma=1.1) -> torch.Tensor:
    """``process_image`` of the reference's m_test.py (:52-78) up to its bytes: ``equalize_luma_u8(gamma_u8(y, gamma))``, (N, H, W, 3)
    uint8 for (3, H, W) or (N, 3, H, W) generator output; four launches whatever N.  The reference's ``/ 255.0`` is the caller's."""
    return equalize_luma_u8(gamma_u8(y, gamma))
