"""The memory contract of include/mstg_hip.h on the 8-bit image side: the existing parity tests of image.hip, image_batch.hip,
standard_mode.hip, local_style.hip, app_local_style.hip, color_blocks.hip, advanced_transform.hip, segment_style.hip, slic.hip,
quickshift.hip, metrics.hip, compare.hip, frechet.hip and display_finish.hip, run again inside guard_helpers.memory_contract.

The pattern is that of test_gpu_memory_contract.py: each case calls an existing test body as a plain function, so its reference
and its bar -- byte for byte nearly everywhere -- stay that test's own, and a stray 0xFF or 0x7FC1 byte in a result fails it by
itself.  What the guard adds is described there: red zones around every output, workspace and upload, workspaces of exactly the
size their query named, outputs and workspaces that start as 0xFF and are never recycled memory, uploads compared with their host
copy afterwards, and -- align16 -- every one of them 16 bytes past a 256-byte boundary.  mstg_hip/image.py and metrics.py allocate
their workspaces with torch.empty, so workspaces count as outputs here.

Four things differ from the hot-path file.

* Which C entries ran.  Every case declares the entries it is there for, and the guarded test checks that they were called:
  ``mstg_hip._lib.load`` is monkeypatched for the duration of the case to return a recording proxy of the loaded library (image.py
  and metrics.py call ``_lib.load()`` at every use and keep no library object of their own, so the proxy reaches every call).
  test_every_image_entry_is_covered_or_exempt (no GPU needed) derives the image-side entries from the extern "C" definitions of
  the files above and requires each to be declared by a case or listed in EXEMPT with its reason.
* The tests' own sentinel buffers.  Many of these tests call a C entry directly on ``torch.full((n + 64,), 7)`` and assert that
  the last 64 bytes survive; the guard does not patch torch.full.  For the duration of a case torch.full / torch.full_like for the
  device go through torch.empty (+ fill_), and the ``_guarded`` helpers of the test modules through torch.empty with only the 64
  sentinel bytes written, so that the same buffers stand between red zones, at the guard's alignment, and -- for ``_guarded`` --
  start as 0xFF.  The tests themselves are unchanged and keep their sentinel assertions.
* Tests that already open a memory_contract of their own (test_gpu_quickshift.py, test_gpu_compare.py): contexts do not nest, so
  for the duration of a case their ``memory_contract`` name yields the case's guard instead.
* Device tables that image.py caches (coefficients, look-up tables) are rebuilt inside every case, so that they are guarded
  uploads at the case's alignment as well.

Inputs that a test takes from a fixture are requested from the same fixtures (imported below); the fixtures used here return
host arrays, and the one that returns device tensors (``images`` of test_gpu_image_batch.py) is replaced by uploads of ``arrays``
inside the guard.  Shapes are the smallest of each test's table that still reach ragged tiles, one-row and one-column strips,
the 1 x 1 image and batches whose second image starts on an odd byte ((67, 93), (37, 53), (17, 65) and (5, 3) times three
bytes are odd); nothing that captures a graph, starts a process, counts launches, expects a refusal or runs a real network is
wrapped, and test_mixed_batch_in_one_call runs with its fp32 stub only (its fp16 variant is the one case that would reach an fp16
network path).  The large CLAHE tiling (256 x 256) stays in the original: 64 x 64 and 40 x 72 take the same tiled route.
"""
import contextlib
import os
import re
import types

import numpy as np
import pytest
import torch

import quickshift_ref as QR
import test_gpu_advanced_transform as tadv
import test_gpu_app_local_style as tapp
import test_gpu_color_blocks as tcb
import test_gpu_compare as tcmp
import test_gpu_enhanced_local_style as tels
import test_gpu_image as timg
import test_gpu_image_batch as tib
import test_gpu_local_style as tls
import test_gpu_local_style_finish as tlsf
import test_gpu_m_test as tmt
import test_gpu_metrics as tmet
import test_gpu_quickshift as tqs
import test_gpu_slic as tslic
import test_gpu_standard_mode as tsm
from conftest import PKG
from guard_helpers import memory_contract
from oracle import image_ref as IR
# the fixtures of the wrapped tests, under names that do not collide: every one returns host arrays
from test_gpu_color_blocks import chain_inputs as color_block_chain_inputs  # noqa: F401
from test_gpu_compare import mixed as compare_mixed  # noqa: F401
from test_gpu_image_batch import arrays, cyclegan_refs  # noqa: F401
from test_gpu_local_style import full_refs  # noqa: F401
from test_gpu_local_style_finish import canvas_cases  # noqa: F401
from test_gpu_standard_mode import chain_inputs as standard_chain_inputs  # noqa: F401

DEV = "cuda:0"
IMAGE_SOURCES = ("image", "image_batch", "standard_mode", "local_style", "app_local_style", "color_blocks", "advanced_transform",
                 "segment_style", "slic", "quickshift", "metrics", "compare", "frechet", "display_finish")

# The only cases that run with check_inputs=False: the operation's contract is to write an argument the test uploaded.
# wrapped test -> what it writes in place.  None of the image-side entries does.
WRITES_AN_ARGUMENT = {}

HOST_ONLY = "host only, touches no device memory"
EXEMPT = {
    "mstg_resample_ksize": HOST_ONLY,
    "mstg_resample_coeffs": HOST_ONLY,
    "mstg_img_batch_validate": HOST_ONLY,
    "mstg_img_batch_tiles": HOST_ONLY,
    "mstg_bilateral_tables": HOST_ONLY,
    "mstg_standard_color_lut": HOST_ONLY,
    "mstg_gaussian_kernel_f64": HOST_ONLY,
    "mstg_lab_tables": HOST_ONLY,
    "mstg_bilateral_wide_tables": HOST_ONLY,
    "mstg_lab_inverse_tables": HOST_ONLY,
    "mstg_gaussian_sigma_taps": HOST_ONLY,
    "mstg_felzenszwalb_u8": HOST_ONLY,
    "mstg_slic_grid": HOST_ONLY,
    "mstg_cv_resize_coeffs": HOST_ONLY,
    "mstg_pair_metrics_validate": HOST_ONLY,
    "mstg_pair_metrics_tiles": HOST_ONLY,
}


def image_entries():
    """the image-side C entries: the extern "C" definitions of IMAGE_SOURCES that mstg_hip/_lib.py binds"""
    from mstg_hip import _lib
    names = set()
    for stem in IMAGE_SOURCES:
        with open(os.path.join(PKG, "mstg_hip", "csrc", stem + ".hip")) as f:
            names.update(re.findall(r'extern\s+"C"\s+[\w\s\*]*?\b(mstg_\w+)\s*\(', f.read()))
    return names & set(_lib.SIGNATURES)


class _Recorder:
    """the loaded library, with the name of every mstg_* function that is called through it"""

    def __init__(self, lib):
        self._lib, self.called = lib, set()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("mstg_"):
            return fn

        def call(*args):
            self.called.add(name)
            return fn(*args)
        return call


def _sentinel_buffers_through_empty(monkeypatch):
    """see the docstring: the tests' torch.full sentinel buffers, allocated where the guard reaches them"""
    full, full_like = torch.full, torch.full_like

    def guarded_full(size, fill_value, **kw):
        if "dtype" not in kw or set(kw) - {"dtype", "device"} or torch.device(kw.get("device", "cpu")).type != "cuda":
            return full(size, fill_value, **kw)
        return torch.empty((size,) if isinstance(size, int) else tuple(size), **kw).fill_(fill_value)

    def guarded_full_like(x, fill_value, **kw):
        if kw or not x.is_cuda:
            return full_like(x, fill_value, **kw)
        return torch.empty_like(x).fill_(fill_value)

    def guarded(nbytes):
        buf = torch.empty(nbytes + 64, dtype=torch.uint8, device=DEV)
        buf[nbytes:] = 7
        return buf
    monkeypatch.setattr(torch, "full", guarded_full)
    monkeypatch.setattr(torch, "full_like", guarded_full_like)
    for mod in (tcb, tels, tslic, tmt):
        assert mod.GUARD == 64
        monkeypatch.setattr(mod, "_guarded", guarded)


CASES = []


def case(ident, key, fn, entries):
    """ident: pytest id; key: name of the wrapped test (the key of WRITES_AN_ARGUMENT); fn(fx) runs it, fx.get(name) is the value of a
    fixture; entries: the C entries the case is there for, each of which must be called while it runs"""
    CASES.append(pytest.param(key, fn, tuple(entries), id=ident))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- image.hip ---------------------------------------------------------------------------------------------------------------------
RESAMPLE = ("mstg_resample_h_u8", "mstg_resample_v_u8")
for filt in (IR.BILINEAR, IR.LANCZOS):
    for shape, size in (((97, 301), (256, 82)), ((64, 48), (256, 341))):  # both axes down; both axes up
        case(f"resize-filter{filt}-{shape}->{size}", "test_resize_bit_exact",
             lambda fx, f=filt, s=shape, z=size: timg.test_resize_bit_exact(f, s, z), RESAMPLE)
case("output-conversion", "test_output_conversion_bit_exact", lambda fx: timg.test_output_conversion_bit_exact(), ["mstg_tensor_to_u8"])
for strength in (0.8, 1.0 / 3.0):
    case(f"blend-simple-{strength:.3f}", "test_blend_simple_bit_exact", lambda fx, s=strength: timg.test_blend_simple_bit_exact(s), ["mstg_blend_u8"])
case("blend-weight-map", "test_blend_weight_map_bit_exact", lambda fx: timg.test_blend_weight_map_bit_exact(), ["mstg_blend_u8"])
case("dataset-item", "test_dataset_item_bit_exact_and_mask_stream", lambda fx: timg.test_dataset_item_bit_exact_and_mask_stream(),
     RESAMPLE + ("mstg_u8_to_tensor",))


def _paste_and_crop(shape):
    """mstg_paste_u8 has no test of its own without a network around it (letterbox and the crop back of process_cyclegan): the
    window of an image pasted onto a filled canvas, and Image.crop, byte for byte against numpy slicing"""
    from mstg_hip import image as dimg
    h, w = shape
    img = timg._img(h, w, 91)
    x = _dev(img)
    y0, x0, wh, ww = h // 3, w // 4, h - h // 3, w - w // 4  # an odd offset into the source, down to its last row and column
    for (dh, dw), (ay, ax), fill in (((wh + 5, ww + 3), (2, 1), 255), ((wh, ww), (0, 0), 0), ((wh + 1, ww + 64), (1, 61), 17)):
        want = np.full((dh, dw, 3), fill, dtype=np.uint8)
        want[ay:ay + wh, ax:ax + ww] = img[y0:y0 + wh, x0:x0 + ww]
        got = dimg.paste_u8(x, (y0, x0, wh, ww), (dh, dw), (ay, ax), fill=fill).cpu().numpy()
        assert np.array_equal(got, want), f"paste {shape} -> {(dh, dw)} at {(ay, ax)}: {int((got != want).sum())} bytes differ"
    got = dimg.crop_u8(x, x0, y0, w, h).cpu().numpy()
    assert np.array_equal(got, img[y0:, x0:])


for shape in ((1, 1), (1, 9), (7, 1), (67, 93)):
    case(f"paste-{shape}", "_paste_and_crop", lambda fx, s=shape: _paste_and_crop(s), ["mstg_paste_u8"])

# ---- image_batch.hip ---------------------------------------------------------------------------------------------------------------
BATCH = ("mstg_img_batch_resample_h", "mstg_img_batch_resample_v_tensor", "mstg_img_batch_resample_v_u8", "mstg_img_batch_tensor_to_u8")


def _images(fx):
    """the ``images`` fixture of test_gpu_image_batch.py, uploaded inside the guard"""
    return [_dev(a) for a in fx.get("arrays")]


case("batch-mixed-fp32", "test_mixed_batch_in_one_call",
     lambda fx: tib.test_mixed_batch_in_one_call(_images(fx), fx.get("cyclegan_refs"), "fp32"), BATCH)
for mode, strength in (("simple", 0.8), ("simple", 1.0 / 3.0), ("weight_map", None), ("styled", None)):
    case(f"batch-local-style-{mode}-{strength}", "test_local_style_same_batch",
         lambda fx, m=mode, s=strength: tib.test_local_style_same_batch(fx.get("arrays"), _images(fx), m, s),
         BATCH + (("mstg_blend_u8",) if mode != "styled" else ()))
case("batch-dataset", "test_dataset_batch", lambda fx: tib.test_dataset_batch(), BATCH[:2])

# ---- standard_mode.hip -------------------------------------------------------------------------------------------------------------
for shape in ((1, 1), (1, 7), (67, 93)):
    case(f"standard-median-{shape}", "test_median", lambda fx, s=shape: tsm.test_median(s), ["mstg_median3_u8"])
for params in tsm.BILATERAL_PARAMS:
    for shape in ((1, 1), (3, 5), (67, 93)):
        case(f"standard-bilateral-{params}-{shape}", "test_bilateral", lambda fx, s=shape, p=params: tsm.test_bilateral(s, p), ["mstg_bilateral_u8"])
for ksize in (3, 5, 7):
    for shape in ((1, 1), (3, 5), (67, 93)):
        case(f"standard-blur-{ksize}-{shape}", "test_blur", lambda fx, s=shape, k=ksize: tsm.test_blur(s, k), ["mstg_gaussian_u8"])
for model_type in tsm.SR.MODEL_TYPES:
    case(f"standard-lookup-{model_type}", "test_table_lookup_all_values", lambda fx, m=model_type: tsm.test_table_lookup_all_values(m),
         ["mstg_lut_u8"])
for fix_blocks in (True, False):
    for blend_ratio in (0, 0.3):
        case(f"standard-chain-blend{blend_ratio}-fix{int(fix_blocks)}", "test_chain_equals_the_composed_stages",
             lambda fx, b=blend_ratio, f=fix_blocks: tsm.test_chain_equals_the_composed_stages(fx.get("standard_chain_inputs"), b, f),
             ["mstg_standard_finish", "mstg_standard_finish_workspace_bytes", "mstg_lut_u8", "mstg_gaussian_u8"])

# ---- local_style.hip ---------------------------------------------------------------------------------------------------------------
STAGES = ("mstg_local_style_prepare", "mstg_local_style_hysteresis", "mstg_local_style_weights")
for kind in ("noise", "blocky", "gradient_rects"):
    case(f"local-style-state-map-{kind}", "test_state_map", lambda fx, k=kind: tls.test_state_map(k, (67, 93)), ["mstg_local_style_prepare"])
for pair in ("spirals", "serpentine_diagonal", "candidates_random"):
    case(f"local-style-hysteresis-{pair}", "test_hysteresis_crafted_maps", lambda fx, p=pair: tls.test_hysteresis_crafted_maps(p, (48, 64)),
         ["mstg_local_style_hysteresis"])
case("local-style-sky-threshold", "test_sky_threshold", lambda fx: tls.test_sky_threshold(), STAGES)
for strength, detail, coeff in ((0.8, 0.7, 0.3), (0.1, 0.7, 0.4)):
    case(f"local-style-full-map-{strength}-{detail}-{coeff}", "test_full_map",
         lambda fx, s=strength, d=detail, c=coeff: tls.test_full_map(fx.get("full_refs"), s, d, c, (96, 80)),
         STAGES + ("mstg_local_style_weight_map", "mstg_local_style_workspace_bytes"))
for kinds in (("pixels", "frame", "checker"), ("random", "checker", "pixels")):
    for shape in ((1, 1), (2, 5), (7, 9), (tlsf.TILE_H + 1, tlsf.TILE_W + 1)):
        case(f"local-style-finish-{kinds[0]}-{shape}", "test_smoothing_on_crafted_masks",
             lambda fx, k=kinds, s=shape: tlsf.test_smoothing_on_crafted_masks(k, s), ["mstg_local_style_finish"])
case("local-style-enhanced-(96, 80)", "test_enhanced_from_the_canvas",
     lambda fx: tlsf.test_enhanced_from_the_canvas(fx.get("canvas_cases"), (96, 80)),
     ["mstg_local_style_enhanced", "mstg_local_style_enhanced_workspace_bytes"])

# ---- app_local_style.hip -----------------------------------------------------------------------------------------------------------
for shape in tapp.SHAPES[:4]:  # (1, 1), (1, 9), (5, 3), (37, 70)
    case(f"app-sky-mask-{shape}", "test_sky_mask", lambda fx, s=shape: tapp.test_sky_mask(s), ["mstg_app_sky_mask"])
    case(f"app-edge-weight-{shape}", "test_edge_weight_bit_for_bit", lambda fx, s=shape: tapp.test_edge_weight_bit_for_bit(s),
         ["mstg_app_edge_weight"])
case("app-chain-(5, 3)", "test_chain_every_flag_combination", lambda fx: tapp.test_chain_every_flag_combination((5, 3)), ["mstg_app_chain"])
for model_type in tapp.MODEL_TYPES:
    case(f"app-finish-{model_type}", "test_finish_equals_the_composed_stages",
         lambda fx, m=model_type: tapp.test_finish_equals_the_composed_stages(m),
         ["mstg_app_local_style_finish", "mstg_app_local_style_workspace_bytes", "mstg_app_chain", "mstg_app_edge_weight", "mstg_bilateral_u8"])

# ---- color_blocks.hip --------------------------------------------------------------------------------------------------------------
for shape in ((1, 1), (1, 9), (7, 5), (67, 93)):
    case(f"color-blocks-mask-{shape}", "test_mask", lambda fx, s=shape: tcb.test_mask(s), ["mstg_color_block_mask"])
for shape in ((1, 1), (30, 40)):
    case(f"color-blocks-correction-{shape}", "test_correction", lambda fx, s=shape: tcb.test_correction(s), ["mstg_color_correct_u8"])
for d in (3, 5, 7, 9):
    case(f"color-blocks-wide-d{d}", "test_wide_equals_the_existing_kernel", lambda fx, d=d: tcb.test_wide_equals_the_existing_kernel(d),
         ["mstg_bilateral_wide_u8", "mstg_bilateral_u8"])
case("color-blocks-wide-radius12-(6, 261)", "test_wide_radius_12", lambda fx: tcb.test_wide_radius_12((6, 261)), ["mstg_bilateral_wide_u8"])
for shape in ((1, 1), (7, 5), (40, 33)):
    case(f"color-blocks-wide-radius90-{shape}", "test_wide_radius_90_whole_images", lambda fx, s=shape: tcb.test_wide_radius_90_whole_images(s),
         ["mstg_bilateral_wide_u8"])
for shape in ((1, 1), (5, 7), (67, 93)):
    case(f"color-blocks-detail-blend-{shape}", "test_detail_blend", lambda fx, s=shape: tcb.test_detail_blend(s), ["mstg_detail_blend_u8"])
for with_orig in (False, True):
    case(f"color-blocks-chain-orig{int(with_orig)}", "test_chain_equals_the_composed_stages",
         lambda fx, w=with_orig: tcb.test_chain_equals_the_composed_stages(fx.get("color_block_chain_inputs"), w),
         ["mstg_color_block_fix", "mstg_color_block_fix_workspace_bytes", "mstg_color_block_mask", "mstg_color_correct_u8", "mstg_bilateral_wide_u8"]
         + (["mstg_detail_blend_u8"] if with_orig else []))

# ---- advanced_transform.hip --------------------------------------------------------------------------------------------------------
for shape, n in tadv.SHAPES:
    case(f"advanced-lab-{shape}-n{n}", "test_lab_round_trip_and_gains", lambda fx, s=shape, n=n: tadv.test_lab_round_trip_and_gains(s, n),
         ["mstg_lab_u8", "mstg_lab2rgb_u8", "mstg_hsv_gain_u8"])
case("advanced-lab2rgb-table", "test_lab2rgb_on_a_table_of_triples", lambda fx: tadv.test_lab2rgb_on_a_table_of_triples(), ["mstg_lab2rgb_u8"])
for shape, n in (((37, 53), 1), ((5, 3), 1), ((17, 65), 3), ((1, 7), 2), ((7, 1), 1), ((1, 1), 1)):
    case(f"advanced-gaussian-sigma-{shape}-n{n}", "test_gaussian_sigma", lambda fx, s=shape, n=n: tadv.test_gaussian_sigma(s, n),
         ["mstg_gaussian_sigma_u8"])
KMEANS = ("mstg_kmeans_u8", "mstg_kmeans_workspace_bytes")
case("advanced-kmeans", "test_kmeans_solo_batch_and_winner", lambda fx: tadv.test_kmeans_solo_batch_and_winner(), KMEANS)
case("advanced-kmeans-edges", "test_kmeans_edge_cases", lambda fx: tadv.test_kmeans_edge_cases(), KMEANS)
for shape, n in (((37, 53), 1), ((5, 3), 1), ((17, 65), 3)):
    case(f"advanced-region-blend-fusion-{shape}-n{n}", "test_region_blend_and_fusion",
         lambda fx, s=shape, n=n: tadv.test_region_blend_and_fusion(s, n),
         ["mstg_region_blend_u8", "mstg_fuse_scales_u8"])
for n in (1, 3):
    case(f"advanced-chains-(40, 72)-n{n}", "test_chains_equal_their_stages", lambda fx, n=n: tadv.test_chains_equal_their_stages((40, 72), n),
         ("mstg_contrast_enhanced_finish", "mstg_contrast_enhanced_finish_workspace_bytes", "mstg_detail_enhanced_finish",
          "mstg_region_blend_gain_u8", "mstg_clahe_u8", "mstg_clahe_workspace_bytes", "mstg_gaussian_sigma_u8") + KMEANS)

# ---- segment_style.hip -------------------------------------------------------------------------------------------------------------
SEGMENT_MAP = ("mstg_segment_blend_map", "mstg_segment_blend_map_workspace_bytes")
for kind in ("one", "grid", "gaps", "outside", "borders"):
    case(f"segment-map-{kind}-(37, 53)", "test_segment_map", lambda fx, k=kind: tels.test_segment_map((37, 53), k), SEGMENT_MAP)
for extra in (0, 1, tels.TILE_SLOTS):
    case(f"segment-map-tile-slots+{extra}", "test_segment_map_around_the_tile_slot_limit",
         lambda fx, e=extra: tels.test_segment_map_around_the_tile_slot_limit(e), SEGMENT_MAP)
for shape in ((37, 53), (5, 3)):
    case(f"segment-gaussian-{shape}", "test_gaussian", lambda fx, s=shape: tels.test_gaussian(s), ["mstg_gaussian_reflect_f32"])
case("segment-blend-(37, 53)", "test_blend", lambda fx: tels.test_blend((37, 53)), ["mstg_blend_map_f32_u8"])
for shape in ((37, 53), (2, 2)):
    case(f"segment-sharpen-{shape}", "test_sharpen", lambda fx, s=shape: tels.test_sharpen(s), ["mstg_sharpen3_u8"])
for shape, n in tels.TILED[:2]:
    case(f"segment-clahe-{shape}", "test_clahe", lambda fx, s=shape, n=n: tels.test_clahe(s, n), ["mstg_clahe_u8", "mstg_clahe_workspace_bytes"])
    case(f"segment-hsv-enhance-{shape}", "test_hsv_enhance", lambda fx, s=shape, n=n: tels.test_hsv_enhance(s, n),
         ["mstg_hsv_enhance_u8", "mstg_clahe_workspace_bytes"])
    case(f"segment-chain-{shape}", "test_chain_equals_the_restatement_and_the_stages",
         lambda fx, s=shape, n=n: tels.test_chain_equals_the_restatement_and_the_stages(s, n),
         ["mstg_enhanced_style_finish", "mstg_enhanced_style_finish_workspace_bytes", "mstg_blend_map_f32_u8", "mstg_hsv_enhance_u8",
          "mstg_sharpen3_u8", "mstg_bilateral_u8"])

# ---- slic.hip ----------------------------------------------------------------------------------------------------------------------
for name in ("smooth", "noise", "flat", "blocks96"):  # 37 x 53, 40 x 70, 64 x 48, 96 x 80
    case(f"slic-{name}", "test_assign_and_labels_equal_the_restatement", lambda fx, n=name: tslic.test_assign_and_labels_equal_the_restatement(n),
         ["mstg_slic_assign_u8", "mstg_slic_u8", "mstg_slic_workspace_bytes"])
CONNECT = ("mstg_connect_labels", "mstg_connect_labels_workspace_bytes")
for shape in ((1, 70), (70, 1), (1, 1)):
    case(f"connect-strip-{shape}", "test_connect_strips", lambda fx, s=shape: tslic.test_connect_strips(s), CONNECT)
case("connect-serpentine", "test_connect_serpentine", lambda fx: tslic.test_connect_serpentine(), CONNECT)
case("connect-checkerboard", "test_connect_checkerboard", lambda fx: tslic.test_connect_checkerboard(), CONNECT)
case("connect-tile-corners", "test_connect_components_across_tile_corners", lambda fx: tslic.test_connect_components_across_tile_corners(), CONNECT)

# ---- quickshift.hip ----------------------------------------------------------------------------------------------------------------
RUNS = {name: (name, params) for name, params in QR.RUNS if params == QR.REFERENCE_PARAMS}
for name in ("one", "flat_small", "strip_h", "strip_w", "smooth"):  # 1 x 1, 7 x 11, 1 x 70, 70 x 1, 37 x 53
    case(f"quickshift-density-{name}", "test_density_is_within_the_tap_count_of_the_restatement",
         lambda fx, r=RUNS[name]: tqs.test_density_is_within_the_tap_count_of_the_restatement(r), ["mstg_quickshift_density_u8"])
    case(f"quickshift-parents-{name}", "test_parents_of_the_restatements_density_equal_the_restatements",
         lambda fx, r=RUNS[name]: tqs.test_parents_of_the_restatements_density_equal_the_restatements(r), ["mstg_quickshift_parents_u8"])
    case(f"quickshift-labels-{name}", "test_labels_equal_the_restatement_on_the_devices_density",
         lambda fx, r=RUNS[name]: tqs.test_labels_equal_the_restatement_on_the_devices_density(r),
         ["mstg_quickshift_u8", "mstg_quickshift_workspace_bytes", "mstg_quickshift_density_u8"])
case("quickshift-flat", "test_a_flat_image_is_one_segment_wherever_its_tiles_fall",
     lambda fx: tqs.test_a_flat_image_is_one_segment_wherever_its_tiles_fall(),
     ["mstg_quickshift_u8", "mstg_quickshift_workspace_bytes", "mstg_quickshift_density_u8"])

# ---- metrics.hip, compare.hip ------------------------------------------------------------------------------------------------------
METRICS = ("mstg_image_metrics_u8", "mstg_image_metrics_workspace_bytes")
for shape in tmet.SHAPES[:5]:  # (7, 7), (7, 40), (40, 7), (8, 9), (23, 37)
    case(f"metrics-{shape}", "test_shapes_and_pair_kinds_against_the_oracle",
         lambda fx, s=shape: tmet.test_shapes_and_pair_kinds_against_the_oracle(s), METRICS)
case("metrics-batch-of-three", "test_batch_of_three_different_pairs_and_bit_identity",
     lambda fx: tmet.test_batch_of_three_different_pairs_and_bit_identity(), METRICS)
for src, dst in (((1, 1), (7, 7)), ((2, 3), (9, 8)), ((22, 36), (11, 18)), ((129, 67), (8, 9))):  # the smallest two up, the smallest two down
    case(f"cv-resize-{src}->{dst}", "test_cv_resize_matches_the_restatement",
         lambda fx, s=src, d=dst: tcmp.test_cv_resize_matches_the_restatement(s, d),
         ["mstg_cv_resize_linear_u8"])
case("cv-resize-batch-of-three", "test_cv_resize_batch_of_three_equals_the_single_calls",
     lambda fx: tcmp.test_cv_resize_batch_of_three_equals_the_single_calls(), ["mstg_cv_resize_linear_u8"])
case("pair-metrics-one-call", "test_pair_metrics_one_call_is_the_composition_bit_for_bit",
     lambda fx: tcmp.test_pair_metrics_one_call_is_the_composition_bit_for_bit(fx.get("compare_mixed")),
     ("mstg_pair_metrics_u8", "mstg_pair_metrics_workspace_bytes", "mstg_cv_resize_linear_u8") + METRICS)

# ---- frechet.hip, display_finish.hip -----------------------------------------------------------------------------------------------
FRECHET = ("mstg_frechet_distance", "mstg_frechet_workspace_bytes")
for shape in tmt.FR.CASES[:2]:  # (2, 2, 1), (7, 5, 3)
    for dtype in ("float32", "float64"):
        case(f"frechet-{shape}-{dtype}", "test_frechet_equals_the_float64_restatement",
             lambda fx, s=shape, t=dtype: tmt.test_frechet_equals_the_float64_restatement(s, t), FRECHET)
case("frechet-constant-column", "test_frechet_constant_column_and_identical_sets",
     lambda fx: tmt.test_frechet_constant_column_and_identical_sets(), FRECHET)
for shape in ((1, 1), (1, 5), (5, 1), (7, 5), (5, 7), (130, 128)):  # the smallest, and the first shape that lives in the workspace
    case(f"singular-values-{shape}", "test_singular_values_equal_numpy", lambda fx, s=shape: tmt.test_singular_values_equal_numpy(s),
         ["mstg_singular_values", "mstg_singular_values_workspace_bytes"])
for name in ("1x1", "37x53", "three histograms", "constant", "one row"):
    case(f"equalize-luma-{name}", "test_equalize_luma_equals_the_restatement", lambda fx, n=name: tmt.test_equalize_luma_equals_the_restatement(n),
         ["mstg_equalize_luma_u8", "mstg_equalize_luma_workspace_bytes"])
for seed, shape, dtype in tmt.GAMMA_CASES[:4]:
    case(f"gamma-display-finish-{shape}-{dtype}", "test_gamma_and_display_finish_equal_the_restatement",
         lambda fx, a=(seed, shape, dtype): tmt.test_gamma_and_display_finish_equal_the_restatement(*a),
         ["mstg_gamma_u8", "mstg_equalize_luma_u8", "mstg_equalize_luma_workspace_bytes"])


@pytest.fixture(scope="module")
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    return _lib.load()  # raises if the HIP library is missing -- there is no fallback to test instead


@pytest.mark.gpu
@pytest.mark.parametrize("align16", [False, True], ids=["align256", "align16"])
@pytest.mark.parametrize("key,fn,entries", CASES)
def test_memory_contract_image(key, fn, entries, align16, _lib_loaded, monkeypatch, request):
    from mstg_hip import _lib, image as dimg
    lib = _Recorder(_lib_loaded)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(dimg, "_dev_tables", {})
    monkeypatch.setattr(dimg, "_std_tables", {})
    monkeypatch.setattr(tqs, "_density_cache", {})
    _sentinel_buffers_through_empty(monkeypatch)
    fx = types.SimpleNamespace(monkeypatch=monkeypatch, get=request.getfixturevalue)
    with memory_contract(align16=align16, check_inputs=key not in WRITES_AN_ARGUMENT) as mc:
        for mod in (tqs, tcmp):  # contexts do not nest: the test's own guard is this one
            monkeypatch.setattr(mod, "memory_contract", lambda *a, **kw: contextlib.nullcontext(mc))
        fn(fx)
    print(f"  [guard] outputs {mc.outputs} uploads {mc.uploads} passthrough {mc.passthrough} entries {' '.join(sorted(lib.called))}")
    assert mc.outputs >= 1 and mc.uploads >= 1, (mc.outputs, mc.uploads)
    assert set(entries) <= lib.called, f"declared and not called: {sorted(set(entries) - lib.called)}"


@pytest.mark.gpu
@pytest.mark.parametrize("align16", [False, True], ids=["align256", "align16"])
def test_sentinel_buffers_stand_inside_the_guard(align16, _lib_loaded, monkeypatch):
    """The self-check of what this file adds to the guard: the wrapped tests' own sentinel buffers are allocations of the guard, at
    its alignment, a ``_guarded`` buffer starts as 0xFF in front of its 64 sentinel bytes, and every other torch.full is untouched."""
    _sentinel_buffers_through_empty(monkeypatch)
    with memory_contract(align16=align16) as mc:
        a = tslic._guarded(10)
        b = torch.full((3, 5), 9, dtype=torch.uint8, device=DEV)
        c = torch.full_like(b, 4)
        count = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        for t in (a, b, c, count):
            mc.raw(t)  # KeyError if the guard did not allocate it
            assert t.data_ptr() % 256 == (16 if align16 else 0)
        assert a.numel() == 74 and bool(a[:10].eq(255).all()) and bool(a[10:].eq(7).all())
        assert bool(b.eq(9).all()) and bool(c.eq(4).all()) and count.tolist() == [-1, -1]
        host = torch.full((2,), 1.5)
        assert not host.is_cuda and host.tolist() == [1.5, 1.5] and torch.full_like(host, 2.0).tolist() == [2.0, 2.0]
    assert (mc.outputs, mc.uploads, mc.passthrough) == (4, 0, 0)


def test_recorder_records_what_is_called():
    lib = types.SimpleNamespace(mstg_a=lambda x: x + 1, mstg_b=lambda: 0, other=5)
    rec = _Recorder(lib)
    looked_up = rec.mstg_b  # noqa: F841  (looked up, never called)
    assert rec.mstg_a(1) == 2 and rec.other == 5 and rec.called == {"mstg_a"}


def test_every_image_entry_is_covered_or_exempt():
    """every C entry of the image-side sources is declared by a guarded case or exempt with a reason, and nothing is listed that
    is not such an entry"""
    entries = image_entries()
    assert len(entries) >= 90, len(entries)  # the extern "C" pattern still finds them
    declared = set().union(*(p.values[2] for p in CASES))
    assert declared <= entries, f"declared by a case, not an image-side entry: {sorted(declared - entries)}"
    assert set(EXEMPT) <= entries, f"exempt, not an image-side entry: {sorted(set(EXEMPT) - entries)}"
    assert not declared & set(EXEMPT), sorted(declared & set(EXEMPT))
    assert all(isinstance(r, str) and (r == HOST_ONLY or r.startswith("reached only through a wrapped chain: ")) for r in EXEMPT.values())
    missing = entries - declared - set(EXEMPT)
    assert not missing, f"neither reached by a guarded case nor exempt: {sorted(missing)}"


def test_exemptions_name_wrapped_tests():
    keys = {p.values[0] for p in CASES}
    assert set(WRITES_AN_ARGUMENT) <= keys, set(WRITES_AN_ARGUMENT) - keys
