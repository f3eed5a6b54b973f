"""Drop-in for the reference's enhanced_local_style.py: the segmentation-driven local style with everything between decoding and
encoding on the GPU (mstg_hip.image, csrc/segment_style.hip) except the Felzenszwalb segmentation, which runs on the host inside
the library (``mstg_felzenszwalb_u8``).  PIL / numpy in, PIL / numpy out; Pillow decodes and encodes; ``cv2``, ``skimage`` and
``torchvision`` are not imported.

Differences from the reference, on purpose: ``get_segmentation_mask`` builds 'felzenszwalb' only ('slic' and 'quickshift' raise
NotImplementedError by name); equal edge costs of the segmentation keep their order (a stable sort; scikit-image leaves them as
numpy's unstable sort does), so labels can differ from scikit-image's where costs tie; ``analyze_segments`` reports the hue and
value means of ``avg_color_hsv`` as NaN (the device record holds the saturation sum, the only one the ratio reads); and no
comparison chart is written (the reference's ``create_comparison`` needs matplotlib); ``enhanced_local_style_transfer`` and the
command line take ``segmentation`` / ``--segmentation``: 'felzenszwalb' (the reference's choice, the default) or 'slic', the
device segmentation ``mstg_hip.image.slic_labels`` (8-bit Lab features and a connectivity step of this build's own), with which the
whole call stays on the GPU.  ``--device-segmentation {slic,quickshift}`` (``segments=`` of
``enhanced_local_style_transfer``: a callable such as ``mstg_hip.image.quickshift_segmenter()``), when given, takes the place of
``--segmentation``: that is how quickshift (``mstg_hip.image.quickshift_labels`` with the reference's kernel_size 3, max_dist 6,
ratio 0.5; a fixed-point density and a tie rule by raster index of this build's own) is reached.  It is not a value of
``--segmentation`` because that option, ``segmentation=`` and ``get_segmentation_mask`` keep refusing 'quickshift' by name, as
they did before it was built, and callers may rely on that.  The OpenCV and scikit-image steps are
restated from their definitions (include/mstg_hip.h) and have not been compared with an OpenCV or scikit-image binary.
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch
from PIL import Image

from enhanced_generator import EnhancedGenerator
from mstg_hip import image as dimg


def load_model(model_path, device, channels=16, blocks=1):
    """:14-38: the generator of a checkpoint that holds ``G_AB_state_dict`` or ``G_BA_state_dict`` -> (model, model_type)"""
    checkpoint = torch.load(model_path, map_location=device)
    if "G_AB_state_dict" in checkpoint:
        state_dict, model_type = checkpoint["G_AB_state_dict"], "G_AB"
    elif "G_BA_state_dict" in checkpoint:
        state_dict, model_type = checkpoint["G_BA_state_dict"], "G_BA"
    else:
        raise ValueError("unknown checkpoint format: neither G_AB_state_dict nor G_BA_state_dict")
    print(f"model type: {model_type}")
    model = EnhancedGenerator(channels=channels, num_transformer_blocks=blocks)
    model.load_state_dict(state_dict)
    model = model.to(device)
    model.eval()
    return model, model_type


def _u8(img, device=None):
    a = np.array(img.convert("RGB") if isinstance(img, Image.Image) else img, dtype=np.uint8)  # a writable, contiguous copy
    return torch.from_numpy(a).to(device or "cuda")


def preprocess_image(img, size=256):
    """:40-47: Resize((size, size)) -> ToTensor -> Normalize(0.5, 0.5) of a PIL image or (H, W, 3) uint8 array -> (1, 3, size, size)"""
    x = _u8(img)
    if tuple(x.shape[:2]) != (size, size):
        x = dimg.resize_u8(x, (size, size), dimg.BILINEAR)
    return dimg.to_tensor(x).unsqueeze(0)


def standard_postprocess(tensor):
    """:49-54: (1, 3, H, W) in [-1, 1] -> PIL image"""
    return Image.fromarray(dimg.to_u8(tensor[0] if tensor.dim() == 4 else tensor).cpu().numpy())


def get_segmentation_mask(img, method="felzenszwalb", n_segments=100, compactness=10):
    """:56-74: 'felzenszwalb' (scale 100, sigma 0.5, min_size 50) -> int32 (H, W); 'slic' and 'quickshift' are not built"""
    if method in ("slic", "quickshift"):
        raise NotImplementedError(f"enhanced_local_style: segmentation method {method!r} is not part of this build; "
                                  "pass your own labels to mstg_hip.image.process_enhanced_local_style(segments=...)")
    if method != "felzenszwalb":
        raise ValueError(f"unknown segmentation method: {method}")
    return dimg.felzenszwalb_labels(np.asarray(img.convert("RGB") if isinstance(img, Image.Image) else img, dtype=np.uint8))


def analyze_segments(img, segments):
    """:76-124 from the device record: {label: {'avg_color_rgb', 'avg_color_hsv', 'std_color', 'edge_density', 'size', 'position'}}
    for every label that has a pixel.  ``avg_color_hsv`` holds the saturation mean at [1] and NaN for hue and value."""
    segments = np.asarray(segments)
    _, sums, _ = dimg.segment_blend_map(_u8(img), segments, smooth=False, return_stats=True)
    H, W = segments.shape
    stats = {}
    for label, row in enumerate(sums.cpu().numpy().tolist()):
        n = row[0]
        if n == 0:
            continue
        fn = float(n)
        stats[label] = {
            "avg_color_rgb": np.array([float(row[1 + c]) / fn for c in range(3)]),
            "avg_color_hsv": np.array([np.nan, float(row[7]) / fn, np.nan]),
            "std_color": np.array([np.sqrt(float(n * row[4 + c] - row[1 + c] ** 2)) / fn for c in range(3)]),
            "edge_density": float(row[10]) / 4294967296.0 / float(H * W),  # below 2^63: exact as torch's int64
            "size": n,
            "position": np.array([float(row[8]) / fn, float(row[9]) / fn]),
        }
    return stats


def determine_blend_ratios(segment_stats, segments, img_shape):
    """:126-176: the ratio of every segment from its statistics in the order include/mstg_hip.h fixes, the map, and
    ``scipy.ndimage.gaussian_filter(map, sigma=3)`` on the GPU -> float32 numpy (H, W)"""
    segments = np.asarray(segments)
    H, W = img_shape[:2]
    center_y, center_x = H // 2, W // 2
    max_dist = float(np.sqrt(float(center_x ** 2 + center_y ** 2)))
    blend_map = np.zeros((H, W), dtype=np.float32)
    for segment_id, stats in segment_stats.items():
        sd = stats["std_color"]
        mstd = ((float(sd[0]) + float(sd[1])) + float(sd[2])) / 3.0
        pos_y, pos_x = (float(v) for v in stats["position"])
        dy, dx = pos_y - center_y, pos_x - center_x
        dist = float(np.sqrt(dy * dy + dx * dx))
        adjustment = ((((0.3 * (stats["edge_density"] / 30) + 0.2 * (mstd / 50)) - 0.1 * (dist / max_dist))
                       + (-0.1 * (float(stats["size"]) / (H * W / 100.0)))) + 0.2 * (float(stats["avg_color_hsv"][1]) / 255))
        blend_map[segments == segment_id] = max(0.3, min(0.9, 0.7 + adjustment))
    return dimg.gaussian_reflect_f32(torch.from_numpy(blend_map).to("cuda")).cpu().numpy()


def enhanced_local_style_transfer(model, img_path, output_path, device, segmentation="felzenszwalb", segments=None):
    """:178-292 without the comparison chart: decode, ``mstg_hip.image.process_enhanced_local_style``, encode -> PIL image.
    ``segmentation``: 'felzenszwalb' (on the host) or 'slic' (on the device); ``segments``: passed through (labels, or a callable
    such as ``mstg_hip.image.quickshift_segmenter()``), wins when given."""
    original = Image.open(img_path).convert("RGB")
    out = dimg.process_enhanced_local_style(model, _u8(original, device), segments=segments, segmentation=segmentation)
    final_img = Image.fromarray(out.cpu().numpy())
    if os.path.dirname(output_path):
        os.makedirs(os.path.dirname(output_path), exist_ok=True)
    final_img.save(output_path)
    print(f"saved the enhanced image to {output_path}")
    return final_img


DEVICE_SEGMENTERS = {"slic": dimg.slic_segmenter, "quickshift": dimg.quickshift_segmenter}


def build_parser():
    parser = argparse.ArgumentParser(description="segmentation-driven local style transfer")
    parser.add_argument("--image", type=str, required=True, help="input image")
    parser.add_argument("--model", type=str, required=True, help="checkpoint file")
    parser.add_argument("--output", type=str, default="output/enhanced_local_style.jpg", help="output image")
    parser.add_argument("--channels", type=int, default=16, help="model channels")
    parser.add_argument("--blocks", type=int, default=1, help="transformer blocks")
    parser.add_argument("--segmentation", choices=dimg.SEGMENTATIONS, default="felzenszwalb",
                        help="felzenszwalb: the reference's, on the host; slic: on the device")
    parser.add_argument("--device-segmentation", choices=tuple(DEVICE_SEGMENTERS), default=None,
                        help="a segmentation that stays on the device; when given it takes the place of --segmentation")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("enhanced_local_style: no GPU; this build has no CPU path")
    device = torch.device("cuda")
    print(f"device: {device}")
    model, _ = load_model(args.model, device, args.channels, args.blocks)
    segments = DEVICE_SEGMENTERS[args.device_segmentation]() if args.device_segmentation else None
    enhanced_local_style_transfer(model, args.image, args.output, device, args.segmentation, segments)


if __name__ == "__main__":
    main()
