"""Colour-block repair that keeps the image sharp, on the GPU: the five functions and the command line of the reference's
improved_smooth.py, running through mstg_hip.image (csrc/color_blocks.hip).  Every function takes a PIL image or a numpy array
(H, W, 3) uint8 RGB and returns the same kind; the pixels go to the device, the kernels run there, the result comes back.  Files
are decoded and encoded with Pillow; OpenCV is not needed.  The OpenCV steps are restated from their definitions
(include/mstg_hip.h) and have not been compared with an OpenCV binary.  There is no CPU path: without a GPU every call raises.

usage: python improved_smooth.py --input IMAGE [--original IMAGE] [--output output/fixed_image_improved.jpg]
"""
import argparse
import os

import numpy as np
import torch
from PIL import Image

DEVICE = "cuda"


def _to_numpy(img):
    a = np.array(img) if isinstance(img, Image.Image) else np.asarray(img)
    if a.ndim == 2:  # a grey image: the three channels are equal
        a = np.stack([a, a, a], axis=-1)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"improved_smooth: expected an RGB image of bytes, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _to_device(img):
    return torch.from_numpy(_to_numpy(img)).to(DEVICE)


def _like(img, result):
    """``result`` (a device tensor) as the kind of ``img``"""
    a = result.cpu().numpy()
    return Image.fromarray(a) if isinstance(img, Image.Image) else a


def adaptive_color_correction(img, blocks_detected=None, radius=50):
    """Pull every pixel of a detected block halfway towards the mean colour of its (2 radius + 1)^2 surroundings; the other pixels
    stay.  ``blocks_detected``: a bool (H, W) array, or None to detect the blocks first."""
    from mstg_hip import image as dimg
    mask = None if blocks_detected is None else torch.from_numpy(np.ascontiguousarray(np.asarray(blocks_detected) != 0)).to(DEVICE)
    return _like(img, dimg.adaptive_color_correction(_to_device(img), mask, radius))


def detect_color_blocks(img, threshold=30, kernel_size=11):
    """-> bool (H, W) array: the surroundings (a ``kernel_size`` box) of every pixel where the a and b channels of Lab change by more
    than ``threshold`` on average"""
    from mstg_hip import image as dimg
    return dimg.detect_color_blocks(_to_device(img), threshold, kernel_size).cpu().numpy()


def edge_preserving_smoothing(img, sigma_s=60, sigma_r=0.4):
    """The bilateral filter with the radius derived from ``sigma_s`` (90 pixels at the default) and a colour sigma of
    ``sigma_r * 255``"""
    from mstg_hip import image as dimg
    return _like(img, dimg.edge_preserving_smoothing(_to_device(img), sigma_s, sigma_r))


def detail_enhancing_blend(img, original, alpha=0.3, beta=1.5):
    """``img * (1 - alpha) + original * alpha + detail * beta`` with ``detail`` = the original minus its Gaussian blur (sigma 3).  As in
    the reference the blend happens for two PIL images (an original of another size is resized with Lanczos first); any other pair
    returns ``img`` as it is."""
    if not (isinstance(img, Image.Image) and isinstance(original, Image.Image)):
        return img
    from mstg_hip import image as dimg
    return _like(img, dimg.detail_enhancing_blend(_to_device(img), _to_device(original), alpha, beta))


def fix_color_blocks_improved(input_img_path, original_img_path=None, output_img_path=None):
    """Detect the blocks, correct them, smooth with preserved edges and, when the original exists, blend its detail back in
    (alpha 0.1, beta 0.5): one chain on the device.  -> PIL image; saved to ``output_img_path`` when that is given."""
    from mstg_hip import image as dimg
    generated = Image.open(input_img_path).convert("RGB")
    original = None
    if original_img_path and os.path.exists(original_img_path):
        original = _to_device(Image.open(original_img_path).convert("RGB"))
    final = _like(generated, dimg.fix_color_blocks(_to_device(generated), original))
    if output_img_path:
        folder = os.path.dirname(output_img_path)
        if folder:
            os.makedirs(folder, exist_ok=True)
        final.save(output_img_path)
        print(f"saved the repaired image to: {output_img_path}")
    return final


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="colour-block repair that keeps the image sharp")
    parser.add_argument("--input", type=str, required=True, help="image to repair")
    parser.add_argument("--original", type=str, help="the original image, for the detail blend")
    parser.add_argument("--output", type=str, default="output/fixed_image_improved.jpg", help="where to save the result")
    args = parser.parse_args()
    fix_color_blocks_improved(args.input, args.original, args.output)
