"""Five ways of finishing a generated image, on the GPU: the functions and the command line of the reference's
advanced_transform.py, running through mstg_hip.image (csrc/advanced_transform.hip).  The post-process functions take the
generator's output tensor (1, 3, H, W) and, where the reference does, the original PIL image, and return a PIL image; the pixels
stay on the device between the forward pass and the final copy.  Files are decoded and encoded with Pillow; OpenCV, torchvision and
matplotlib are not needed.  The OpenCV steps are restated from their definitions (include/mstg_hip.h) and have not been compared
with an OpenCV binary; the K-means draws its centres from numpy's generator (a seed), not from OpenCV's.  Not built: the random
ColorJitter on the input of the contrast setting and the comparison chart.  There is no CPU path: without a GPU every call raises.

usage: python advanced_transform.py --image IMAGE --model CHECKPOINT [--output_dir output/advanced]
"""
import argparse
import os

import numpy as np
import torch
from PIL import Image

from enhanced_generator import EnhancedGenerator

SETTINGS = (("standard", "standard"), ("contrast", "contrast"), ("multi_scale", "multi_scale_fusion"), ("detail", "detail_enhanced"),
            ("regions", "local_style"))


def load_model(model_path, device, channels=16, blocks=1):
    """the generator of a checkpoint that holds ``G_AB_state_dict`` or ``G_BA_state_dict`` -> (model, model_type)"""
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


def _u8(img, device="cuda"):
    a = np.array(img.convert("RGB") if isinstance(img, Image.Image) else img, dtype=np.uint8)  # a writable, contiguous copy
    return torch.from_numpy(a).to(device)


def _pil(t):
    return Image.fromarray(t.cpu().numpy())


def _styled(tensor):
    """the plain post-process of a (1, 3, H, W) or (3, H, W) output, on its device -> uint8 (H, W, 3)"""
    from mstg_hip import image as dimg
    return dimg.to_u8(tensor[0] if tensor.dim() == 4 else tensor)


def _original(original_img, styled):
    """the original at the size of the output (LANCZOS), on the device"""
    from mstg_hip import image as dimg
    h, w = styled.shape[:2]
    return dimg.resize_u8(_u8(original_img, styled.device), (w, h), dimg.LANCZOS)


def standard_postprocess(tensor):
    """(x + 1) / 2, clamp, * 255, truncate"""
    return _pil(_styled(tensor))


def contrast_enhanced_postprocess(tensor):
    """CLAHE(2.0, 8 x 8) on the lightness of Lab, then saturation * 1.2"""
    from mstg_hip import image as dimg
    return _pil(dimg.contrast_enhanced_finish(_styled(tensor)))


def multi_scale_fusion(tensor, original_img, model):
    """The original at 0.5, 0.75 and 1.0 of its size, each through ``model`` (one image per pass, as in the reference: a batch of
    three does not give the same bytes), fused with the weights 0.2, 0.3, 0.5 and brightened by 1.1.  ``model`` is an argument
    here: the reference reads a global.  As in the reference ``tensor`` itself does not enter the result."""
    from mstg_hip import image as dimg
    img = _u8(original_img, tensor.device)
    height, width = img.shape[:2]
    inputs = [dimg.resize_u8(dimg.resize_u8(img, (int(width * s), int(height * s)), dimg.LANCZOS), (256, 256), dimg.BILINEAR)
              for s in (0.5, 0.75, 1.0)]
    with torch.no_grad():
        outs = [dimg.to_u8(model(dimg.to_tensor(i).unsqueeze(0))[0]) for i in inputs]
    return _pil(dimg.fuse_scales_u8(torch.stack(outs)))


def detail_enhanced_postprocess(tensor, original_img):
    """The detail layer of the original's grey image (grey minus its Gaussian blur, sigma 3) added to the lightness, then
    saturation * 1.2 and value * 1.1"""
    from mstg_hip import image as dimg
    styled = _styled(tensor)
    return _pil(dimg.detail_enhanced_finish(styled, _original(original_img, styled)))


def local_style_transfer(tensor, original_img, seed=0):
    """K-means (K = 5) of the original's colours, a blend ratio per region (0.8, 0.4, then 0.6), then saturation * 1.2.  ``seed``
    fixes the initial centres; the reference's come from OpenCV's generator."""
    from mstg_hip import image as dimg
    styled = _styled(tensor)
    return _pil(dimg.local_regions_finish(styled, _original(original_img, styled), seed))


def generate_with_different_settings(model, image_path, output_dir, device, model_type, seed=0):
    """The five settings for one image file, each saved as ``<model_type>_<name>.jpg`` -> [(name, PIL image)]"""
    from mstg_hip import image as dimg
    os.makedirs(output_dir, exist_ok=True)
    img = _u8(Image.open(image_path), device)
    results = []
    for setting, name in SETTINGS:
        print(f"trying {name}...")
        out = _pil(dimg.process_advanced(model, img, setting, seed))
        path = os.path.join(output_dir, f"{model_type}_{name}.jpg")
        out.save(path)
        print(f"saved to {path}")
        results.append((name, out))
    return results


def main(argv=None):
    parser = argparse.ArgumentParser(description="advanced image style transfer")
    parser.add_argument("--image", type=str, required=True, help="input image")
    parser.add_argument("--model", type=str, required=True, help="checkpoint file")
    parser.add_argument("--output_dir", type=str, default="output/advanced", help="output folder")
    args = parser.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("advanced_transform: no GPU; this build has no CPU path")
    device = torch.device("cuda")
    print(f"device: {device}")
    model, model_type = load_model(args.model, device)
    generate_with_different_settings(model, args.image, args.output_dir, device, model_type)


if __name__ == "__main__":
    main()
