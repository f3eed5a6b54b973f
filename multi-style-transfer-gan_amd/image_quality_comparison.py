"""Drop-in for the reference's image_quality_comparison.py: ``calculate_metrics`` (:11-34) and ``compare_folders`` (:36-176) with
the metrics computed on the GPU (mstg_hip.metrics, csrc/metrics.hip).  PIL decodes the files on the host; every pair of one image
size then goes through one batched launch and the numbers come back in one copy.

Differences from the reference, on purpose: images of different shapes raise ValueError instead of being resized with cv2.resize
(``mstg_hip.metrics.evaluate_pairs_resized`` and the drop-ins compare_image_quality.py / complete_comparison.py /
improved_image_compare.py resize as the reference does), and no spreadsheet or chart is written (``output_excel`` / ``output_chart`` must
stay None): ``compare_folders`` returns the per-pair list and the three averages.
"""
from __future__ import annotations

import glob
import os

import numpy as np

from mstg_hip.metrics import calculate_metrics, evaluate_pairs  # noqa: F401  (calculate_metrics is part of this module's surface)

EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp")


def list_images(folder):
    """image files of ``folder`` in the reference's order: per extension, lower case then upper case (:41-45)"""
    files = []
    for ext in EXTENSIONS:
        files += glob.glob(os.path.join(folder, f"*{ext}"))
        files += glob.glob(os.path.join(folder, f"*{ext.upper()}"))
    return files


def match_images(files1, files2):
    """Pairs (path1, path2): each file of the first list with the FIRST file of the second whose name is equal to its own, contains
    it or is contained in it (:60-66; prefixes such as cyclegan_ / local_style_ are ignored that way)."""
    names2 = [os.path.basename(f) for f in files2]
    pairs = []
    for f1 in files1:
        n1 = os.path.basename(f1)
        for f2, n2 in zip(files2, names2):
            if n1 == n2 or n1 in n2 or n2 in n1:
                pairs.append((f1, f2))
                break
    return pairs


def _decode(path):
    """uint8 (H, W, 3) in cv2.imread's channel order (B, G, R), or None if the file cannot be read (:82-87)"""
    from PIL import Image
    try:
        with Image.open(path) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])
    except (OSError, ValueError):
        return None


def compare_folders(folder1, folder2, output_excel=None, output_chart=None):
    """Metrics of every matching image pair of two folders.  Returns (results, averages): results = one dict {'image1', 'image2',
    'mse', 'psnr', 'ssim'} per readable pair, averages = {'mse', 'psnr', 'ssim'} plain means; None when nothing matches (:70-72)."""
    if output_excel is not None or output_chart is not None:
        raise ValueError("image_quality_comparison: spreadsheet and chart output are not part of this build; "
                         "use the returned results and averages")
    files1, files2 = list_images(folder1), list_images(folder2)
    print(f"{folder1}: {len(files1)} images\n{folder2}: {len(files2)} images")
    common = match_images(files1, files2)
    print(f"{len(common)} comparable pairs")
    names, pairs = [], []
    for p1, p2 in common:
        a, b = _decode(p1), _decode(p2)
        if a is None or b is None:
            print(f"  cannot read {os.path.basename(p1)} / {os.path.basename(p2)}, skipped")
            continue
        names.append((os.path.basename(p1), os.path.basename(p2)))
        pairs.append((a, b))
    if not pairs:
        print("nothing to compare")
        return None
    metrics, averages = evaluate_pairs(pairs)
    results = []
    for (n1, n2), m in zip(names, metrics):
        results.append({"image1": n1, "image2": n2, **m})
        print(f"  {n1} vs {n2}: MSE {m['mse']:.6f}, PSNR {m['psnr']:.2f} dB, SSIM {m['ssim']:.4f}")
    print(f"averages: MSE {averages['mse']:.6f}, PSNR {averages['psnr']:.2f} dB, SSIM {averages['ssim']:.4f}")
    return results, averages


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="MSE / PSNR / SSIM of the matching images of two folders, on the GPU")
    ap.add_argument("--folder1", required=True)
    ap.add_argument("--folder2", required=True)
    args = ap.parse_args()
    compare_folders(args.folder1, args.folder2)
