"""Drop-in for the reference's compare_image_quality.py: ``calculate_mse`` / ``calculate_ssim`` / ``calculate_psnr`` (:14-33),
``find_matching_images`` (:35-59), ``compare_with_test_images`` (:61-215, local style and CycleGAN against the original test
images) and ``compare_image_folders`` (:217-392, one base folder against several), with the metrics on the GPU
(mstg_hip.metrics, csrc/metrics.hip and csrc/compare.hip).  PIL decodes the files on the host in cv2.imread's channel order; an
image whose shape differs from its original is resized as the reference's ``cv2.resize`` does (:100-106, :299-301) INSIDE the
metric kernel, and all comparisons of a folder go through one call and come back in one copy.  The resize is this build's
restatement of OpenCV's 8-bit INTER_LINEAR (include/mstg_hip.h), not compared with an OpenCV binary.

Differences from the reference, on purpose: ``compare_image_folders`` iterates the common names SORTED (the reference iterates a
``set`` in hash order, :276); results are returned, and an ``output_file`` ending in ``.csv`` gets the reference's column names
(:171-179 and :370-376) -- an ``.xlsx`` path and the charts are refused by name (no spreadsheet or plotting library is a
dependency of this build).
"""
from __future__ import annotations

import csv
import os
from pathlib import Path

import numpy as np

from complete_comparison import check_output
from image_quality_comparison import _decode
from mstg_hip.metrics import calculate_metrics, compare_three_way, evaluate_pairs_resized

PATTERNS = ("*.jpg", "*.jpeg", "*.png")  # :43
TEST_COLUMNS = ("图像", "局部风格_SSIM", "局部风格_PSNR", "局部风格_MSE", "CycleGAN_SSIM", "CycleGAN_PSNR", "CycleGAN_MSE")  # :171-179
FOLDER_COLUMNS = ("文件夹", "图像数量", "平均SSIM", "平均PSNR", "平均MSE")  # :370-376


def _as_u8(img, name):
    """uint8 arrays as they are; the reference's ``x.astype(float) / 255.0`` arrays (:114-116) mapped back with rint(x * 255) -- an
    array that does not lie on the byte grid to 1e-9 is not such an image and raises ValueError"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img
    if not np.issubdtype(img.dtype, np.floating):
        raise ValueError(f"compare_image_quality: {name} must be uint8 or the reference's float image / 255, got {img.dtype}")
    scaled = img.astype(np.float64) * 255.0
    back = np.rint(scaled)
    off = float(np.abs(scaled - back).max()) if img.size else 0.0
    if not off <= 1e-9 or back.min() < 0 or back.max() > 255:
        raise ValueError(f"compare_image_quality: {name} is not an 8-bit image / 255: it is off the byte grid by {off:.3g} "
                         f"(values {float(img.min()):.6g} .. {float(img.max()):.6g})")
    return back.astype(np.uint8)


def _one(img1, img2):
    return calculate_metrics(_as_u8(img1, "img1"), _as_u8(img2, "img2"))  # images of different shapes raise, as skimage does


def calculate_mse(img1, img2):
    return _one(img1, img2)["mse"]


def calculate_ssim(img1, img2):
    return _one(img1, img2)["ssim"]


def calculate_psnr(img1, img2):
    return _one(img1, img2)["psnr"]


def list_names(folder):
    """names of the image files of ``folder`` as the reference globs them: lower-case extensions only, per pattern (:43-44, :69-70)"""
    names = []
    for pattern in PATTERNS:
        names += [f.name for f in Path(folder).glob(pattern)]
    return names


def find_matching_images(base_folder, comparison_folder):
    """names present in both folders, as a set (:35-59)"""
    base, comp = set(list_names(base_folder)), set(list_names(comparison_folder))
    common = base & comp
    print(f"base folder: {len(base)} images, comparison folder: {len(comp)} images, {len(common)} in common")
    return common


def match_test_images(local_style_folder, cyclegan_folder, test_images_folder):
    """names of the test images that exist under the SAME name in both result folders, in listing order (:82-87)"""
    return [n for n in list_names(test_images_folder)
            if (Path(local_style_folder) / n).exists() and (Path(cyclegan_folder) / n).exists()]


def compare_with_test_images(local_style_folder, cyclegan_folder, test_images_folder, output_file=None):
    """Local style and CycleGAN against the original test images.  Returns None when nothing can be compared (:213-215), else the
    reference's dict (:204-212): 'avg_local_ssim', 'avg_local_psnr', 'avg_local_mse', 'avg_cyclegan_ssim', 'avg_cyclegan_psnr',
    'avg_cyclegan_mse' and 'details' (one dict per image with the reference's keys, :132-140)."""
    check_output(output_file, "compare_image_quality")
    names, images = [], ([], [], [])
    for n in match_test_images(local_style_folder, cyclegan_folder, test_images_folder):
        decoded = [_decode(str(Path(f) / n)) for f in (test_images_folder, cyclegan_folder, local_style_folder)]
        if any(d is None for d in decoded):
            print(f"  cannot read one of the images of {n}, skipped")  # :95-97
            continue
        names.append(n)
        for lst, d in zip(images, decoded):
            lst.append(d)
    if not names:
        print("no comparable images found")
        return None
    rows, avg_cy, avg_ls = compare_three_way(*images)
    details = []
    for n, r in zip(names, rows):
        ls, cy = r["local_style"], r["cyclegan"]
        details.append({"image": n, "local_style_ssim": ls["ssim"], "local_style_psnr": ls["psnr"], "local_style_mse": ls["mse"],
                        "cyclegan_ssim": cy["ssim"], "cyclegan_psnr": cy["psnr"], "cyclegan_mse": cy["mse"]})
        print(f"  {n}: local style SSIM={ls['ssim']:.4f}, PSNR={ls['psnr']:.4f}dB, MSE={ls['mse']:.8f}; "
              f"CycleGAN SSIM={cy['ssim']:.4f}, PSNR={cy['psnr']:.4f}dB, MSE={cy['mse']:.8f}")
    out = {"avg_local_ssim": avg_ls["ssim"], "avg_local_psnr": avg_ls["psnr"], "avg_local_mse": avg_ls["mse"],
           "avg_cyclegan_ssim": avg_cy["ssim"], "avg_cyclegan_psnr": avg_cy["psnr"], "avg_cyclegan_mse": avg_cy["mse"], "details": details}
    if output_file is not None:
        with open(output_file, "w", newline="", encoding="utf-8") as f:
            w = csv.writer(f)
            w.writerow(TEST_COLUMNS)
            for d in details:
                w.writerow([d["image"], d["local_style_ssim"], d["local_style_psnr"], d["local_style_mse"], d["cyclegan_ssim"],
                            d["cyclegan_psnr"], d["cyclegan_mse"]])
            w.writerow(["平均值", out["avg_local_ssim"], out["avg_local_psnr"], out["avg_local_mse"], out["avg_cyclegan_ssim"],
                        out["avg_cyclegan_psnr"], out["avg_cyclegan_mse"]])  # :182-192
    return out


def _valid(v):
    return not (np.isnan(v) or np.isinf(v) or v == 0)  # :323-329


def compare_image_folders(base_folder, comparison_folders, output_file=None):
    """One base folder against several: per comparison folder {'folder', 'images_count', 'avg_ssim', 'avg_psnr', 'avg_mse',
    'details'} (:260-267).  As in the reference a folder equal to the base is skipped (:238-240), and so are identical image pairs
    (:309-311) and pairs whose SSIM or PSNR is NaN, infinite or zero (:323-329)."""
    check_output(output_file, "compare_image_quality")
    results = []
    if not list_names(base_folder):
        print(f"no images in the base folder {base_folder}")
        return results
    for folder in comparison_folders:
        if os.path.normpath(base_folder) == os.path.normpath(folder):
            print(f"  {folder}: a folder is not compared with itself, skipped")
            continue
        common = find_matching_images(base_folder, folder)
        if not common:
            print(f"  {folder}: no matching images")
            continue
        names, pairs = [], []
        for n in sorted(common):
            a, b = _decode(os.path.join(base_folder, n)), _decode(os.path.join(folder, n))
            if a is None or b is None:
                print(f"  cannot read {n}, skipped")
                continue
            names.append(n)
            pairs.append((a, b))
        metrics, _ = evaluate_pairs_resized(pairs)
        details = []
        for n, m in zip(names, metrics):
            if m["mse"] == 0.0:  # the sum of squared byte differences is zero: np.array_equal of the two images, after the resize
                print(f"  {n}: the two images are identical, skipped")
            elif not _valid(m["ssim"]) or not _valid(m["psnr"]):
                print(f"  {n}: invalid SSIM / PSNR ({m['ssim']}, {m['psnr']}), skipped")
            else:
                details.append({"image": n, "ssim": m["ssim"], "psnr": m["psnr"], "mse": m["mse"]})
        k = len(details)
        res = {"folder": os.path.basename(folder), "images_count": len(common),
               "avg_ssim": sum(d["ssim"] for d in details) / k if k else 0.0, "avg_psnr": sum(d["psnr"] for d in details) / k if k else 0.0,
               "avg_mse": sum(d["mse"] for d in details) / k if k else 0.0, "details": details}
        print(f"  {res['folder']}: {k} pairs, SSIM {res['avg_ssim']:.4f}, PSNR {res['avg_psnr']:.4f} dB, MSE {res['avg_mse']:.8f}")
        results.append(res)
    if output_file is not None and any(r["details"] for r in results):
        with open(output_file, "w", newline="", encoding="utf-8") as f:
            w = csv.writer(f)
            w.writerow(FOLDER_COLUMNS)
            for r in results:
                w.writerow([r["folder"], r["images_count"], r["avg_ssim"], r["avg_psnr"], r["avg_mse"]])
    return results


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="image-quality metrics of folders of results, on the GPU")
    ap.add_argument("--base_folder", default="output/batch/local_style_enhanced_photo2monet")
    ap.add_argument("--comparison_folders", nargs="+")
    ap.add_argument("--output", default=None, help="path of a .csv with the reference's column names")
    ap.add_argument("--with_test_images", action="store_true")
    ap.add_argument("--test_images_folder", default="test_images")
    args = ap.parse_args(argv)
    if args.with_test_images:
        cyclegan = args.comparison_folders[0] if args.comparison_folders else "output/batch/cyclegan_photo2monet"  # :495-499
        return compare_with_test_images(args.base_folder, cyclegan, args.test_images_folder, args.output)
    if not args.comparison_folders:
        ap.error("--comparison_folders is required without --with_test_images")
    return compare_image_folders(args.base_folder, args.comparison_folders, args.output)


if __name__ == "__main__":
    main()
