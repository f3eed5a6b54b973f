"""Drop-in for the reference's complete_comparison.py: ``calculate_metrics`` (:13-32) and ``compare_with_original`` (:34-429), the
three-way comparison of every original against its CycleGAN output and its local-style output, with the metrics on the GPU
(mstg_hip.metrics.compare_three_way, csrc/compare.hip).  PIL decodes the files on the host in cv2.imread's channel order; an
output whose shape differs from its original is resized as the reference's ``cv2.resize`` does INSIDE the metric kernel, and all
comparisons of a run go through one call and come back in one copy.  The resize is this build's restatement of OpenCV's 8-bit
INTER_LINEAR (include/mstg_hip.h), not compared with an OpenCV binary.

Differences from the reference, on purpose: the three folders are arguments and command-line options (the reference hard-codes
Windows paths, :36-38); the rows are RETURNED, and with ``output`` ending in ``.csv`` the detailed table is written with the
reference's column names (:147-158) and its AVERAGE row (:313-324); an ``.xlsx`` path and charts are refused by name (no
spreadsheet or plotting library is a dependency of this build, as in image_quality_comparison.py).
"""
from __future__ import annotations

import csv
import glob
import os

from image_quality_comparison import _decode
from mstg_hip.metrics import better_labels, compare_three_way, evaluate_pairs_resized

EXTENSIONS = ("*.jpg", "*.jpeg", "*.png", "*.bmp")  # :41
COLUMNS = ("Image Name", "CycleGAN MSE", "LocalStyle MSE", "MSE Better", "CycleGAN PSNR", "LocalStyle PSNR", "PSNR Better",
           "CycleGAN SSIM", "LocalStyle SSIM", "SSIM Better")  # :147-158


def calculate_metrics(original_img, processed_img):
    """(mse, psnr, ssim) of two uint8 (H, W, 3) images, numpy arrays or cuda tensors; a processed image of another shape is resized
    to the original's as cv2.resize does (:16-17)"""
    (r,), _ = evaluate_pairs_resized([(original_img, processed_img)])
    return r["mse"], r["psnr"], r["ssim"]


def list_images(folder):
    """image files of ``folder`` in the reference's order: per extension, lower case only (:41-53)"""
    files = []
    for ext in EXTENSIONS:
        files += glob.glob(os.path.join(folder, ext))
    return files


def match_sets(original_files, cyclegan_files, local_style_files):
    """(original, cyclegan, local style) paths: each original with the FIRST file of either other folder whose name equals its own
    or contains it (``orig == other or orig in other``), kept only when both folders have one (:60-82)"""
    def by_name(files):
        return {os.path.basename(f): f for f in files}  # a later file of the same name replaces an earlier one (:60-62)
    orig, cy, ls = by_name(original_files), by_name(cyclegan_files), by_name(local_style_files)
    sets = []
    for name in orig:
        found = []
        for other in (cy, ls):
            found.append(next((n for n in other if name == n or name in n), None))
        if found[0] and found[1]:
            sets.append((orig[name], cy[found[0]], ls[found[1]]))
    return sets


def check_output(output, who):
    if output is None:
        return
    ext = os.path.splitext(str(output))[1].lower()
    if ext == ".xlsx":
        raise ValueError(f"{who}: .xlsx output is not part of this build (no spreadsheet library); give a path ending in .csv")
    if ext != ".csv":
        raise ValueError(f"{who}: output {output!r}: only .csv is written; .xlsx and charts are not part of this build")


def three_way_folders(sets, output):
    """decode, compare and (optionally) write: the part the three-way drop-ins share.  Returns None when nothing can be compared,
    else {'results', 'cyclegan_averages', 'local_style_averages', 'wins'}"""
    names, images = [], ([], [], [])
    for paths in sets:
        decoded = [_decode(p) for p in paths]
        if any(d is None for d in decoded):
            print(f"  cannot read image set {os.path.basename(paths[0])}, skipped")  # :107-109
            continue
        names.append(tuple(os.path.basename(p) for p in paths))
        for lst, d in zip(images, decoded):
            lst.append(d)
    if not names:
        print("nothing to compare")
        return None
    rows, avg_cy, avg_ls = compare_three_way(*images)
    results = []
    for (orig, cy, ls), row in zip(names, rows):
        results.append({"orig_name": orig, "cyclegan": {"name": cy, **row["cyclegan"]}, "local_style": {"name": ls, **row["local_style"]},
                        "comparison": row["comparison"]})
        print(f"  {orig}: CycleGAN ({cy}) MSE {row['cyclegan']['mse']:.6f}, PSNR {row['cyclegan']['psnr']:.2f}dB, SSIM {row['cyclegan']['ssim']:.4f}; "
              f"LocalStyle ({ls}) MSE {row['local_style']['mse']:.6f}, PSNR {row['local_style']['psnr']:.2f}dB, SSIM {row['local_style']['ssim']:.4f}")
    wins = {m: {"CycleGAN": 0, "LocalStyle": 0} for m in ("mse", "psnr", "ssim")}
    for r in results:
        for m in wins:
            wins[m][r["comparison"][f"{m}_better"]] += 1
    for label, avg in (("CycleGAN", avg_cy), ("LocalStyle", avg_ls)):
        print(f"average {label}: MSE {avg['mse']:.6f}, PSNR {avg['psnr']:.2f}dB, SSIM {avg['ssim']:.4f}")
    if output is not None:
        write_csv(output, results, avg_cy, avg_ls)
    return {"results": results, "cyclegan_averages": avg_cy, "local_style_averages": avg_ls, "wins": wins}


def csv_row(name, cy, ls, labels):
    return [name, cy["mse"], ls["mse"], labels["mse_better"], cy["psnr"], ls["psnr"], labels["psnr_better"], cy["ssim"], ls["ssim"],
            labels["ssim_better"]]


def write_csv(path, results, avg_cy, avg_ls):
    """the 'Detailed Results' table of the reference's spreadsheet (:147-158) and its AVERAGE row (:313-324), floats as repr()"""
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        w.writerow(COLUMNS)
        for r in results:
            w.writerow(csv_row(r["orig_name"], r["cyclegan"], r["local_style"], r["comparison"]))
        w.writerow(csv_row("AVERAGE", avg_cy, avg_ls, better_labels(avg_cy, avg_ls)))


def compare_with_original(original_folder, cyclegan_folder, local_style_folder, output=None):
    """The reference's ``compare_with_original`` for three folders given by the caller.  Returns None when no complete image set is
    found (:86-88), else a dict: 'results' (per image 'orig_name', 'cyclegan' / 'local_style' = {'name', 'mse', 'psnr', 'ssim',
    'resized'}, 'comparison' = the three "better" labels, :124-143), 'cyclegan_averages', 'local_style_averages' and 'wins'
    (:182-199)."""
    check_output(output, "complete_comparison")
    folders = (original_folder, cyclegan_folder, local_style_folder)
    files = [list_images(f) for f in folders]
    for label, fl in zip(("Original photos", "CycleGAN processed", "LocalStyle processed"), files):
        print(f"{label}: Found {len(fl)} images")
    sets = match_sets(*files)
    print(f"Found {len(sets)} comparable image sets")
    if not sets:
        print("No complete image matches found, please check file naming")
        return None
    return three_way_folders(sets, output)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="original vs CycleGAN vs local style: MSE / PSNR / SSIM on the GPU")
    ap.add_argument("--original_folder", required=True)
    ap.add_argument("--cyclegan_folder", required=True)
    ap.add_argument("--local_style_folder", required=True)
    ap.add_argument("--output", default=None, help="path of a .csv with the reference's columns")
    args = ap.parse_args()
    compare_with_original(args.original_folder, args.cyclegan_folder, args.local_style_folder, args.output)
