"""Drop-in for the reference's improved_image_compare.py: ``calculate_metrics`` (:8-27), ``get_file_ext`` (:29-31) and
``compare_folders_with_original`` (:33-191), the three-way comparison with file stems matched by containment, with the metrics on
the GPU (mstg_hip.metrics.compare_three_way, csrc/compare.hip; see complete_comparison.py for what is shared).  The resize of an
output whose shape differs from its original is this build's restatement of OpenCV's 8-bit INTER_LINEAR, not compared with an
OpenCV binary.

Differences from the reference, on purpose: the three folders are arguments and command-line options (the reference hard-codes
Windows paths, :35-37); the reference collects the common names in a ``set`` and iterates it in hash order (:64, :78) -- here the
set is iterated SORTED, so the order of the rows is defined; the rows are returned, ``output`` ending in ``.csv`` writes
complete_comparison.py's columns, and ``.xlsx`` is refused by name.
"""
from __future__ import annotations

import os

from complete_comparison import calculate_metrics, check_output, list_images, three_way_folders  # noqa: F401  (calculate_metrics: :8-27)


def get_file_ext(path):
    return os.path.splitext(path)[1].lower()


def _stem(path):
    return os.path.splitext(os.path.basename(path))[0]


def match_sets(original_files, cyclegan_files, local_style_files):
    """(original, cyclegan, local style) paths by the reference's two steps (:59-105).  A stem of the originals is common when the
    FIRST CycleGAN stem that contains it or is contained in it exists and some local-style stem does the same (:64-72: only that
    first CycleGAN stem is tried); then, per common stem in sorted order, the first file of each folder whose stem equals it,
    contains it or is contained in it."""
    def touches(a, b):
        return a in b or b in a
    cy_stems, ls_stems = [_stem(f) for f in cyclegan_files], [_stem(f) for f in local_style_files]
    common = set()
    for name in (_stem(f) for f in original_files):
        if any(touches(name, c) for c in cy_stems) and any(touches(name, s) for s in ls_stems):
            common.add(name)
    sets = []
    for name in sorted(common):
        found = [next((f for f in files if touches(name, _stem(f))), None) for files in (original_files, cyclegan_files, local_style_files)]
        if all(found):
            sets.append(tuple(found))
    return sets


def compare_folders_with_original(original_folder, cyclegan_folder, local_style_folder, output=None):
    """The reference's ``compare_folders_with_original`` for three folders given by the caller.  Returns None when nothing matches
    (:107-109), else complete_comparison.py's dict plus 'better_count' = on how many images the local style beats CycleGAN per
    metric (:181-185)."""
    check_output(output, "improved_image_compare")
    files = [list_images(f) for f in (original_folder, cyclegan_folder, local_style_folder)]
    for label, fl in zip(("original", "CycleGAN", "local style"), files):
        print(f"{label}: {len(fl)} images")
    sets = match_sets(*files)
    if not sets:
        print("no image is present in all three folders, check the file names")
        return None
    print(f"{len(sets)} complete sets")
    out = three_way_folders(sets, output)
    if out is not None:
        out["better_count"] = {m: w["LocalStyle"] for m, w in out["wins"].items()}
    return out


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="original vs CycleGAN vs local style, stems matched by containment, on the GPU")
    ap.add_argument("--original_folder", required=True)
    ap.add_argument("--cyclegan_folder", required=True)
    ap.add_argument("--local_style_folder", required=True)
    ap.add_argument("--output", default=None, help="path of a .csv with complete_comparison.py's columns")
    args = ap.parse_args()
    compare_folders_with_original(args.original_folder, args.cyclegan_folder, args.local_style_folder, args.output)
