"""MI355X: the segmentation-driven local style (csrc/segment_style.hip through mstg_hip.image) on 1 and on 64 canvases of 256 x 256
that are already on the device, with labels from ``felzenszwalb_labels`` of synthetic images.

usage: python tools/bench_enhanced_local_style.py [--n 64] [--seconds 0.5] [--repeats 5] [--json FILE]

  map_raw, map_smooth     segment_blend_map without and with the smoothing (four and six launches), for N = 1 and N = --n;
  smoothing               gaussian_reflect_f32 alone (two launches);
  finish                  enhanced_style_finish (five launches);
  kernels                 the library's per-launch profiler (two device events around every launch) over ``--repeats`` calls of
                          map_smooth and finish: the median duration of every kernel, seg_stats_kernel among them;
  stats_bounds            for seg_stats_kernel, what its time would be if one resource alone bound it: HBM (the bytes it reads at
                          ``--hbm-gbs``), the global 64-bit atomics it issues (counted on the host from the labels: one per used slot
                          and sum of every tile, at ``--atomic-gops`` billion a second -- a rate this tool does NOT measure), and the
                          measured time; LDS and vector issue are not modelled here (DESIGN.md 3d says what the counts suggest);
  segmentation_host_ms    mstg_felzenszwalb_u8 per image on the host (single thread), median over the distinct images;
  numpy_restatement_ms    tests/enhanced_local_style_ref.py through the host for ONE canvas: statistics + smoothing, and the finish.
The bytes of the chain are checked against the composed stage functions on the first image.  Device timings are device events
around windows long enough to fill ``--seconds``, after a warm-up, with a synchronise at both ends; each figure is reported as
min / median / max over its repeats.  Prints one JSON line.  Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "multi-style-transfer-gan_amd"), ROOT):
    sys.path.insert(0, p)

DEV = "cuda:0"
T = 256
DISTINCT = 8  # distinct synthetic images (and host segmentations); the batch repeats them


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters  # ms per call


def device_stats(fn, seconds, repeats):
    for _ in range(2):
        fn()
    iters = max(2, int(seconds * 1e3 / max(window(fn, 2), 1e-3)) + 1)
    s = [window(fn, iters) for _ in range(repeats)]
    return {"min_ms": min(s), "median_ms": statistics.median(s), "max_ms": max(s), "iters_per_window": iters, "windows": len(s)}


def kernel_times(fn, repeats):
    """{kernel: median ms} from the library's per-launch profiler over ``repeats`` calls"""
    from mstg_hip import _lib
    lib = _lib.load()
    fn()
    torch.cuda.synchronize()
    lib.mstg_prof_enable(1)
    try:
        for _ in range(repeats):
            fn()
        torch.cuda.synchronize()
        per = {}
        name, ms = C.create_string_buffer(256), C.c_float()
        for i in range(lib.mstg_prof_count()):
            lib.mstg_prof_get(i, name, 256, C.byref(ms))
            per.setdefault(name.value.decode(), []).append(ms.value)
    finally:
        lib.mstg_prof_enable(0)
    return {k: statistics.median(v) for k, v in per.items()}


def tile_atomics(labels, slots=128, th=16, tw=64):
    """global 64-bit atomics of seg_stats_kernel for one (H, W) label map, counted on the host: per tile, eleven sums for every
    distinct label of the tile and its halo (an upper bound: a sum that is zero is skipped); (atomics, tiles, most labels a tile)"""
    H, W = labels.shape
    total = tiles = most = 0
    for y in range(0, H, th):
        for x in range(0, W, tw):
            k = len(np.unique(labels[max(y - 1, 0):y + th + 1, max(x - 1, 0):x + tw + 1]))
            total += 11 * k
            tiles += 1
            most = max(most, k)
    return total, tiles, most


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="HBM rate for the bound, GB/s (an assumption, not measured here)")
    ap.add_argument("--atomic-gops", type=float, default=10.0, help="global 64-bit atomics per second for the bound, 1e9 (an assumption)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_enhanced_local_style.py needs a GPU")
    import enhanced_local_style_ref as ER
    from mstg_hip import image as dimg
    distinct = [ER.smooth_noise(T, T, 100 + i, sigma=4.0 + 2 * i) for i in range(DISTINCT)]
    seg_ms, labels_np = [], []
    for im in distinct:
        t0 = time.perf_counter()
        labels_np.append(dimg.felzenszwalb_labels(im))
        seg_ms.append((time.perf_counter() - t0) * 1e3)
    S = max(int(l.max()) for l in labels_np) + 1
    imgs = torch.from_numpy(np.stack([distinct[i % DISTINCT] for i in range(args.n)])).to(DEV)
    labels = torch.from_numpy(np.stack([labels_np[i % DISTINCT] for i in range(args.n)])).to(DEV)
    styled = torch.from_numpy(np.ascontiguousarray(255 - np.stack([distinct[(i + 1) % DISTINCT] for i in range(args.n)])[..., ::-1])).to(DEV)
    maps = dimg.segment_blend_map(imgs, labels, S)
    first = dimg.enhanced_style_finish(imgs[0], styled[0], maps[0])
    composed = dimg.bilateral_u8(dimg.sharpen3_u8(dimg.hsv_enhance_u8(dimg.blend_map_u8(imgs[0], styled[0], maps[0]))), 5, 50, 50)
    counts = [tile_atomics(l) for l in labels_np]
    result = {"H": T, "W": T, "num_segments": S, "segments_per_image": [int(l.max()) + 1 for l in labels_np],
              "chain_equals_composed_stages": bool(torch.equal(first, composed)),
              "segmentation_host_ms": {"median": statistics.median(seg_ms), "min": min(seg_ms), "max": max(seg_ms)},
              "stats_global_atomics_per_image": statistics.median(c[0] for c in counts),
              "stats_most_labels_in_a_tile": max(c[2] for c in counts)}
    t0 = time.perf_counter()
    ref_map = ER.segment_blend_map(distinct[0], labels_np[0], int(labels_np[0].max()) + 1)[0]
    t1 = time.perf_counter()
    ref_out = ER.enhanced_style_finish(distinct[0], styled[0].cpu().numpy(), ref_map)
    t2 = time.perf_counter()
    result["numpy_restatement_ms"] = {"map": (t1 - t0) * 1e3, "finish": (t2 - t1) * 1e3}
    result["device_equals_numpy_on_first_image"] = bool(np.array_equal(ref_map.view(np.uint32), maps[0].cpu().numpy().view(np.uint32))
                                                        and np.array_equal(ref_out, first.cpu().numpy()))
    for n in sorted({1, args.n}):
        x, lab, st, m = imgs[:n], labels[:n], styled[:n], maps[:n]
        r = {"map_raw": device_stats(lambda: dimg.segment_blend_map(x, lab, S, smooth=False), args.seconds, args.repeats),
             "map_smooth": device_stats(lambda: dimg.segment_blend_map(x, lab, S, smooth=True), args.seconds, args.repeats),
             "smoothing": device_stats(lambda: dimg.gaussian_reflect_f32(m), args.seconds, args.repeats),
             "finish": device_stats(lambda: dimg.enhanced_style_finish(x, st, m), args.seconds, args.repeats)}
        r["kernels_ms"] = kernel_times(lambda: (dimg.segment_blend_map(x, lab, S, smooth=True), dimg.enhanced_style_finish(x, st, m)),
                                       max(args.repeats, 5))
        stats_ms = next((v for k, v in r["kernels_ms"].items() if "seg_stats_kernel" in k), None)
        px = n * T * T
        atomics = sum(counts[i % DISTINCT][0] for i in range(n))
        r["stats_bounds"] = {"measured_ms": stats_ms, "hbm_ms": px * 7 / (args.hbm_gbs * 1e9) * 1e3,
                             "global_atomics": atomics, "atomic_ms": atomics / (args.atomic_gops * 1e9) * 1e3,
                             "pixels_per_s": px / (stats_ms * 1e-3) if stats_ms else None}
        r["host_segmentation_share_of_end_to_end"] = result["segmentation_host_ms"]["median"] * n / (
            result["segmentation_host_ms"]["median"] * n + r["map_smooth"]["median_ms"] + r["finish"]["median_ms"])
        result[f"N{n}"] = r
        for key in ("map_raw", "map_smooth", "smoothing", "finish"):
            print(f"N = {n:3d}  {key:12s} {r[key]['median_ms']:10.3f} ms  [{r[key]['min_ms']:.3f} .. {r[key]['max_ms']:.3f}]", file=sys.stderr)
        for k, v in sorted(r["kernels_ms"].items()):
            print(f"N = {n:3d}    {k:40s} {v * 1e3:10.1f} us", file=sys.stderr)
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
