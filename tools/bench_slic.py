"""MI355X: the device SLIC segmentation (csrc/slic.hip through mstg_hip.image) on 1 and on 64 canvases of 256 x 256 that are already
on the device, and the segmentation-driven local style end to end under each segmentation.

usage: python tools/bench_slic.py [--n 64] [--seconds 0.5] [--repeats 5] [--json FILE]

  assign                  slic_assign: the Lab bytes, the grid and ten rounds of assignment and update (22 launches), N = 1 and --n;
  connect                 connect_labels of the raw labels (13 launches at 256 x 256);
  slic_labels             the whole segmentation (35 launches);
  kernels                 the library's per-launch profiler (two device events around every launch) over ``--repeats`` calls of
                          slic_labels: the median duration of every kernel, slic_assign_kernel among them;
  assign_bounds           for slic_assign_kernel, what a round would cost if one resource alone bound it: HBM (the bytes it reads and
                          writes at ``--hbm-gbs``), the float32 operations of the candidate walk (counted on the host from the final
                          centres: the centres whose window meets each tile, 4 pixels x 17 operations a thread and centre, at
                          ``--fp32-tflops``), and the measured time; both rates are assumptions, not measured here;
  end_to_end              process_enhanced_local_style of ONE 256 x 256 image with segmentation="felzenszwalb" (the host step) and
                          with "slic", wall clock with a synchronise at both ends, median over ``--repeats`` runs after a warm-up;
  segmentation_host_ms    mstg_felzenszwalb_u8 per canvas on the host, for comparison.
The labels of the first image are checked against tests/slic_ref.py.  Device timings are device events around windows long enough
to fill ``--seconds``, after a warm-up, with a synchronise at both ends; each figure is reported as min / median / max over its
repeats.  Prints one JSON line.  Needs a GPU: there is no fallback."""
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
DISTINCT = 8  # distinct synthetic images; the batch repeats them


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


def wall_stats(fn, repeats):
    fn()
    s = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": min(s), "median_ms": statistics.median(s), "max_ms": max(s), "runs": len(s)}


def kernel_times(fn, repeats):
    """{kernel: (median ms, launches per call)} from the library's per-launch profiler over ``repeats`` calls"""
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
    return {k: {"median_ms": statistics.median(v), "launches_per_call": len(v) // repeats} for k, v in per.items()}


def walk_entries(centres, step, th=16, tw=64):
    """list entries of slic_assign_kernel for one image, counted on the host from (K, 5) centres: per tile the centres whose
    window meets it; (sum over the tiles, most in a tile)"""
    iy, ix = centres[:, 0].astype(np.int64), centres[:, 1].astype(np.int64)
    total = most = 0
    for y in range(0, T, th):
        for x in range(0, T, tw):
            k = int(((iy - 2 * step <= y + th - 1) & (iy + 2 * step >= y) & (ix - 2 * step <= x + tw - 1) & (ix + 2 * step >= x)).sum())
            total += k
            most = max(most, k)
    return total, most


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="HBM rate for the bound, GB/s (an assumption, not measured here)")
    ap.add_argument("--fp32-tflops", type=float, default=100.0, help="vector float32 rate for the bound (an assumption, not measured here)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_slic.py needs a GPU")
    import enhanced_generator as eg
    import enhanced_local_style_ref as ER
    import slic_ref as SR
    from mstg_hip import image as dimg
    distinct = [ER.smooth_noise(T, T, 100 + i, sigma=4.0 + 2 * i) for i in range(DISTINCT)]
    imgs = torch.from_numpy(np.stack([distinct[i % DISTINCT] for i in range(args.n)])).to(DEV)
    step, ny, nx = dimg.slic_grid(T, T)
    min_size = dimg.slic_min_size(T, T)
    labels, count = dimg.slic_labels(imgs, return_count=True)
    raw, centres = dimg.slic_assign(imgs)
    want, want_count = SR.slic(distinct[0])
    result = {"H": T, "W": T, "n_segments": 100, "step": step, "K": ny * nx, "min_size": min_size, "bound": dimg.slic_segment_bound(T, T),
              "segments_per_image": count[:DISTINCT].cpu().tolist(),
              "device_equals_numpy_on_first_image": bool(np.array_equal(want, labels[0].cpu().numpy()) and want_count == int(count[0]))}
    seg_ms = []
    for im in distinct:
        t0 = time.perf_counter()
        dimg.felzenszwalb_labels(im)
        seg_ms.append((time.perf_counter() - t0) * 1e3)
    result["segmentation_host_ms"] = {"median": statistics.median(seg_ms), "min": min(seg_ms), "max": max(seg_ms)}
    torch.manual_seed(11)
    model = eg.EnhancedGenerator(16, 1).to(DEV)
    model.eval()
    one = imgs[0]
    result["end_to_end"] = {s: wall_stats(lambda: dimg.process_enhanced_local_style(model, one, segmentation=s), max(args.repeats, 9))
                            for s in dimg.SEGMENTATIONS}
    cen_np = centres.cpu().numpy()
    entries = [walk_entries(cen_np[i % DISTINCT], step) for i in range(DISTINCT)]
    for n in sorted({1, args.n}):
        x, rw = imgs[:n], raw[:n]
        r = {"assign": device_stats(lambda: dimg.slic_assign(x), args.seconds, args.repeats),
             "connect": device_stats(lambda: dimg.connect_labels(rw, min_size), args.seconds, args.repeats),
             "slic_labels": device_stats(lambda: dimg.slic_labels(x), args.seconds, args.repeats)}
        r["kernels"] = kernel_times(lambda: dimg.slic_labels(x), max(args.repeats, 5))
        assign_ms = next((v["median_ms"] for k, v in r["kernels"].items() if "slic_assign_kernel" in k), None)
        px = n * T * T
        walked = sum(entries[i % DISTINCT][0] for i in range(n))  # list entries over all tiles; every one costs 256 threads x 4 pixels
        r["assign_bounds"] = {"measured_ms_per_round": assign_ms, "hbm_ms": px * (3 + 4 + 4) / (args.hbm_gbs * 1e9) * 1e3,
                              "walked_entries": walked, "most_in_a_tile": max(e[1] for e in entries),
                              "fp32_ms": walked * 1024 * 17 / (args.fp32_tflops * 1e12) * 1e3,
                              "pixels_per_s": px / (assign_ms * 1e-3) if assign_ms else None}
        result[f"N{n}"] = r
        for key in ("assign", "connect", "slic_labels"):
            print(f"N = {n:3d}  {key:12s} {r[key]['median_ms']:10.3f} ms  [{r[key]['min_ms']:.3f} .. {r[key]['max_ms']:.3f}]", file=sys.stderr)
        for k, v in sorted(r["kernels"].items()):
            print(f"N = {n:3d}    {k:60s} {v['median_ms'] * 1e3:10.1f} us x {v['launches_per_call']}", file=sys.stderr)
    for s, v in result["end_to_end"].items():
        print(f"end to end, {s:12s} {v['median_ms']:10.3f} ms  [{v['min_ms']:.3f} .. {v['max_ms']:.3f}]", file=sys.stderr)
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
