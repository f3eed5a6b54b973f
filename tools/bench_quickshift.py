"""MI355X: the device quickshift segmentation (csrc/quickshift.hip through mstg_hip.image) on 1 and on 64 canvases of 256 x 256 that
are already on the device, and the segmentation-driven local style end to end under each segmentation.

usage: python tools/bench_quickshift.py [--n 64] [--seconds 0.5] [--repeats 5] [--json FILE]

  density                 quickshift_density with the reference's parameters (ratio 0.5, kernel_size 3: 361 float64 exponentials a
                          pixel, one launch), N = 1 and --n, with one lane per pixel (MSTG_QUICKSHIFT_SPLIT=1), with four (=4) and as
                          the library chooses; ``exp_per_s`` is taps / time for the chosen variant;
  parents                 quickshift_parents of that density (max_dist 6: a 13 x 13 search square, one launch);
  flatten_number          quickshift_labels minus the two, from the library's per-launch profiler: the rounds of pointer jumping
                          and the four launches of the numbering;
  quickshift_labels       the whole segmentation (10 launches at 256 x 256);
  kernels                 the per-launch profiler (two device events around every launch) over ``--repeats`` calls of
                          quickshift_labels: the median duration of every kernel;
  blend_map               segment_blend_map of the quickshift labels with num_segments = H * W (what quickshift_segmenter passes:
                          no synchronisation) against num_segments = the true count (read back beforehand, outside the timing);
  end_to_end              process_enhanced_local_style of ONE 256 x 256 image with segmentation="felzenszwalb" (the host step), with
                          "slic" and with segments=quickshift_segmenter(), wall clock with a synchronise at both ends, median over
                          ``--repeats`` runs after a warm-up, all three in this one session;
  segmentation_host_ms    mstg_felzenszwalb_u8 per canvas on the host, for comparison.
The labels of a 64 x 72 crop of the first image are checked against tests/quickshift_ref.py run on the device's density.  Device
timings are device events around windows long enough to fill ``--seconds``, after a warm-up, with a synchronise at both ends; each
figure is reported as min / median / max over its repeats.  Prints one JSON line.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "multi-style-transfer-gan_amd"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

from bench_slic import DEV, DISTINCT, T, device_stats, kernel_times, wall_stats  # noqa: E402  (the same windows and statistics)

PARAMS = (0.5, 3, 6)  # the reference's call: ratio, kernel_size, max_dist


def with_split(split, fn):
    """fn with MSTG_QUICKSHIFT_SPLIT set to ``split`` (None: unset, the library chooses)"""
    def run():
        if split is None:
            os.environ.pop("MSTG_QUICKSHIFT_SPLIT", None)
        else:
            os.environ["MSTG_QUICKSHIFT_SPLIT"] = str(split)
        try:
            return fn()
        finally:
            os.environ.pop("MSTG_QUICKSHIFT_SPLIT", None)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_quickshift.py needs a GPU")
    import enhanced_generator as eg
    import enhanced_local_style_ref as ER
    import quickshift_ref as QR
    from mstg_hip import image as dimg
    ratio, ks, md = PARAMS
    distinct = [ER.smooth_noise(T, T, 100 + i, sigma=4.0 + 2 * i) for i in range(DISTINCT)]
    imgs = torch.from_numpy(np.stack([distinct[i % DISTINCT] for i in range(args.n)])).to(DEV)
    labels, count = dimg.quickshift_labels(imgs, *PARAMS, return_count=True)
    crop = np.ascontiguousarray(distinct[0][:64, :72])
    crop_dev = torch.from_numpy(crop).to(DEV)
    want = QR.quickshift(crop, *PARAMS, density=dimg.quickshift_density(crop_dev, ratio, ks).cpu().numpy())
    got, got_count = dimg.quickshift_labels(crop_dev, *PARAMS, return_count=True)
    w = QR.window(ks)
    taps = int(QR.taps(T, T, w).sum())
    result = {"H": T, "W": T, "ratio": ratio, "kernel_size": ks, "max_dist": md, "w": w, "taps_per_image": taps,
              "segments_per_image": count[:DISTINCT].cpu().tolist(),
              "device_equals_numpy_on_a_crop": bool(np.array_equal(want["labels"], got.cpu().numpy()) and want["count"] == int(got_count))}
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
    runs = max(args.repeats, 9)
    result["end_to_end"] = {s: wall_stats(lambda: dimg.process_enhanced_local_style(model, one, segmentation=s), runs) for s in dimg.SEGMENTATIONS}
    result["end_to_end"]["quickshift"] = wall_stats(lambda: dimg.process_enhanced_local_style(model, one, segments=dimg.quickshift_segmenter()), runs)
    for n in sorted({1, args.n}):
        x = imgs[:n]
        dens = dimg.quickshift_density(x, ratio, ks)
        r = {"density": device_stats(lambda: dimg.quickshift_density(x, ratio, ks), args.seconds, args.repeats),
             "density_split1": device_stats(with_split(1, lambda: dimg.quickshift_density(x, ratio, ks)), args.seconds, args.repeats),
             "density_split4": device_stats(with_split(4, lambda: dimg.quickshift_density(x, ratio, ks)), args.seconds, args.repeats),
             "parents": device_stats(lambda: dimg.quickshift_parents(x, dens, *PARAMS), args.seconds, args.repeats),
             "quickshift_labels": device_stats(lambda: dimg.quickshift_labels(x, *PARAMS), args.seconds, args.repeats)}
        r["density"]["exp_per_s"] = n * taps / (r["density"]["median_ms"] * 1e-3)
        r["kernels"] = kernel_times(lambda: dimg.quickshift_labels(x, *PARAMS), max(args.repeats, 5))
        r["flatten_number"] = {"median_ms": sum(v["median_ms"] * v["launches_per_call"] for k, v in r["kernels"].items() if "qs_" not in k),
                               "launches": sum(v["launches_per_call"] for k, v in r["kernels"].items() if "qs_" not in k)}
        lab, cnt = labels[:n], int(count[:n].max())
        r["blend_map"] = {"num_segments_hw": device_stats(lambda: dimg.segment_blend_map(x, lab, num_segments=T * T), args.seconds, args.repeats),
                          "num_segments_count": device_stats(lambda: dimg.segment_blend_map(x, lab, num_segments=cnt), args.seconds, args.repeats),
                          "count": cnt}
        result[f"N{n}"] = r
        for key in ("density", "density_split1", "density_split4", "parents", "quickshift_labels"):
            print(f"N = {n:3d}  {key:18s} {r[key]['median_ms']:10.3f} ms  [{r[key]['min_ms']:.3f} .. {r[key]['max_ms']:.3f}]", file=sys.stderr)
        print(f"N = {n:3d}  flatten + number   {r['flatten_number']['median_ms']:10.3f} ms in {r['flatten_number']['launches']} launches", file=sys.stderr)
        for key, v in r["blend_map"].items():
            if key != "count":
                print(f"N = {n:3d}  blend map, {key:20s} {v['median_ms']:10.3f} ms", file=sys.stderr)
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
