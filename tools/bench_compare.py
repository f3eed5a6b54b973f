"""MI355X: the mixed-size comparison (csrc/compare.hip through mstg_hip.metrics.pair_metrics) against the only other way to the
same bits, at one pair and at 64 pairs with ``a`` at 256 x 256 and ``b`` at sizes spread over 192 .. 320:

  (i)   fused        ``pair_metrics(A, B)``: every pair in two launches, the resize evaluated while b's patch is staged;
  (ii)  composition  per pair ``cv_resize_u8`` + ``image_metrics``: three launches and a resized image in memory per pair;
  (iii) floor        ``image_metrics`` on the same number of EQUAL-shape 256 x 256 pairs (no resize at all), one batched call.

usage: python tools/bench_compare.py [--reps 30] [--warmup 5] [--json FILE]

Per repetition the three are run one after the other (alternating, so that a drift of the machine hits all of them), each timed
with a host clock from a synchronised device to the synchronise after the call: what a caller waits for, host work included.
Reported: min / median / max over the repetitions.  A second pass with the library's per-launch profiler on gives the DEVICE time
of the kernels alone (sum per call, median over the repetitions) -- profiling slows the host, so those runs are not mixed with
the timed ones.  The decision rule of the design: the fused kernel stays only if its median is not above the
composition's by more than the observed spread, at both sizes.  Prints one JSON line.  Needs a GPU: there is no fallback."""
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
SIDE = 256


def b_sizes(P):
    """P (height, width) spread over 192 .. 320, none equal to 256 x 256"""
    rs = np.random.RandomState(P)
    sizes = []
    while len(sizes) < P:
        h, w = int(rs.randint(192, 321)), int(rs.randint(192, 321))
        if (h, w) != (SIDE, SIDE):
            sizes.append((h, w))
    return sizes


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6  # us


def kernel_us(lib, fn):
    """device time of the library's kernels in one call, by kernel name"""
    torch.cuda.synchronize()
    lib.mstg_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        out = {}
        name, ms = C.create_string_buffer(256), C.c_float()
        for i in range(lib.mstg_prof_count()):
            if lib.mstg_prof_get(i, name, 256, C.byref(ms)) == 0:
                k = name.value.decode()
                out[k] = out.get(k, 0.0) + ms.value * 1e3
        return out
    finally:
        lib.mstg_prof_enable(0)


def stats(v):
    return {"min_us": min(v), "median_us": statistics.median(v), "max_us": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_compare.py needs a GPU")
    if args.reps < 20:
        raise SystemExit("at least 20 timed repetitions")
    from mstg_hip import _lib, image as dimg, metrics
    lib = _lib.load()
    result = {"side": SIDE, "reps": args.reps, "warmup": args.warmup, "launches_fused": _lib.PAIR_METRICS_LAUNCHES, "sizes": []}
    for P in (1, 64):
        rs = np.random.RandomState(100 + P)
        A = [torch.from_numpy(rs.randint(0, 256, size=(SIDE, SIDE, 3)).astype(np.uint8)).to(DEV) for _ in range(P)]
        B = [torch.from_numpy(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).to(DEV) for h, w in b_sizes(P)]
        A4 = torch.stack(A)
        E4 = torch.from_numpy(rs.randint(0, 256, size=(P, SIDE, SIDE, 3)).astype(np.uint8)).to(DEV)

        def fused():
            return metrics.pair_metrics(A, B)

        def composition():
            return [metrics.image_metrics(a, dimg.cv_resize_u8(b, (SIDE, SIDE))) for a, b in zip(A, B)]

        def floor():
            return metrics.image_metrics(A4, E4)

        cases = (("fused", fused), ("composition", composition), ("floor", floor))
        got, want = fused(), composition()
        same = all(torch.equal(got[k][i], want[i][k][0]) for i in range(P) for k in got)
        for _ in range(args.warmup):
            for _, fn in cases:
                fn()
        samples = {n: [] for n, _ in cases}
        for _ in range(args.reps):
            for n, fn in cases:
                samples[n].append(timed(fn))
        kern = {n: [] for n, _ in cases}
        names = {}
        for _ in range(min(args.reps, 20)):
            for n, fn in cases:
                k = kernel_us(lib, fn)
                kern[n].append(sum(k.values()))
                names[n] = {key: round(v, 2) for key, v in k.items()}
        row = {"pairs": P, "bits_equal_to_composition": same}
        for n, _ in cases:
            row[n] = {**stats(samples[n]), "kernels_median_us": statistics.median(kern[n]), "kernels_last_call_us": names[n]}
        spread = max(row[n]["max_us"] - row[n]["min_us"] for n in ("fused", "composition"))
        row["spread_us"] = spread
        row["fused_stays"] = row["fused"]["median_us"] <= row["composition"]["median_us"] + spread
        result["sizes"].append(row)
        for n, _ in cases:
            r = row[n]
            print(f"P={P:3d} {n:12s} {r['median_us']:9.1f} us [{r['min_us']:.1f} .. {r['max_us']:.1f}]  kernels {r['kernels_median_us']:8.1f} us",
                  file=sys.stderr)
        print(f"P={P:3d} bits equal: {same}  spread {spread:.1f} us  fused stays: {row['fused_stays']}", file=sys.stderr)
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
