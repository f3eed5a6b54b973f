"""MI355X: the device image-quality metrics (csrc/metrics.hip through mstg_hip.metrics.image_metrics) at 256 x 256 and
1024 x 1024 with N = 1 and N = 64 pairs, against the float64 CPU restatement of the scikit-image evaluation on this machine.

usage: python tools/bench_metrics.py [--seconds 0.5] [--repeats 5] [--json FILE]

Per shape: the median of ``--repeats`` windows of device-event time per call, each window long enough to fill ``--seconds`` of
timed work, after a warm-up of the same shape and with a synchronise at both ends; the achieved rate on the algorithmic bytes
2 N H W 3 (each input byte read once; the result is 48 bytes per pair) as a share of achievable HBM bandwidth; and the wall time
of tests/metrics_ref.py for the same pairs (a Python loop over pairs, so it is timed on at most ``--cpu-pairs`` of them and
scaled to N; the JSON says how many were timed).  Prints one JSON line.  Needs a GPU: there is no fallback."""
import argparse
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

ACHIEVABLE_HBM_GBS = 6290.0  # what a streaming copy reaches on this part; the share below is against this figure
DEV = "cuda:0"
SHAPES = [(1, 256, 256), (64, 256, 256), (1, 1024, 1024), (64, 1024, 1024)]


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-pairs", type=int, default=4)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py needs a GPU")
    import metrics_ref as MR
    from mstg_hip import metrics
    result = {"achievable_hbm_gbs": ACHIEVABLE_HBM_GBS, "tile": [metrics.TILE_H, metrics.TILE_W], "shapes": []}
    for N, H, W in SHAPES:
        rs = np.random.RandomState(N + H)
        a_np = rs.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
        b_np = (a_np.astype(np.int16) + rs.randint(-30, 31, size=a_np.shape, dtype=np.int16)).clip(0, 255).astype(np.uint8)
        a, b = torch.from_numpy(a_np).to(DEV), torch.from_numpy(b_np).to(DEV)

        def call():
            return metrics.image_metrics(a, b)
        for _ in range(3):
            call()
        iters = max(3, int(args.seconds * 1e3 / max(window(call, 3), 1e-3)) + 1)
        samples = [window(call, iters) for _ in range(args.repeats)]
        ms = statistics.median(samples)
        nbytes = 2.0 * N * H * W * 3
        gbs = nbytes / ms / 1e6
        timed = min(N, args.cpu_pairs)
        MR.metrics(a_np[0], b_np[0])
        t0 = time.perf_counter()
        ref = [MR.metrics(a_np[i], b_np[i]) for i in range(timed)]
        cpu_ms = (time.perf_counter() - t0) * 1e3 / timed * N
        got = call()["ssim"][:timed].cpu().tolist()
        diff = max(abs(g - r["ssim"]) for g, r in zip(got, ref))
        row = {"N": N, "H": H, "W": W, "ms": ms, "min_ms": min(samples), "max_ms": max(samples), "iters_per_window": iters,
               "windows": args.repeats, "gbs": gbs, "share_of_achievable_hbm": gbs / ACHIEVABLE_HBM_GBS, "pairs_per_s": N / ms * 1e3,
               "cpu_ms": cpu_ms, "cpu_pairs_timed": timed, "speedup_over_cpu": cpu_ms / ms, "max_ssim_diff_vs_cpu": diff}
        result["shapes"].append(row)
        print(f"N={N:3d} {H}x{W}: {ms * 1e3:9.1f} us [{min(samples) * 1e3:.1f} .. {max(samples) * 1e3:.1f}]  {gbs:8.1f} GB/s "
              f"({100 * gbs / ACHIEVABLE_HBM_GBS:5.2f} % of achievable HBM)  CPU restatement {cpu_ms:9.1f} ms  x{cpu_ms / ms:8.0f}  "
              f"ssim diff {diff:.1e}", file=sys.stderr)
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
