"""MI355X: the device arithmetic of the reference's m_test.py -- ``mstg_hip.metrics.frechet_distance`` (csrc/frechet.hip) at
(n1, n2, d) = (100, 100, 2048), the reference's shape, and at the sample cap (256, 256, 2048), and
``mstg_hip.image.display_finish`` (csrc/display_finish.hip) for 1 and 64 images at 256 x 256 -- against the numpy / scipy
evaluation on this machine (tests/fid_ref.py reference_fid = np.cov + scipy.linalg.sqrtm; tests/display_finish_ref.py).

usage: python tools/bench_m_test.py [--seconds 0.3] [--repeats 5] [--json FILE]

Per case: the median of ``--repeats`` windows of device-event time per call, each window long enough to fill ``--seconds`` of timed
work, after a warm-up of the same shape and with a synchronise at both ends; the launches of one call and the median duration of
each kernel from the library's per-launch profiler (a run of its own); the sweeps the Jacobi used; the wall time of the CPU
evaluation (once) and the difference of the two results.  Prints one JSON line.  Needs a GPU: there is no fallback."""
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


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters  # ms per call


def timed(fn, seconds, repeats):
    for _ in range(3):
        fn()
    iters = max(3, int(seconds * 1e3 / max(window(fn, 3), 1e-3)) + 1)
    samples = [window(fn, iters) for _ in range(repeats)]
    return {"ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "iters_per_window": iters, "windows": repeats}


def kernel_times(fn, repeats=5):
    """median duration and launches per call of every kernel symbol of ``fn``"""
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
    kernels = {k: {"median_ms": statistics.median(v), "launches_per_call": len(v) // repeats} for k, v in per.items()}
    return kernels, sum(k["launches_per_call"] for k in kernels.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_m_test.py needs a GPU")
    import display_finish_ref as DR
    import fid_ref as FR
    from mstg_hip import image as dimg, metrics
    result = {"frechet_distance": [], "display_finish": []}
    for n1, n2, d in ((100, 100, 2048), (metrics.MAX_SAMPLES, metrics.MAX_SAMPLES, 2048)):
        x1, x2 = FR.draw(n1, n2, d, 7 + n1 + d, np.float32)
        a, b = torch.from_numpy(x1).to(DEV), torch.from_numpy(x2).to(DEV)

        def call():
            return metrics.frechet_distance(a, b, return_parts=True)
        row = {"n1": n1, "n2": n2, "d": d, **timed(call, args.seconds, args.repeats)}
        row["kernels"], row["launches"] = kernel_times(call)
        parts = call()
        row["sweeps"], row["converged"] = (int(v) for v in parts["info"].cpu())
        t0 = time.perf_counter()
        ref = FR.reference_fid(x1, x2)
        row["cpu_sqrtm_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        svd = FR.frechet(x1, x2)["fid"]
        row["cpu_numpy_svd_form_ms"] = (time.perf_counter() - t0) * 1e3
        fid = float(parts["fid"])
        row.update(fid=fid, rel_diff_vs_sqrtm=abs(fid - ref) / abs(ref), rel_diff_vs_numpy_svd_form=abs(fid - svd) / abs(svd),
                   speedup_over_sqrtm=row["cpu_sqrtm_ms"] / row["ms"])
        result["frechet_distance"].append(row)
        print(f"frechet_distance {(n1, n2, d)}: {row['ms'] * 1e3:9.1f} us [{row['min_ms'] * 1e3:.1f} .. {row['max_ms'] * 1e3:.1f}], "
              f"{row['launches']} launches, {row['sweeps']} sweeps; scipy sqrtm {row['cpu_sqrtm_ms']:.0f} ms, numpy SVD form "
              f"{row['cpu_numpy_svd_form_ms']:.1f} ms; rel diff {row['rel_diff_vs_sqrtm']:.1e} / {row['rel_diff_vs_numpy_svd_form']:.1e}",
              file=sys.stderr)
        for k, v in row["kernels"].items():
            print(f"    {k}: {v['median_ms'] * 1e3:.1f} us x {v['launches_per_call']}", file=sys.stderr)
    for N in (1, 64):
        y_np = np.tanh(np.random.RandomState(N).randn(N, 3, 256, 256) * 1.5).astype(np.float32)
        y = torch.from_numpy(y_np).to(DEV)

        def call():
            return dimg.display_finish(y)
        row = {"N": N, "H": 256, "W": 256, **timed(call, args.seconds, args.repeats)}
        row["kernels"], row["launches"] = kernel_times(call)
        t0 = time.perf_counter()
        ref = DR.display_finish(y_np)
        row["cpu_numpy_ms"] = (time.perf_counter() - t0) * 1e3
        row["bytes_differing_from_cpu"] = int((call().cpu().numpy() != ref).sum())
        row["images_per_s"] = N / row["ms"] * 1e3
        row["speedup_over_cpu"] = row["cpu_numpy_ms"] / row["ms"]
        result["display_finish"].append(row)
        print(f"display_finish N={N:2d} 256x256: {row['ms'] * 1e3:9.1f} us [{row['min_ms'] * 1e3:.1f} .. {row['max_ms'] * 1e3:.1f}], "
              f"{row['launches']} launches; numpy restatement {row['cpu_numpy_ms']:.1f} ms; {row['bytes_differing_from_cpu']} bytes differ",
              file=sys.stderr)
        for k, v in row["kernels"].items():
            print(f"    {k}: {v['median_ms'] * 1e3:.1f} us x {v['launches_per_call']}", file=sys.stderr)
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
