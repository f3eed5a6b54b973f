"""MI355X: the advanced transform (csrc/advanced_transform.hip through mstg_hip.image) on 1 and on 64 images of 256 x 256 that are
already on the device.

usage: python tools/bench_advanced_transform.py [--n 64] [--seconds 0.3] [--repeats 5] [--json FILE]

  stages                  lab_u8, lab2rgb_u8, gaussian_sigma_u8(3), hsv_gain_u8 beside the existing hsv_enhance_u8, kmeans_u8 (K = 5,
                          10 attempts, 10 iterations), region_blend_u8, fuse_scales_u8 (three scales), for N = 1 and N = --n;
  chains                  contrast_enhanced_finish, detail_enhanced_finish, local_regions_finish;
  kernels                 the library's per-launch profiler (two device events around every launch) over ``--repeats`` calls of
                          the three chains: the median duration of every kernel;
  kmeans_per_iteration    the medians of km_assign_kernel and km_update_kernel, and the duration of every assignment launch of one
                          call in launch order (a frozen problem returns at once, so later rounds are shorter);
  numpy_restatement_ms    tests/advanced_transform_ref.py through the host for ONE image: every stage and chain.
The bytes of every chain are checked against the composed stage functions and against the restatement on the first image.  Device
timings are device events around windows long enough to fill ``--seconds``, after a warm-up, with a synchronise at both ends;
each figure is reported as min / median / max over its repeats.  Prints one JSON line.  Needs a GPU: there is no fallback."""
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
    return {k: {"median_ms": statistics.median(v), "launches_per_call": len(v) / repeats} for k, v in per.items()}


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_advanced_transform.py needs a GPU")
    import advanced_transform_ref as AR
    import enhanced_local_style_ref as ER
    from mstg_hip import image as dimg
    distinct = [ER.smooth_noise(T, T, 100 + i, sigma=4.0 + 2 * i) for i in range(DISTINCT)]
    orig = torch.from_numpy(np.stack([distinct[i % DISTINCT] for i in range(args.n)])).to(DEV)
    styled = torch.from_numpy(np.ascontiguousarray(255 - np.stack([distinct[(i + 1) % DISTINCT] for i in range(args.n)])[..., ::-1])).to(DEV)
    s0, o0 = styled[0].cpu().numpy(), orig[0].cpu().numpy()
    labels = dimg.kmeans_u8(orig, seed=0)[0]
    # the chains against their stages and against the restatement, first image
    lab = dimg.lab_u8(styled[0])
    lab[..., 0] = dimg.clahe_u8(lab[..., 0].contiguous())
    contrast = dimg.contrast_enhanced_finish(styled[0])
    detail = dimg.detail_enhanced_finish(styled[0], orig[0])
    regions = dimg.local_regions_finish(styled[0], orig[0], seed=0)
    ref = {}
    ms = {}
    ms["lab_u8"], ref_lab = host_ms(lambda: AR.lab_u8(s0))
    ms["lab2rgb_u8"], _ = host_ms(lambda: AR.lab2rgb_u8(ref_lab))
    ms["gaussian_sigma_u8"], _ = host_ms(lambda: AR.gaussian_sigma_u8(np.ascontiguousarray(o0[..., 1]), 3.0))
    ms["hsv_gain_u8"], _ = host_ms(lambda: AR.hsv_gain_u8(s0, 1.2, 1.0))
    ms["hsv_enhance_u8"], _ = host_ms(lambda: ER.hsv_enhance(s0))
    ms["kmeans_u8"], ref_km = host_ms(lambda: AR.kmeans_u8(o0, seed=0))
    ms["region_blend_u8"], _ = host_ms(lambda: AR.region_blend_u8(s0, o0, ref_km[0]))
    ms["fuse_scales_u8"], _ = host_ms(lambda: AR.fuse_scales_u8([s0, o0, s0]))
    ms["contrast_enhanced_finish"], ref["contrast"] = host_ms(lambda: AR.contrast_enhanced_finish(s0))
    ms["detail_enhanced_finish"], ref["detail"] = host_ms(lambda: AR.detail_enhanced_finish(s0, o0))
    ms["local_regions_finish"], ref["regions"] = host_ms(lambda: AR.local_regions_finish(s0, o0, seed=0))
    result = {"H": T, "W": T, "numpy_restatement_ms": ms,
              "chains_equal_composed_stages": bool(
                  torch.equal(contrast, dimg.hsv_gain_u8(dimg.lab2rgb_u8(lab), 1.2, 1.0))
                  and torch.equal(regions, dimg.hsv_gain_u8(dimg.region_blend_u8(styled[0], orig[0], labels[0]), 1.2, 1.0))),
              "device_equals_numpy_on_first_image": bool(
                  np.array_equal(ref["contrast"], contrast.cpu().numpy()) and np.array_equal(ref["detail"], detail.cpu().numpy())
                  and np.array_equal(ref["regions"], regions.cpu().numpy()) and np.array_equal(ref_km[0], labels[0].cpu().numpy()))}
    for n in sorted({1, args.n}):
        st, o, lb = styled[:n], orig[:n], labels[:n]
        plane = o[..., 1].contiguous()
        three = torch.stack([st, o, st])
        labn = dimg.lab_u8(st)
        fns = {"lab_u8": lambda: dimg.lab_u8(st), "lab2rgb_u8": lambda: dimg.lab2rgb_u8(labn),
               "gaussian_sigma_u8": lambda: dimg.gaussian_sigma_u8(plane, 3.0), "hsv_gain_u8": lambda: dimg.hsv_gain_u8(st, 1.2, 1.0),
               "hsv_enhance_u8": lambda: dimg.hsv_enhance_u8(st), "kmeans_u8": lambda: dimg.kmeans_u8(o, seed=0),
               "region_blend_u8": lambda: dimg.region_blend_u8(st, o, lb), "fuse_scales_u8": lambda: dimg.fuse_scales_u8(three),
               "contrast_enhanced_finish": lambda: dimg.contrast_enhanced_finish(st),
               "detail_enhanced_finish": lambda: dimg.detail_enhanced_finish(st, o),
               "local_regions_finish": lambda: dimg.local_regions_finish(st, o, seed=0)}
        r = {k: device_stats(f, args.seconds, args.repeats) for k, f in fns.items()}
        r["kernels"] = kernel_times(lambda: (fns["contrast_enhanced_finish"](), fns["detail_enhanced_finish"](), fns["local_regions_finish"]()),
                                    max(args.repeats, 5))
        # the K-means round by round: every assignment launch of one call, in order (11 of them; the last assigns every problem)
        rounds = kernel_rounds(fns["kmeans_u8"], "km_assign_kernel")
        r["kmeans_assign_ms_by_round"] = rounds
        assign = next((v["median_ms"] for k, v in r["kernels"].items() if "km_assign_kernel" in k), None)
        update = next((v["median_ms"] for k, v in r["kernels"].items() if "km_update_kernel" in k), None)
        r["kmeans_per_iteration_ms"] = {"assign_median": assign, "update_median": update, "assign_first_round": rounds[0] if rounds else None,
                                        "pixels_x_attempts_per_s_first_round": n * 10 * T * T / (rounds[0] * 1e-3) if rounds else None}
        result[f"N{n}"] = r
        for key in fns:
            print(f"N = {n:3d}  {key:26s} {r[key]['median_ms']:10.3f} ms  [{r[key]['min_ms']:.3f} .. {r[key]['max_ms']:.3f}]"
                  f"   numpy, one image: {ms[key]:9.1f} ms", file=sys.stderr)
        for k, v in sorted(r["kernels"].items()):
            print(f"N = {n:3d}    {k[:60]:60s} {v['median_ms'] * 1e3:10.1f} us x {v['launches_per_call']:.0f}", file=sys.stderr)
        print(f"N = {n:3d}    km_assign_kernel by round (us): {[round(v * 1e3, 1) for v in rounds]}", file=sys.stderr)
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


def kernel_rounds(fn, kernel):
    """the durations (ms) of every launch of ``kernel`` in ONE call of ``fn``, in launch order"""
    from mstg_hip import _lib
    lib = _lib.load()
    fn()
    torch.cuda.synchronize()
    lib.mstg_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        out = []
        name, ms = C.create_string_buffer(256), C.c_float()
        for i in range(lib.mstg_prof_count()):
            lib.mstg_prof_get(i, name, 256, C.byref(ms))
            if kernel in name.value.decode():
                out.append(ms.value)
    finally:
        lib.mstg_prof_enable(0)
    return out


if __name__ == "__main__":
    main()
