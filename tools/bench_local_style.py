"""MI355X: the 'enhanced' local-style weight map of a chunk of 64 canvases at 256 x 256, built on the device
(csrc/local_style.hip through mstg_hip.image.enhanced_weight_map) and blended with mstg_blend_u8, against the host path it
replaces and against the blend with maps that already exist.

usage: python tools/bench_local_style.py [--n 64] [--seconds 0.5] [--repeats 7] [--host-repeats 3] [--json FILE]

Three ways through the same chunk, each ending in the same blended (N, 256, 256, 3) bytes (checked):
  device      enhanced_weight_map (three launches) + the blend, everything on the GPU;
  host        device -> host copy of the canvases, tests/local_style_ref.py (numpy / scipy; OpenCV is not installed) per canvas,
              host -> device copy of the float64 maps, the blend -- what a caller of mode="weight_map" had to do before;
  floor       the blend with maps computed beforehand: ``floor_upload`` stacks and uploads host maps as the batched pipeline does
              for caller-supplied maps, ``floor_resident`` has them on the device already.
A further row is the reference's default mode, ``mode="enhanced"`` with enhance_colors and smooth: ``enhanced`` is the four
launches from the canvas batch to the finished bytes (mstg_local_style_enhanced), ``finish`` the fourth launch alone on a resident
map and detail mask (``finish_no_smooth``: the same without the smoothing, which then pays for no halo), checked against
tests/local_style_finish_ref.py on the first four canvases.
Device timings are device events around windows long enough to fill ``--seconds``, after a warm-up, with a synchronise at both
ends; the host path is wall time around a call that ends in a synchronise.  Each figure is reported as min / median / max over
its repeats.  Stage B (the hysteresis, one workgroup per image) is also timed alone through the library's per-launch profiler for
64 copies of a natural canvas's state map and for 64 copies of the 256 x 256 spiral of tests/local_style_ref.py, its worst case.
Prints one JSON line.  Needs a GPU: there is no fallback."""
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

DEV = "cuda:0"
T = 256


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
    for _ in range(3):
        fn()
    iters = max(3, int(seconds * 1e3 / max(window(fn, 3), 1e-3)) + 1)
    s = [window(fn, iters) for _ in range(repeats)]
    return {"min_ms": min(s), "median_ms": statistics.median(s), "max_ms": max(s), "iters_per_window": iters, "windows": repeats}


def wall_stats(fn, repeats):
    fn()
    s = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": min(s), "median_ms": statistics.median(s), "max_ms": max(s), "repeats": repeats}


def stage_b_stats(lib, states, repeats):
    """device time of local_style_hysteresis_kernel alone on an (N, H, W) uint8 state batch, from the per-launch profiler"""
    import ctypes as C
    from mstg_hip import _lib
    from mstg_hip.ops import _p, _stream
    N, H, W = states.shape
    edge = torch.empty_like(states)
    s = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        lib.mstg_prof_enable(1)
        try:
            _lib.check(lib.mstg_local_style_hysteresis(_p(states), N, H, W, _p(edge), _stream()), "mstg_local_style_hysteresis")
            torch.cuda.synchronize()
            name, ms = C.create_string_buffer(256), C.c_float()
            _lib.check(lib.mstg_prof_get(0, name, 256, C.byref(ms)), "mstg_prof_get")
        finally:
            lib.mstg_prof_enable(0)
        s.append(ms.value)
    s = s[1:]  # the first launch loads the code object
    return {"min_ms": min(s), "median_ms": statistics.median(s), "max_ms": max(s), "repeats": repeats, "edge_pixels": int(edge[0].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_local_style.py needs a GPU")
    import local_style_ref as LR
    from mstg_hip import _lib, image as dimg
    lib = _lib.load()
    N = args.n
    gens = [LR.landscape, LR.blocky, LR.gradient_rects, LR.bright_low_saturation]
    canv_np = np.stack([gens[i % 4](T, T, 100 + i) for i in range(N)])
    styled_np = np.ascontiguousarray(255 - canv_np[:, :, ::-1])
    canvas, styled = torch.from_numpy(canv_np).to(DEV), torch.from_numpy(styled_np).to(DEV)
    tall = lambda t: t.view(N * T, T, 3)  # noqa: E731  the batch as one tall image, as the batched pipeline blends it

    def device_path():
        wm = dimg.enhanced_weight_map(canvas)
        return dimg.blend_u8(tall(canvas), tall(styled), weight_map=wm.view(N * T, T))

    def host_maps():
        c = canvas.cpu().numpy()
        return [LR.enhanced_weight_map(c[i])["weight"] for i in range(N)]

    def host_path():
        maps = host_maps()
        wm = torch.stack([torch.as_tensor(m) for m in maps]).to(device=DEV, dtype=torch.float64).contiguous()
        return dimg.blend_u8(tall(canvas), tall(styled), weight_map=wm.view(N * T, T))

    maps_host = host_maps()
    maps_dev = torch.from_numpy(np.stack(maps_host)).to(DEV)

    def floor_upload():
        wm = torch.stack([torch.as_tensor(m) for m in maps_host]).to(device=DEV, dtype=torch.float64).contiguous()
        return dimg.blend_u8(tall(canvas), tall(styled), weight_map=wm.view(N * T, T))

    def floor_resident():
        return dimg.blend_u8(tall(canvas), tall(styled), weight_map=maps_dev.view(N * T, T))

    def map_only():
        return dimg.enhanced_weight_map(canvas)

    import local_style_finish_ref as FR
    wm_dev, _, _, det_dev, _ = dimg.enhanced_weight_map(canvas, return_masks=True)

    def enhanced():
        return dimg._local_style_enhanced(canvas, styled, 0.8, 0.7, 0.3, True, True)

    def finish():
        return dimg.local_style_finish(canvas, styled, wm_dev, det_dev)

    def finish_no_smooth():
        return dimg.local_style_finish(canvas, styled, wm_dev, None, smooth=False)

    enh = enhanced()
    same_enh = bool(torch.equal(enh, finish())) and all(
        np.array_equal(enh[i].cpu().numpy(), FR.enhanced_ref(canv_np[i], styled_np[i])[0]) for i in range(min(N, 4)))

    out_dev = device_path()
    same_map = bool(torch.equal(dimg.enhanced_weight_map(canvas), maps_dev))
    same_bytes = bool(torch.equal(out_dev, host_path()) and torch.equal(out_dev, floor_resident()))
    result = {"N": N, "H": T, "W": T, "map_equals_host_restatement": same_map, "blend_equals_host_path": same_bytes,
              "device": device_stats(device_path, args.seconds, args.repeats),
              "device_map_only": device_stats(map_only, args.seconds, args.repeats),
              "floor_resident": device_stats(floor_resident, args.seconds, args.repeats),
              "floor_upload": wall_stats(floor_upload, args.repeats),
              "host": wall_stats(host_path, args.host_repeats)}
    result["enhanced_equals_host_restatement"] = same_enh
    result["enhanced"] = device_stats(enhanced, args.seconds, args.repeats)
    result["finish"] = device_stats(finish, args.seconds, args.repeats)
    result["finish_no_smooth"] = device_stats(finish_no_smooth, args.seconds, args.repeats)
    result["host_over_device"] = result["host"]["median_ms"] / result["device"]["median_ms"]
    natural = torch.from_numpy(np.stack([LR.state_map(LR.gray_u8(canv_np[0]))] * N)).to(DEV)
    spiral = torch.from_numpy(np.stack([LR.spiral_state(T, T)] * N)).to(DEV)
    result["stage_b_natural"] = stage_b_stats(lib, natural, args.repeats)
    result["stage_b_spiral"] = stage_b_stats(lib, spiral, args.repeats)
    for k in ("device", "device_map_only", "floor_resident", "floor_upload", "host", "enhanced", "finish", "finish_no_smooth", "stage_b_natural",
              "stage_b_spiral"):
        r = result[k]
        print(f"{k:16s} {r['median_ms']:10.3f} ms  [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]", file=sys.stderr)
    print(f"host / device = {result['host_over_device']:.0f}x   map equal: {same_map}   bytes equal: {same_bytes}   enhanced equal: {same_enh}",
          file=sys.stderr)
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
