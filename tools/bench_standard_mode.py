"""MI355X: the finish of the application's standard mode (csrc/standard_mode.hip through mstg_hip.image.standard_finish) on a chunk
of 64 canvases at 256 x 256 that are already on the device: each stage alone, the chain, the mode end to end, and the host path
the chain replaces.

usage: python tools/bench_standard_mode.py [--n 64] [--seconds 0.5] [--repeats 7] [--host-repeats 3] [--json FILE]

  median, bilateral, lookup, blur   one stage entry alone on the chunk (d = 9, (75, 75); ksize 7), one launch each;
  chain                             standard_finish with the tab's defaults: three launches;
  chain_batch1                      the same on one canvas;
  end_to_end                        process_standard_batch with Generator(64).half_inference() on 64 images of 256 x 256:
                                    letterbox, forward in fp16, output conversion, the chain, resize back; ``forward_only`` is
                                    process_cyclegan_batch on the same images;
  host                              what a caller had to do before: device -> host copy of canvases and styled images,
                                    tests/standard_mode_ref.py (numpy; OpenCV is not installed) per canvas, host -> device copy of
                                    the result; ``host_batch1`` the same for one canvas.
The chain's bytes are checked against the host path on the first ``--check`` canvases.  Device timings are device events around
windows long enough to fill ``--seconds``, after a warm-up, with a synchronise at both ends; the host path is wall time around a
call that ends in a synchronise.  Each figure is reported as min / median / max over its repeats.  Prints one JSON line.  Needs a
GPU: there is no fallback."""
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
    s = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": min(s), "median_ms": statistics.median(s), "max_ms": max(s), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--model-type", default="photo_to_monet")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_standard_mode.py needs a GPU")
    import local_style_ref as LR
    import plain_generator
    import standard_mode_ref as SR
    from mstg_hip import _lib, image as dimg
    from mstg_hip.ops import _p, _stream
    lib = _lib.load()
    N, mt = args.n, args.model_type
    gens = [LR.landscape, LR.blocky, LR.gradient_rects, LR.noise]
    canv_np = np.stack([gens[i % 4](T, T, 100 + i) for i in range(N)])
    styled_np = np.ascontiguousarray(255 - canv_np[:, :, ::-1])
    canvas, styled = torch.from_numpy(canv_np).to(DEV), torch.from_numpy(styled_np).to(DEV)
    lut = dimg._color_lut(mt, torch.device(DEV))
    scratch = torch.empty_like(canvas)

    def lookup():
        _lib.check(lib.mstg_lut_u8(_p(canvas), N, T, T, _p(lut), _p(scratch), _stream()), "mstg_lut_u8")

    def chain(n=N):
        return dimg.standard_finish(canvas[:n], styled[:n], mt)

    def host_path(n=N):
        c, s = canvas[:n].cpu().numpy(), styled[:n].cpu().numpy()
        out = np.stack([SR.standard_finish(c[i], s[i], mt) for i in range(n)])
        return torch.from_numpy(out).to(DEV)

    k = max(1, min(args.check, N))
    same = bool(torch.equal(chain(k), host_path(k)))
    torch.manual_seed(0)
    model = plain_generator.Generator(64).to(DEV).half_inference().eval()
    images = [canvas[i] for i in range(N)]
    result = {"N": N, "H": T, "W": T, "model_type": mt, "chain_equals_host_restatement": same, "checked_canvases": k,
              "median": device_stats(lambda: dimg.median3_u8(canvas), args.seconds, args.repeats),
              "bilateral": device_stats(lambda: dimg.bilateral_u8(canvas), args.seconds, args.repeats),
              "lookup": device_stats(lookup, args.seconds, args.repeats),
              "blur": device_stats(lambda: dimg.gaussian_u8(canvas, 7), args.seconds, args.repeats),
              "chain": device_stats(chain, args.seconds, args.repeats),
              "chain_batch1": device_stats(lambda: chain(1), args.seconds, args.repeats),
              "end_to_end": device_stats(lambda: dimg.process_standard_batch(model, images, mt), args.seconds, args.repeats),
              "forward_only": device_stats(lambda: dimg.process_cyclegan_batch(model, images), args.seconds, args.repeats),
              "host_batch1": wall_stats(lambda: host_path(1), args.host_repeats),
              "host": wall_stats(host_path, args.host_repeats)}
    result["host_over_chain"] = result["host"]["median_ms"] / result["chain"]["median_ms"]
    result["host_over_chain_batch1"] = result["host_batch1"]["median_ms"] / result["chain_batch1"]["median_ms"]
    px = N * T * T
    result["bilateral_pixel_taps_per_s"] = px * 49 / (result["bilateral"]["median_ms"] * 1e-3)
    result["bilateral_bytes_per_s"] = px * 6 / (result["bilateral"]["median_ms"] * 1e-3)  # 3 bytes read and 3 written per pixel
    result["end_to_end_images_per_s"] = N / (result["end_to_end"]["median_ms"] * 1e-3)
    result["forward_only_images_per_s"] = N / (result["forward_only"]["median_ms"] * 1e-3)
    for key in ("median", "bilateral", "lookup", "blur", "chain", "chain_batch1", "end_to_end", "forward_only", "host_batch1", "host"):
        r = result[key]
        print(f"{key:14s} {r['median_ms']:12.3f} ms  [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]", file=sys.stderr)
    print(f"host / chain = {result['host_over_chain']:.0f}x (batch 1: {result['host_over_chain_batch1']:.0f}x)   chain equal: {same}   "
          f"bilateral {result['bilateral_pixel_taps_per_s'] / 1e9:.1f} G pixel-taps/s, {result['bilateral_bytes_per_s'] / 1e9:.1f} GB/s",
          file=sys.stderr)
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
