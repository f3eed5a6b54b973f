"""MI355X: the colour-block repair (csrc/color_blocks.hip through mstg_hip.image.fix_color_blocks) on 1 and on 64 images of
256 x 256 that are already on the device: each stage alone, the chain, and the wide bilateral filter at radius 90 against two
yardsticks.

usage: python tools/bench_color_blocks.py [--n 64] [--seconds 0.5] [--repeats 5] [--json FILE]

  mask, correction, bilateral_wide, detail_blend   one stage function alone (the reference's constants), for N = 1 and N = --n;
  chain, chain_orig                                fix_color_blocks without and with an original: five and seven launches;
  first yardstick    mstg_bilateral_u8(d = 9) on the same images, timed in the same call in alternating windows; both in
                     tap-pixels per second (49 and 25 445 taps a pixel): ``wide_over_narrow_rate`` is the ratio of the rates;
  second yardstick   the vector-issue floor: ``--instr-per-tap`` vector instructions a tap-pixel (counted from the ISA of the inner
                     loop) * tap-pixels over 256 CUs * 4 SIMDs * 32 lanes a clock at 2.4 GHz;
                     ``share_of_issue_floor`` = floor / measured.
The numpy restatement through the host is not compared: one 256 x 256 image at radius 90 takes it longer than a minute.  The bytes
of the chain are checked against the composed stage functions on the first image.  Device timings are device events around windows
long enough to fill ``--seconds``, after a warm-up, with a synchronise at both ends; each figure is reported as min / median / max
over its repeats.  Prints one JSON line.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "multi-style-transfer-gan_amd"), ROOT):
    sys.path.insert(0, p)

DEV = "cuda:0"
T = 256
WIDE_TAPS, NARROW_TAPS = 25445, 49
LANES_PER_CLOCK, CLOCK_HZ = 256 * 4 * 32, 2.4e9


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters  # ms per call


def _iters(fn, seconds):
    for _ in range(2):
        fn()
    return max(2, int(seconds * 1e3 / max(window(fn, 2), 1e-3)) + 1)


def _stats(s, iters):
    return {"min_ms": min(s), "median_ms": statistics.median(s), "max_ms": max(s), "iters_per_window": iters, "windows": len(s)}


def device_stats(fn, seconds, repeats):
    iters = _iters(fn, seconds)
    return _stats([window(fn, iters) for _ in range(repeats)], iters)


def alternating(fa, fb, seconds, repeats):
    """two functions timed in alternating windows of one call, so that clocks and temperature are shared"""
    ia, ib = _iters(fa, seconds), _iters(fb, seconds)
    sa, sb = [], []
    for _ in range(repeats):
        sa.append(window(fa, ia))
        sb.append(window(fb, ib))
    return _stats(sa, ia), _stats(sb, ib)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--instr-per-tap", type=float, default=7.75)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_color_blocks.py needs a GPU")
    import color_blocks_ref as CR
    import local_style_ref as LR
    from mstg_hip import image as dimg
    gens = [LR.landscape, LR.blocky, LR.gradient_rects, LR.noise]
    imgs_np = np.stack([gens[i % 4](T, T, 100 + i) if i % 5 else CR.blocks(T, T, i) for i in range(args.n)])
    imgs = torch.from_numpy(imgs_np).to(DEV)
    origs = torch.from_numpy(np.ascontiguousarray(255 - imgs_np[:, :, ::-1])).to(DEV)
    first = dimg.fix_color_blocks(imgs[0], origs[0])
    composed = dimg.detail_enhancing_blend(dimg.edge_preserving_smoothing(dimg.adaptive_color_correction(imgs[0], dimg.detect_color_blocks(
        imgs[0]))), origs[0], alpha=0.1, beta=0.5)
    result = {"H": T, "W": T, "chain_equals_composed_stages": bool(torch.equal(first, composed)),
              "flagged_share": float(dimg.detect_color_blocks(imgs).float().mean())}
    for n in sorted({1, args.n}):
        x, o = imgs[:n], origs[:n]
        m = dimg.detect_color_blocks(x)
        r = {"mask": device_stats(lambda: dimg.detect_color_blocks(x), args.seconds, args.repeats),
             "correction": device_stats(lambda: dimg.adaptive_color_correction(x, m), args.seconds, args.repeats),
             "detail_blend": device_stats(lambda: dimg.detail_enhancing_blend(x, o, 0.1, 0.5), args.seconds, args.repeats),
             "chain": device_stats(lambda: dimg.fix_color_blocks(x), args.seconds, args.repeats),
             "chain_orig": device_stats(lambda: dimg.fix_color_blocks(x, o), args.seconds, args.repeats)}
        r["bilateral_wide"], r["bilateral_d9"] = alternating(lambda: dimg.edge_preserving_smoothing(x), lambda: dimg.bilateral_u8(x),
                                                             args.seconds, args.repeats)
        px = n * T * T
        wide_rate = px * WIDE_TAPS / (r["bilateral_wide"]["median_ms"] * 1e-3)
        narrow_rate = px * NARROW_TAPS / (r["bilateral_d9"]["median_ms"] * 1e-3)
        floor_ms = args.instr_per_tap * px * WIDE_TAPS / (LANES_PER_CLOCK * CLOCK_HZ) * 1e3
        r.update(wide_tap_pixels_per_s=wide_rate, narrow_tap_pixels_per_s=narrow_rate, wide_over_narrow_rate=wide_rate / narrow_rate,
                 issue_floor_ms=floor_ms, share_of_issue_floor=floor_ms / r["bilateral_wide"]["median_ms"],
                 bilateral_wide_ms_per_image=r["bilateral_wide"]["median_ms"] / n, numpy_restatement="not compared")
        result[f"N{n}"] = r
        for key in ("mask", "correction", "bilateral_wide", "bilateral_d9", "detail_blend", "chain", "chain_orig"):
            print(f"N = {n:3d}  {key:15s} {r[key]['median_ms']:12.3f} ms  [{r[key]['min_ms']:.3f} .. {r[key]['max_ms']:.3f}]", file=sys.stderr)
        print(f"N = {n:3d}  wide {wide_rate / 1e9:.1f} G tap-pixels/s, d = 9 {narrow_rate / 1e9:.1f} G tap-pixels/s, ratio "
              f"{wide_rate / narrow_rate:.2f}; issue floor {floor_ms:.3f} ms = {100 * r['share_of_issue_floor']:.0f} % of the measured time",
              file=sys.stderr)
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
