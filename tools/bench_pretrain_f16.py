"""MI355X: one full pre-training step (``pretrain.PretrainStep``) of the plain CycleGAN Generator(64) in training mode at
256 x 256 -- the fp32 path (``amp=False``) against the mixed-precision path (``amp=True``), in one process -- and the kernels of the
mixed-precision step one by one.

usage: python tools/bench_pretrain_f16.py [--batches 1,16,64] [--repeats 5] [--seconds 0.5] [--json FILE]

Each figure is the median of ``--repeats`` timed windows (device events around enough steps to fill ``--seconds``, a device
synchronise inside the timed region), taken after a warm-up of the same shape; the windows of the two forms are interleaved so
that a disturbance hits both, and the spread (min .. max over the windows) is printed next to the median.  Per kernel (the
library's launch profiler, one profiled step): algorithmic FLOP (2 per multiply-add, no padding) and bytes (every tensor read
once and written once) over the kernel time, as a share of the fp16 MFMA peak and of achievable HBM bandwidth.  Needs a GPU:
there is no fallback."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-style-transfer-gan_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_plain_f16 import ACHIEVABLE_HBM_GBS, DEV, PEAK_F16_TFLOPS, measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pretrain_f16.py needs a GPU")
    import plain_generator
    import pretrain
    from emulate_plain_f16_train import pretrain_draw
    from mstg_hip import ops
    sd, _, _, _ = pretrain_draw(args.channels, 1, 16, 7)

    def step_of(amp):
        m = plain_generator.Generator(channels=args.channels)
        m.load_state_dict(sd)
        return pretrain.PretrainStep(m.to(DEV).train(), amp=amp)
    s32, s16 = step_of(False), step_of(True)
    result = {"channels": args.channels, "size": args.size, "step": {}, "kernels": {}}
    for N in [int(v) for v in args.batches.split(",")]:
        _, x, real, m = pretrain_draw(args.channels, N, args.size, 11)
        x, real, m = x.to(DEV), real.to(DEV), m.to(DEV)
        r = measure({"fp32": lambda: s32(x, real, m), "amp": lambda: s16(x, real, m)}, args.repeats, args.seconds)
        faster = r["amp"][2] < r["fp32"][1]  # every amp window below every fp32 window
        print(f"batch {N:3d} at {args.size}x{args.size}, channels={args.channels}: one PretrainStep call")
        for k, (med, lo, hi) in r.items():
            print(f"  {k:5s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  {N / med * 1e3:10.1f} images/s   x{r['fp32'][0] / med:5.2f} of fp32")
        print(f"  amp faster than fp32 by more than the spread: {'yes' if faster else 'NO'}")
        result["step"][N] = {k: {"ms": v[0], "min_ms": v[1], "max_ms": v[2]} for k, v in r.items()}
        result["step"][N]["amp_faster_beyond_spread"] = faster
        torch.cuda.synchronize()
        ops.KernelTimer.start()
        s16(x, real, m)
        torch.cuda.synchronize()
        ops.KernelTimer.stop()
        rows = sorted(ops.KernelTimer.summary().items(), key=lambda kv: -kv[1]["ms"])
        total = sum(v["ms"] for _, v in rows)
        print(f"    kernels of one amp step (profiled launches, {total:.3f} ms in all):")
        out = []
        for name, v in rows:
            tf, gbs = v["flops"] / max(v["ms"], 1e-9) / 1e9, v["bytes"] / max(v["ms"], 1e-9) / 1e6
            print(f"    {name[:56]:56s} x{v['launches']:3d} {v['ms'] * 1e3:9.1f} us {100 * v['ms'] / total:5.1f} %  {tf:7.1f} TFLOP/s "
                  f"({100 * tf / PEAK_F16_TFLOPS:4.1f} % of fp16 MFMA)  {gbs:7.0f} GB/s ({100 * gbs / ACHIEVABLE_HBM_GBS:4.1f} % of achievable HBM)")
            out.append({"kernel": name, "launches": v["launches"], "ms": v["ms"], "tflops": tf, "gbs": gbs})
        result["kernels"][N] = out
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
