"""MI355X: the multi-style loss alone -- VGG features + Gram matrices, forward + backward to dL/dy -- in fp32 and mixed precision
(style_loss.py precision="fp32" / "mixed"; csrc/style_f16.hip), full width, and the mixed path's kernels call by call.

usage: python tools/bench_style_f16.py [--shapes 32x512,32x256] [--repeats 5] [--seconds 1.0] [--width-div 1] [--json FILE]

Each time is the median of ``--repeats`` windows (device events around enough forward + backward passes to fill ``--seconds``) taken
after a warm-up of the same shape; the windows of the two precisions are interleaved so that a disturbance hits both, and the
spread (min .. max) is printed next to the median.  Per call of an instrumented pass (HIP events around every launch, a run of its
own): algorithmic FLOP (2 per multiply-add, no padding) over the kernel time as a share of the 16-bit (mixed) or fp32 MFMA peak.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-style-transfer-gan_amd"))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = {"mixed": 2500.0, "fp32": 157.3}  # dense fp16 / bf16 MFMA and v_mfma_f32_16x16x4_f32, MI355X
DEV = "cuda:0"


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(forms, repeats, seconds):
    iters = {}
    for k, fn in forms.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        iters[k] = max(2, int(seconds * 1e3 / max(window(fn, 2), 1e-3)))
    samples = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            samples[k].append(window(fn, iters[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x512,32x256", help="batch x side, comma separated")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--width-div", type=int, default=1)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_style_f16.py needs a GPU")
    import style_loss as sl
    from mstg_hip import ops
    from oracle import restatement as R
    result = {"width_div": args.width_div, "shapes": {}}
    for spec in args.shapes.split(","):
        N, S = (int(v) for v in spec.split("x"))
        styles = [R.make_input((2, 3, S, S), 80 + k).to(DEV) for k in range(3)]
        mods, ys = {}, {}
        for prec in ("fp32", "mixed"):
            feats = sl.VGGFeatures(width_div=args.width_div, precision=prec).to(DEV)
            mods[prec] = sl.MultiStyleGramLoss(feats, styles, (0.5, 0.3, 0.2), precision=prec)
            ys[prec] = R.make_input((N, 3, S, S), 79).to(DEV).requires_grad_(True)

        def run(prec):
            ys[prec].grad = None
            loss = mods[prec](ys[prec])
            loss.backward()
            return loss

        l32, lmx = float(run("fp32")), float(run("mixed"))
        dist = float((ys["mixed"].grad - ys["fp32"].grad).norm() / ys["fp32"].grad.norm())
        r = measure({p: (lambda p=p: run(p)) for p in ("fp32", "mixed")}, args.repeats, args.seconds)
        print(f"{N} x 3 x {S} x {S}, width_div={args.width_div}: loss fp32 {l32:.6e}  mixed {lmx:.6e} (rel {abs(lmx - l32) / abs(l32):.1e}); "
              f"dL/dy mixed vs fp32 rel-L2 {dist:.2e}, largest |dL/dy| {float(ys['fp32'].grad.abs().max()):.1e}")
        for p, (med, lo, hi) in r.items():
            print(f"  {p:5s} forward + backward {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  {N / med * 1e3:8.1f} images/s   x{r['fp32'][0] / med:5.2f} of fp32")
        entry = {p: {"ms": v[0], "min_ms": v[1], "max_ms": v[2]} for p, v in r.items()}
        entry.update(loss_fp32=l32, loss_mixed=lmx, dy_rel_l2=dist, calls={})
        for prec in ("mixed", "fp32"):  # instrumented passes, each a run of its own
            ops.KernelTimer.start()
            try:
                run(prec)
                torch.cuda.synchronize()
                rows = ops.KernelTimer.summary(detail=True, by_call=True)
                launches = len(ops.KernelTimer.kernels())
            finally:
                ops.KernelTimer.stop()
            total = sum(v["ms"] for v in rows.values())
            print(f"  {prec}: {launches} launches, {total:.3f} ms of kernel time in the instrumented pass")
            for name, v in sorted(rows.items(), key=lambda kv: -kv[1]["ms"]):
                tf = v["flops"] / v["ms"] / 1e9 if v["ms"] else 0.0
                print(f"    {name:64s} x{v['launches']:2d} {v['ms']:8.3f} ms  {tf:8.1f} TFLOP/s  {100 * tf / PEAK_TFLOPS[prec]:5.1f} % of the {prec} MFMA peak")
                entry["calls"][f"{prec} {name}"] = {"calls": v["launches"], "ms": v["ms"], "tflops": tf, "frac_of_peak": tf / PEAK_TFLOPS[prec]}
            conv = [v for k, v in rows.items() if "conv" in k and v["flops"]]
            if conv:
                cf, cm = sum(v["flops"] for v in conv), sum(v["ms"] for v in conv)
                print(f"    all convolutions: {cm:.3f} ms, {cf / cm / 1e9:.1f} TFLOP/s = {100 * cf / cm / 1e9 / PEAK_TFLOPS[prec]:.1f} % of the {prec} MFMA peak")
                entry[f"{prec}_conv_ms"], entry[f"{prec}_conv_tflops"] = cm, cf / cm / 1e9
        result["shapes"][spec] = entry
        del mods, ys, styles
        torch.cuda.empty_cache()
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
