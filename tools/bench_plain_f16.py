"""MI355X: the plain CycleGAN Generator(64).eval() forward at 256 x 256 -- fp32 path, fp16 eager, fp16 graph replay -- and the
eight fp16 layers one by one (csrc/infer_f16_plain.hip).

usage: python tools/bench_plain_f16.py [--batches 1,16,64] [--repeats 5] [--seconds 0.3] [--json FILE]

Each figure is the median of ``--repeats`` timed windows (device events around enough forwards to fill ``--seconds``), taken after
a warm-up of the same shape; the windows of the three forms are interleaved so that a disturbance hits all of them, and the spread
(min .. max over the windows) is printed next to the median.  Per layer: algorithmic FLOP (2 per multiply-add, no padding) and
bytes (every tensor read once and written once) over the kernel time, as a share of the fp16 MFMA peak and of achievable HBM
bandwidth.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-style-transfer-gan_amd"))
sys.path.insert(0, ROOT)

PEAK_F16_TFLOPS = 2500.0   # dense fp16 MFMA, MI355X
ACHIEVABLE_HBM_GBS = 6300.0  # what a streaming float4 copy reaches on this part; shares below are against this figure
DEV = "cuda:0"


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters  # ms per call


def calibrate(fn, seconds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = window(fn, 3)
    return max(3, int(seconds * 1e3 / max(ms, 1e-3)))


def measure(forms, repeats, seconds):
    """forms: {name: fn}; returns {name: (median ms, min ms, max ms)} from interleaved windows."""
    iters = {k: calibrate(fn, seconds) for k, fn in forms.items()}
    samples = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            samples[k].append(window(fn, iters[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plain_f16.py needs a GPU")
    import plain_generator
    from oracle import restatement as R
    sd = R.make_state_dict(R.plain_generator_spec(args.channels), 7)

    def gen():
        m = plain_generator.Generator(channels=args.channels)
        m.load_state_dict(sd)
        return m.to(DEV).eval()
    m32, m16, mgr = gen(), gen().half_inference(), gen().half_inference().graph_inference()
    result = {"channels": args.channels, "size": args.size, "forward": {}, "layers": {}}
    torch.set_grad_enabled(False)
    for N in [int(v) for v in args.batches.split(",")]:
        x = R.make_input((N, 3, args.size, args.size), 11).to(DEV)
        y32, y16, ygr = m32(x), m16(x), mgr(x)
        err = float((y16.float() - y32).norm() / y32.norm())
        assert torch.equal(y16, ygr), "graph replay differs from eager"
        r = measure({"fp32": lambda: m32(x), "fp16 eager": lambda: m16(x), "fp16 graph": lambda: mgr(x)}, args.repeats, args.seconds)
        print(f"batch {N:3d} at {args.size}x{args.size}, channels={args.channels}   (fp16 vs fp32 output: rel-L2 {err:.2e})")
        for k, (med, lo, hi) in r.items():
            print(f"  {k:11s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  {N / med * 1e3:10.1f} images/s   x{r['fp32'][0] / med:5.2f} of fp32")
        result["forward"][N] = {k: {"ms": v[0], "min_ms": v[1], "max_ms": v[2], "images_per_s": N / v[0] * 1e3} for k, v in r.items()}
        result["forward"][N]["rel_l2"] = err
        # per layer: each packed layer on the activation its predecessor wrote
        plan = m16._half()
        from mstg_hip.infer_plain import TAP_NAMES
        layers = list(zip(TAP_NAMES, plan.layers)) + [("decoder.9", plan.head)]
        h = x
        rows = []
        total = 0.0
        for name, layer in layers:
            hin = h
            h = layer(hin)
            d = layer.desc(N, *(hin.shape[2:4] if layer.src_nchw_f32 else hin.shape[1:3]))
            flop = 2.0 * N * d.Ho * d.Wo * layer.Cin * layer.Cout * (4 if layer.kind == 1 else 16)
            nbytes = hin.numel() * hin.element_size() + h.numel() * 2 + layer.Cin * layer.Cout * 16 * 2
            med, lo, hi = measure({"l": lambda: layer(hin)}, args.repeats, args.seconds / 4)["l"]
            total += med
            tf, gbs = flop / med / 1e9, nbytes / med / 1e6
            roof_ms = max(flop / (PEAK_F16_TFLOPS * 1e9), nbytes / (ACHIEVABLE_HBM_GBS * 1e6))
            bound = "MFMA" if flop / (PEAK_F16_TFLOPS * 1e9) > nbytes / (ACHIEVABLE_HBM_GBS * 1e6) else "HBM"
            rows.append((name, med, lo, hi, tf, gbs))
            print(f"    {name:10s} {layer.Cin:3d}->{layer.Cout:3d}  {med * 1e3:8.1f} us [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  {tf:7.1f} TFLOP/s "
                  f"({100 * tf / PEAK_F16_TFLOPS:4.1f} % of fp16 MFMA)  {gbs:7.0f} GB/s ({100 * gbs / ACHIEVABLE_HBM_GBS:4.1f} % of achievable HBM)"
                  f"  roof {roof_ms * 1e3:6.1f} us ({bound}): {100 * roof_ms / med:4.1f} %")
        print(f"    sum of layers {total:.3f} ms (eager forward {r['fp16 eager'][0]:.3f} ms, graph {r['fp16 graph'][0]:.3f} ms)")
        result["layers"][N] = [{"layer": n, "ms": a, "min_ms": b, "max_ms": c, "tflops": t, "gbs": g} for n, a, b, c, t, g in rows]
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
