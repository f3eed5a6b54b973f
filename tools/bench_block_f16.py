"""MI355X: EnhancedGenerator inference with its StructuralTransformerBlocks -- fp32 path, ``half_inference()`` (blocks on the fp32
kernels) and ``half_inference(fp16_blocks=True)`` (blocks on csrc/infer_f16_block.hip) -- and the block's attention kernel alone,
fp32 ``flash_fwd_kernel<D>`` against fp16 ``blk_flash_f16_kernel<D>``.

usage: python tools/bench_block_f16.py [--repeats 5] [--seconds 0.3] [--quick] [--json FILE]

Each figure is the median of ``--repeats`` timed windows (device events around enough calls to fill ``--seconds``), taken after a
warm-up of the same shape; the windows of the forms compared are interleaved so that a disturbance hits all of them, and the
spread (min .. max over the windows) is printed next to the median.  Launches per forward: the library's kernel launches
(mstg_prof_count), torch's own kernels (the .float() / .half() conversions of the default half form) not included.
On a tree without the ``fp16_blocks`` keyword (the parent of the change that added it) only the forms that exist are timed: the
default half form then gives that tree's time.  Needs a GPU: there is no fallback."""
import argparse
import inspect
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-style-transfer-gan_amd"))
sys.path.insert(0, ROOT)

PEAK_F16_TFLOPS = 2500.0  # dense fp16 MFMA, MI355X
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
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = window(fn, 2)
    return max(2, int(seconds * 1e3 / max(ms, 1e-3)))


def measure(forms, repeats, seconds):
    """forms: {name: fn}; returns {name: (median ms, min ms, max ms)} from interleaved windows."""
    iters = {k: calibrate(fn, seconds) for k, fn in forms.items()}
    samples = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            samples[k].append(window(fn, iters[k]))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def launches(fn):
    from mstg_hip import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.mstg_prof_enable(1)
    fn()
    n = lib.mstg_prof_count()
    lib.mstg_prof_enable(0)
    torch.cuda.synchronize()
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--quick", action="store_true", help="256x256 batch 1 and 16 only, D = 16 attention only")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_block_f16.py needs a GPU")
    import enhanced_generator as eg
    from mstg_hip import ops
    from oracle import restatement as R
    has_blocks = "fp16_blocks" in inspect.signature(eg.EnhancedGenerator.half_inference).parameters
    torch.set_grad_enabled(False)
    result = {"fp16_blocks_available": has_blocks, "forward": [], "attention": []}

    def gen(C, nb, form):
        m = eg.EnhancedGenerator(channels=C, num_transformer_blocks=nb)
        m.load_state_dict(R.make_state_dict(R.generator_spec_with_blocks(C, nb), 7))
        m = m.to(DEV).eval()
        if form == "half":
            m.half_inference()
        elif form == "half+fp16_blocks":
            m.half_inference(fp16_blocks=True)
        return m

    cases = [(16, 1, 1, 256), (16, 1, 16, 256)] if args.quick else \
        [(16, 1, 1, 256), (16, 1, 16, 256), (16, 1, 64, 256), (16, 1, 1, 1024), (64, 3, 16, 256)]
    forms = ["fp32", "half"] + (["half+fp16_blocks"] if has_blocks else [])
    for C, nb, N, S in cases:
        models = {f: gen(C, nb, f) for f in forms}
        x = R.make_input((N, 3, S, S), 11).to(DEV)
        outs = {f: m(x) for f, m in models.items()}
        r = measure({f: (lambda m=m: m(x)) for f, m in models.items()}, args.repeats, args.seconds)
        row = {"channels": C, "blocks": nb, "batch": N, "size": S}
        print(f"EnhancedGenerator({C}, {nb}) at {S}x{S}, batch {N}")
        for f in forms:
            med, lo, hi = r[f]
            nl = launches(lambda: models[f](x)) if f != "fp32" else None
            err = float((outs[f].float() - outs["fp32"]).norm() / outs["fp32"].norm())
            print(f"  {f:17s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  {N / med * 1e3:9.1f} images/s  x{r['half'][0] / med:5.2f} of half"
                  + (f"  launches {nl}" if nl is not None else "") + f"  vs fp32 rel-L2 {err:.2e}")
            row[f] = {"ms": med, "min_ms": lo, "max_ms": hi, "launches": nl, "rel_l2_vs_fp32": err}
        result["forward"].append(row)
        del models, outs
        torch.cuda.empty_cache()

    if has_blocks:
        from mstg_hip import infer_block
    heads = 4
    acases = [(16, 1, 4096)] if args.quick else [(16, 16, 4096), (32, 16, 4096), (64, 16, 4096), (16, 1, 65536)]
    for D, N, L in acases:
        g = torch.Generator().manual_seed(5)
        qkv16 = torch.randn((N, L, 3 * heads * D), generator=g).half().to(DEV)
        qkv32 = qkv16.float()
        fns = {"fp32 flash_fwd_kernel": lambda: ops.flash_attention(qkv32, heads)}
        if has_blocks:
            fns["fp16 blk_flash_f16_kernel"] = lambda: infer_block.flash_attention(qkv16, heads)
        r = measure(fns, args.repeats, args.seconds)
        flop = 4.0 * N * heads * L * L * D
        row = {"D": D, "batch": N, "L": L, "heads": heads}
        print(f"attention D={D} heads={heads} L={L} batch {N}: {flop / 1e9:.1f} GFLOP")
        for k, (med, lo, hi) in r.items():
            tf = flop / med / 1e9
            print(f"  {k:26s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  {tf:7.1f} TFLOP/s ({100 * tf / PEAK_F16_TFLOPS:4.1f} % of fp16 MFMA peak)"
                  f"  x{r['fp32 flash_fwd_kernel'][0] / med:5.2f}")
            row[k] = {"ms": med, "min_ms": lo, "max_ms": hi, "tflops": tf}
        result["attention"].append(row)
        del qkv16, qkv32
        torch.cuda.empty_cache()
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
