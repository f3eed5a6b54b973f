"""MI355X: the transformer block's attention in training, fp32 kernels (csrc/transformer.hip) against the mixed-precision ones
(csrc/flash_f16_train.hip, ``ops.flash_attention(..., precision="mixed")``), and the EnhancedCycleGAN train step with a block in both
precisions, next to the block-free step for scale.

usage: python tools/bench_flash_f16_train.py [--repeats 5] [--seconds 0.3] [--quick] [--json FILE]

Each figure is the median of ``--repeats`` timed windows (device events around enough calls to fill ``--seconds``), taken after a
warm-up of the same shape; the windows of the forms compared alternate in one process so that a disturbance hits both, and the
spread (min .. max over the windows) is printed next to the median.
  forward            ops.flash_attention under no_grad (mixed: the cast pass and the forward kernel)
  backward           the C entry alone on saved tensors (fp32: delta, dQ, dK/dV; mixed: bf16 dO, delta + dQ, dK/dV)
  forward+backward   ops.flash_attention and torch.autograd.grad, what a train step runs
Gate: mixed is faster than fp32 by more than the two forms' combined min .. max spread -- forward+backward at each shape, and the
train step with a block.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-style-transfer-gan_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_block_f16 import DEV, calibrate, measure, window  # noqa: E402

HEADS = 4


def gate(r, slow, fast):
    """(passes, gain ms, combined spread ms): r = {form: (median, min, max)}"""
    gain = r[slow][0] - r[fast][0]
    spread = (r[slow][2] - r[slow][1]) + (r[fast][2] - r[fast][1])
    return bool(gain > spread), gain, spread


def show(r, base):
    for k, (med, lo, hi) in r.items():
        print(f"    {k:6s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  x{r[base][0] / med:5.2f}")


def attention_case(D, L, N, args):
    from mstg_hip import _lib, ops
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    dim = HEADS * D
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn((N, L, 3 * dim), generator=g) * 0.8).to(DEV)
    gy = torch.randn((N, L, dim), generator=g).to(DEV)
    qg = qkv.clone().requires_grad_(True)

    def fwd(p):
        with torch.no_grad():
            return ops.flash_attention(qkv, HEADS, precision=p)

    def both(p):
        return torch.autograd.grad(ops.flash_attention(qg, HEADS, precision=p), [qg], [gy])[0]

    # saved tensors of the two forms for the backward entries alone
    out = torch.empty((N, L, dim), device=DEV)
    lse = torch.empty((N, HEADS, L), device=DEV)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((N, HEADS, L), device=DEV)
    _lib.check(lib.mstg_flash_attn_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), N, L, HEADS, D, st), "fwd")
    qh, qb = torch.empty_like(qkv, dtype=torch.float16), torch.empty_like(qkv, dtype=torch.bfloat16)
    outm, lsem = torch.empty_like(out), torch.empty_like(lse)
    ws = torch.empty(lib.mstg_f16_flash_attn_train_bwd_workspace_bytes(N, L, HEADS, D) // 4 + 4, device=DEV)
    _lib.check(lib.mstg_f16_attn_cast_qkv(qkv.data_ptr(), qh.data_ptr(), qb.data_ptr(), N, L, HEADS, D, st), "cast")
    _lib.check(lib.mstg_f16_flash_attn_train_fwd(qh.data_ptr(), outm.data_ptr(), lsem.data_ptr(), N, L, HEADS, D, st), "fwd")

    def bwd(p):
        if p == "fp32":
            _lib.check(lib.mstg_flash_attn_bwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), gy.data_ptr(), dqkv.data_ptr(),
                                               delta.data_ptr(), N, L, HEADS, D, st), "bwd")
        else:
            _lib.check(lib.mstg_f16_flash_attn_train_bwd(qh.data_ptr(), qb.data_ptr(), lsem.data_ptr(), gy.data_ptr(),
                                                         dqkv.data_ptr(), ws.data_ptr(), ws.numel() * 4, N, L, HEADS, D, st), "bwd")

    flop = 4.0 * N * HEADS * L * L * D  # one forward; the backward is 2.5 x that as an algorithm (five L x L x D products)
    row = {"D": D, "L": L, "batch": N, "heads": HEADS, "forward_gflop": flop / 1e9}
    print(f"attention D={D} heads={HEADS} L={L} batch {N}: forward {flop / 1e9:.1f} GFLOP")
    for name, fn in (("forward", fwd), ("backward", bwd), ("forward+backward", both)):
        r = measure({p: (lambda p=p: fn(p)) for p in ("fp32", "mixed")}, args.repeats, args.seconds)
        ok, gain, spread = gate(r, "fp32", "mixed")
        print(f"  {name}: gain {gain:.3f} ms, combined spread {spread:.3f} ms")
        show(r, "fp32")
        row[name] = {p: {"ms": v[0], "min_ms": v[1], "max_ms": v[2]} for p, v in r.items()}
        row[name].update(speedup=r["fp32"][0] / r["mixed"][0], gain_ms=gain, spread_ms=spread, faster_beyond_spread=ok)
    gm = both("mixed")
    g32 = both("fp32")
    row["dqkv_rel_l2_vs_fp32"] = float((gm - g32).norm() / g32.norm())
    return row


def step_case(pairs, size, args):
    import enhanced_train
    from oracle import restatement as R

    def model(nb, precision):
        torch.manual_seed(7)
        return enhanced_train.EnhancedCycleGAN(channels=16, num_transformer_blocks=nb, device=torch.device(DEV),
                                               attention_precision=precision)

    a, b = R.make_input((pairs, 3, size, size), 21).to(DEV), R.make_input((pairs, 3, size, size), 22).to(DEV)
    models = {"fp32": model(1, "fp32"), "mixed": model(1, "mixed"), "blocks=0": model(0, "fp32")}
    # Windows of at least two seconds (a step is ~20 ms) and one untimed round of windows in front: the first steps size workspaces,
    # optimizer state and the allocator's pools, and one-second windows showed single windows 4 ms above the median, enough to
    # swamp the min .. max spread of five.  Every window's figure is printed so that such a run shows.
    forms = {k: (lambda m=m: m.train_step_async(a, b)) for k, m in models.items()}
    seconds = max(args.seconds, 2.0)
    iters = {k: calibrate(fn, seconds) for k, fn in forms.items()}
    samples = {k: [] for k in forms}
    for rnd in range(args.repeats + 1):
        for k, fn in forms.items():
            ms = window(fn, iters[k])
            if rnd:
                samples[k].append(ms)
    r = {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}
    ok, gain, spread = gate(r, "fp32", "mixed")
    print(f"EnhancedCycleGAN(channels=16) train step, {pairs} pairs x {size}x{size}: blocks=1 fp32 / mixed attention, and blocks=0")
    print(f"  gain {gain:.3f} ms, combined spread {spread:.3f} ms")
    for k, (med, lo, hi) in r.items():
        print(f"    {k:8s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  {pairs / med * 1e3:8.1f} pairs/s   windows " +
              " ".join(f"{v:.2f}" for v in samples[k]))
    row = {"pairs": pairs, "size": size, "channels": 16}
    row.update({k: {"ms": v[0], "min_ms": v[1], "max_ms": v[2]} for k, v in r.items()})
    row.update(speedup=r["fp32"][0] / r["mixed"][0], gain_ms=gain, spread_ms=spread, faster_beyond_spread=ok)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--quick", action="store_true", help="one small attention shape and a 2-pair 64x64 step")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flash_f16_train.py needs a GPU")
    shapes = [(16, 1024, 2)] if args.quick else [(16, 4096, 16), (64, 4096, 16), (16, 1024, 32)]
    result = {"attention": [attention_case(D, L, N, args) for D, L, N in shapes],
              "step": step_case(*((2, 64) if args.quick else (8, 256)), args)}
    result["gates_pass"] = all(r["forward+backward"]["faster_beyond_spread"] for r in result["attention"]) and \
        result["step"]["faster_beyond_spread"]
    line = json.dumps(result)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        open(args.json, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
