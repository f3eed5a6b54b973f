"""Benchmark of the hot path on N MI355X, one process per GPU, image batches sharded data-parallel with one RCCL all-reduce
per optimizer.

    python bench.py --gpus N --steps K --warmup W [--config {1..5}] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Started WITHOUT a launcher and with --gpus N > 1, this script itself starts the N ranks (a torch.distributed.run child,
before anything in this process has touched the GPU) and exits with the child's code; a rank whose world size or backend is
not what --gpus asked for exits non-zero -- a 1-GPU number is never reported under an N-GPU label.

--config selects one of the five BASELINE.json workloads (default 3 = the one the headline metric is quoted on):
  1  EnhancedGenerator forward, one 256x256 image (direct_transform.py:44-79), fp32
  2  EnhancedGenerator forward + backward (loss mean|y|), batch 16 at 256x256, fp32
  3  the reference's CycleGAN train step (enhanced_train.py:59-131): 6 generator + 10 discriminator forwards, backward through
     all of them, two Adam steps; 32 image pairs per GPU at 256x256, fp32   [--style-loss adds the build-defined VGG/Gram loss]
  4  the same step at 512x512, 32 pairs per GPU, with the build-defined multi-style loss (3 weighted references), data parallel
  5  inference-only EnhancedGenerator forward, batch 64 at 1024x1024, fp16 storage + fp16 MFMA with fp32 accumulation
One "step" = one pass of the configured workload on the per-rank batch (synthetic uniform [-1,1) data, random init of the
reference architecture at channels=16: what enhanced_train.py:18-21 trains).  Weak scaling: the per-GPU batch is fixed.  Rank 0
prints ONE JSON line.  An "image" is one input image pushed through the step; a train step consumes 2 * batch images (one per
domain), so value = 2 * batch * N / step_time there, and batch * N / step_time for the generator-only configs.

A plain run sets up, warms up, times the K steps and prints the line; `roofline` and `cpu_baseline` are null there.

--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step computed, as the caller of that path receives
it, to DIR/<name>.npy (float32): train configs `losses` (the step's loss vector), `g_params` / `d_params` (the two optimizers'
flat parameter buffers after the step's Adam updates); config 2 `loss`, `grads` (the flat gradient buffer); forward configs
`mean_abs` and `output` (the generator's output).  An array of more than 4M elements is replaced by `<name>_sample`: 4M elements
at indices drawn with a fixed seed (sorted, with replacement), so a dump stays well below 64 MB.  Inputs and weights are seeded,
so two builds run with the same arguments can be compared array by array.

--full adds what takes runs of its own beside the timed steps (each can still be switched off with --no-roofline /
--no-cpu-baseline; --kernel-table needs it):
  roofline     : the kernel symbol with the largest share of GPU time among ALL launches of an instrumented step that follows the
                 timed region (same shapes, one stream).  The library itself brackets every kernel it launches with HIP events on
                 the launch stream (mstg_prof_*, csrc/runtime.hip), so a call that launches two kernels contributes two rows;
                 achieved = sum of the ALGORITHMIC FLOPs (or bytes) of that symbol's launches (2 FLOP per multiply-add,
                 no recompute, no padding; tensors read once, written once) / sum of their durations, against the MI355X peak.
                 `top` = the five largest symbols the same way, `largest_call` = the largest C-ABI call with all its launches;
  cpu_baseline : the oracle's restatement of the same workload (oracle/restatement.py, validated against the reference in the
                 build container) timed on this box's host cores: thread counts {1, 8, 32, all} are swept on a small probe, then
                 one warm-up pass and 3-5 timed passes of the workload at the best count; `value` = their median.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "multi-style-transfer-gan_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense
PEAK_F16_MFMA_TFLOPS = 2500.0  # same guide: BF16/FP16 MFMA, dense
PEAK_HBM_GBS = 8000.0          # HBM3E spec

CONFIGS = {
    1: dict(kind="fwd", batch=1, size=256, dtype="f32", style=False),
    2: dict(kind="fwdbwd", batch=16, size=256, dtype="f32", style=False),
    3: dict(kind="train", batch=32, size=256, dtype="f32", style=False),
    4: dict(kind="train", batch=32, size=512, dtype="f32", style=True),
    5: dict(kind="fwd", batch=64, size=1024, dtype="f16", style=False),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", type=int, default=3, choices=sorted(CONFIGS), help="BASELINE.json workload (see module docstring)")
    ap.add_argument("--batch", type=int, default=None, help="images (generator configs) / image pairs (train step) per GPU per step")
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--dtype", choices=("f32", "f16"), default=None, help="forward-only configs: storage/MFMA type")
    ap.add_argument("--style-loss", action="store_true",
                    help="add the build-defined VGG/Gram multi-style loss (3 weighted references) to the train step")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float32, < 64 MB in all)")
    ap.add_argument("--full", action="store_true",
                    help="also measure the instrumented roofline step and the CPU baseline (off in a plain run)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the instrumented roofline step")
    ap.add_argument("--kernel-table", action="store_true", help="with --full: print the per-kernel table of the instrumented step to stderr")
    args = ap.parse_args()
    if args.kernel_table and not (args.full and not args.no_roofline):
        ap.error("--kernel-table prints the instrumented step: it needs --full (and no --no-roofline)")
    cfg = CONFIGS[args.config]
    args.kind = cfg["kind"]
    args.batch = cfg["batch"] if args.batch is None else args.batch
    args.size = cfg["size"] if args.size is None else args.size
    args.dtype = cfg["dtype"] if args.dtype is None else args.dtype
    args.style_loss = bool(args.style_loss or cfg["style"])
    if args.dtype == "f16" and args.kind != "fwd":
        ap.error("fp16 is the inference (forward-only) path; training runs in fp32")
    return args


# ------------------------------------------------------------------------------------------------------------------------
# launcher: python bench.py --gpus N  (no torchrun)  ->  N ranks as a child torch.distributed.run
# ------------------------------------------------------------------------------------------------------------------------
def launch_ranks(n: int) -> int:
    """Start `n` ranks of this script.  Nothing here initialises the GPU (device_count() does not, on this image), so the child
    is started from a clean process; the parent only waits and forwards the exit code."""
    rehearse = os.environ.get("MSTG_BENCH_REHEARSE", "0") == "1"
    have = torch.cuda.device_count()
    if have < n and not rehearse:
        print(f"[bench] --gpus {n} but this node shows {have} GPU(s): refusing to report a {have}-GPU number as {n}-GPU "
              f"(MSTG_BENCH_REHEARSE=1 rehearses the N-rank flow on one GPU over gloo)", file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


# ------------------------------------------------------------------------------------------------------------------------
# CPU baseline (the oracle -- the checker, timed here only as the reported baseline)
# ------------------------------------------------------------------------------------------------------------------------
def usable_cpus() -> int:
    """Cores this process may really use: os.cpu_count() reports the host's (256 on the GPU box) while the job's cgroup grants a
    share (16 per GPU there); a thread pool sized to the former oversubscribes 16x and takes minutes per step."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]) + 0.5)))
            else:
                quota = int(txt[0])
                period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if quota > 0:
                    n = min(n, max(1, int(quota / period + 0.5)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def cpu_baseline(args):
    """The oracle's restatement of the configured workload on the host cores, bounded to roughly a minute and talking to stderr
    while it runs.  Thread counts {1, 8, 32, all} and batch {1, 4} are swept on a CHEAP sample (half the workload's edge, at most
    128x128: a quarter of the per-image work or less), then the workload's own size (capped at 512x512 for the forward-only
    configs) is timed at batch 1 with the best thread count: that is `value`; the sweep, with the sizes it was taken at, and the
    1-thread figure are reported beside it."""
    from oracle import restatement as R
    C, kind = args.channels, args.kind
    size = args.size if kind == "train" else min(args.size, 512)
    probe = max(32, min(128, size // 2) // 16 * 16)
    torch.manual_seed(0)
    ncpu = min(usable_cpus(), 64)  # beyond 64 threads this workload only loses (measured: 32 threads already slower than 8)

    def workload(n, edge):
        if kind == "train":
            sds = [R.make_state_dict(R.generator_spec(C), 11), R.make_state_dict(R.generator_spec(C), 12),
                   R.make_state_dict(R.discriminator_spec(C), 13), R.make_state_dict(R.discriminator_spec(C), 14)]
            model = R.CycleGANOracle(*sds)
            a, b = R.make_input((n, 3, edge, edge), 21), R.make_input((n, 3, edge, edge), 22)
            return (lambda: model.train_step(a, b)), 2 * n
        sd = R.make_state_dict(R.generator_spec(C), 11)
        x = R.make_input((n, 3, edge, edge), 21)
        if kind == "fwd":
            def run():
                with torch.no_grad():
                    R.generator_forward(sd, x)
            return run, n
        params = [v.requires_grad_(True) for k, v in sd.items() if not k.startswith("style_encoder")]

        def run():
            torch.autograd.grad(R.generator_forward(sd, x).abs().mean(), params)
        return run, n

    def timed(fn, warm=True):
        if warm:
            fn()
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    sweep = []
    for th in sorted({1, min(8, ncpu), min(32, ncpu), ncpu}):
        torch.set_num_threads(th)
        fn, imgs = workload(1, probe)
        dt = timed(fn, warm=th != 1)  # 1 thread: a single cold pass is the sample
        sweep.append({"threads": th, "batch": 1, "size": probe, "images_per_sec": round(imgs / dt, 4)})
        print(f"[bench] cpu baseline probe {probe}x{probe}: {th} threads {imgs / dt:.3f} images/s", file=sys.stderr, flush=True)
        if len(sweep) >= 2 and sweep[-1]["images_per_sec"] < sweep[-2]["images_per_sec"]:
            break  # more threads already lose (oversubscribed share / memory bound): larger counts only take longer
    best = max(sweep, key=lambda r: r["images_per_sec"])
    torch.set_num_threads(best["threads"])
    fn, imgs = workload(4, probe)
    dt = timed(fn, warm=False)
    sweep.append({"threads": best["threads"], "batch": 4, "size": probe, "images_per_sec": round(imgs / dt, 4)})
    print(f"[bench] cpu baseline probe {probe}x{probe}: batch 4, {best['threads']} threads {imgs / dt:.3f} images/s", file=sys.stderr, flush=True)
    fn, imgs = workload(1, size)
    fn()  # one warm-up pass, then >= 3 timed passes bounded to ~20 s; `value` is their median
    passes, t_all = [], time.perf_counter()
    while len(passes) < 3 or (len(passes) < 5 and time.perf_counter() - t_all < 10.0):
        t0 = time.perf_counter()
        fn()
        passes.append(time.perf_counter() - t0)
    dt = sorted(passes)[len(passes) // 2]
    value = imgs / dt
    print(f"[bench] cpu baseline {size}x{size}: {best['threads']} threads {value:.3f} images/s (median of {len(passes)} passes)",
          file=sys.stderr, flush=True)
    one = next(r for r in sweep if r["threads"] == 1)
    torch.set_num_threads(ncpu)
    what = {"train": "oracle train step", "fwd": "oracle generator forward", "fwdbwd": "oracle generator forward+backward"}[kind]
    return {"value": round(value, 4), "unit": "images/sec", "cores": best["threads"], "kind": "port",
            "one_thread_probe_value": one["images_per_sec"], "host_cpus": os.cpu_count(), "usable_cpus": usable_cpus(), "sweep": sweep,
            "passes_sec": [round(t, 4) for t in passes],
            "sample": f"{what}, channels={C}, fp32: `value` = median of {len(passes)} timed passes after one warm-up pass at {size}x{size}, "
                      f"batch 1, {best['threads']} threads (the best of the sweep); sweep points are single passes at {probe}x{probe}"}


def pmc_traffic(sym: str, args):
    """HBM bytes per launch of `sym` from the committed rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE in separate runs, read side
    doubled as the MI355X guide prescribes for gfx950; tools/gpu_refresh.sh + tools/pmc_traffic.py).  PMC counters cannot be read
    from inside this process, so the figure is the one measured on the default workload and is reported only when this run IS
    the default workload."""
    default = (args.config == 3 and args.batch == 32 and args.size == 256 and args.channels == 16 and not args.style_loss)
    if not default:
        return None, None
    for tag in ("r03", "r02", "r01"):
        path = os.path.join(ROOT, "profiles", f"{tag}_pmc_traffic.json")
        if os.path.exists(path):
            t = json.load(open(path)).get(sym)
            if t:
                return t["hbm_bytes"], f"profiles/{tag}_pmc_traffic.json"
    return None, None


def metric_label(args) -> str:
    sz = f"{args.size}x{args.size}"
    if args.kind == "train":
        return f"train-step images/sec (fwd+bwd+loss), {sz} batch{args.batch}"
    if args.kind == "fwdbwd":
        return f"generator fwd+bwd images/sec, {sz} batch{args.batch}"
    return f"generator forward images/sec, {sz} batch{args.batch}" + (" fp16" if args.dtype == "f16" else "")


def workload_label(args) -> str:
    sz = f"{args.size}x{args.size}"
    if args.kind == "train":
        return (f"config {args.config}: reference CycleGAN train_step (2x EnhancedGenerator + 2x EnhancedDiscriminator, channels={args.channels}, "
                f"num_transformer_blocks=0), {args.batch} image pairs/GPU at {sz}, fwd+bwd+loss+Adam"
                + (" + build-defined VGG16/Gram multi-style loss (3 weighted refs)" if args.style_loss else ""))
    if args.kind == "fwdbwd":
        return (f"config {args.config}: EnhancedGenerator(channels={args.channels}, num_transformer_blocks=0) forward+backward, loss mean|y|, "
                f"{args.batch} images/GPU at {sz}")
    return (f"config {args.config}: EnhancedGenerator(channels={args.channels}, num_transformer_blocks=0) inference forward (no_grad, eval), "
            f"{args.batch} images/GPU at {sz}, " + ("fp16 storage + fp16 MFMA, fp32 accumulate" if args.dtype == "f16" else "fp32"))


DUMP_MAX_ELEMS = 1 << 22  # 16 MB of float32 per array


def dump_outputs(out, path):
    """DIR/<name>.npy in float32 for every array of the last timed step; one of more than DUMP_MAX_ELEMS elements becomes
    DIR/<name>_sample.npy, its elements at DUMP_MAX_ELEMS sorted indices drawn (with replacement) from a fixed seed."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, t in out.items():
        t = t.detach()
        if t.numel() > DUMP_MAX_ELEMS:
            idx = torch.randint(t.numel(), (DUMP_MAX_ELEMS,), generator=torch.Generator().manual_seed(0)).sort().values
            t, name = t.reshape(-1)[idx.to(t.device)], name + "_sample"
        np.save(os.path.join(path, name + ".npy"), t.float().cpu().numpy())


def main():
    args = parse()
    rehearse = os.environ.get("MSTG_BENCH_REHEARSE", "0") == "1"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    from mstg_hip import dp, ops
    # MSTG_BENCH_REHEARSE=1: rehearsal of the N > 1 flow on a one-GPU box -- gloo instead of RCCL, every rank on cuda:0
    local = dp.init_from_env("gloo" if rehearse else "nccl")
    if rehearse:
        local = 0
    world = dp.world_size()
    if world != args.gpus:
        print(f"[bench] world size {world} != --gpus {args.gpus}: refusing to run", file=sys.stderr)
        sys.exit(2)
    if world > 1 and not rehearse and dist.get_backend() != "nccl":
        print(f"[bench] backend {dist.get_backend()} is not nccl (RCCL): refusing to run", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    torch.manual_seed(42)  # reference seeds with set_seed(42) (pretrain.py:13-17); every rank builds the same weights
    gen = torch.Generator().manual_seed(1234 + dp.rank())
    shape = (args.batch, 3, args.size, args.size)

    if args.kind == "train":
        import enhanced_train
        model = enhanced_train.EnhancedCycleGAN(channels=args.channels, num_transformer_blocks=0, device=dev)
        model.sync_replicas()
        if args.style_loss:
            sgen = [torch.Generator().manual_seed(2001 + k) for k in range(3)]
            refs = [(torch.rand((4, 3, args.size, args.size), generator=g_) * 2 - 1) for g_ in sgen]
            model.attach_style_loss(refs, (0.5, 0.3, 0.2), lambda_style=1.0)
        real_A = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
        real_B = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
        images_per_step = 2 * args.batch

        def step():  # (values checked for finiteness, what the caller of the path receives)
            losses = model.train_step_async(real_A, real_B)
            return losses, {"losses": losses, "g_params": model.g_optimizer.flat, "d_params": model.d_optimizer.flat}
    else:
        import enhanced_generator
        from mstg_hip.optim import FlatAdam
        net = enhanced_generator.EnhancedGenerator(channels=args.channels, num_transformer_blocks=0).to(dev)
        x = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
        images_per_step = args.batch
        if args.kind == "fwd":
            net.eval()
            if args.dtype == "f16":
                net.half_inference()

            def step():
                with torch.no_grad():
                    y = net(x)
                    m = y.float().abs().mean().reshape(1)
                    return m, {"mean_abs": m, "output": y}
        else:
            opt = FlatAdam(net.parameters(), lr=5e-5, betas=(0.5, 0.999))  # flat gradient buffer = what DP all-reduces
            for b_ in (opt.flat,):
                dp.broadcast_(b_)

            def step():
                opt.zero_grad()
                with ops.direct_param_grads():
                    loss = net(x).abs().mean()
                    loss.backward()
                dp.allreduce_mean_(opt.grad)
                loss = loss.detach().reshape(1)
                return loss, {"loss": loss, "grads": opt.grad}

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        losses, outputs = step()  # held across the next step as in the timed loop, so its memory pattern is warmed up too
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses, outputs = step()
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    finite = bool(torch.isfinite(losses).all())
    ms = dt / args.steps * 1e3
    value = images_per_step * world / (dt / args.steps)

    roofline = None
    if args.dump_outputs and dp.rank() == 0:
        dump_outputs(outputs, args.dump_outputs)  # before the instrumented step of --full moves parameters on
    outputs = None

    roofline_on = args.full and not args.no_roofline
    if roofline_on:
        # EVERY rank runs the instrumented step (it contains the two gradient all-reduces); only rank 0 reports
        ops.KernelTimer.start()
        step()
        torch.cuda.synchronize()
        ops.KernelTimer.stop()
    if roofline_on and dp.rank() == 0:
        table = ops.KernelTimer.summary()              # per KERNEL symbol (what rocprofv3 --kernel-trace --stats ranks)
        calls = ops.KernelTimer.summary(by_call=True)  # per C-ABI call (an op; may launch several kernels)
        total_ms = sum(r["ms"] for r in table.values())
        peak_mfma = PEAK_F16_MFMA_TFLOPS if args.dtype == "f16" else PEAK_F32_MFMA_TFLOPS

        def against_roofs(r):
            """(bound, achieved, unit, peak, frac) of algorithmic work r over its measured time, on the roof that bounds it."""
            sec = r["ms"] / 1e3
            t_mfma, t_hbm = r["flops"] / (peak_mfma * 1e12), r["bytes"] / (PEAK_HBM_GBS * 1e9)
            if t_mfma >= t_hbm and r["flops"] > 0:
                ach = r["flops"] / sec / 1e12
                return "mfma", round(ach, 3), "TFLOP/s", peak_mfma, round(ach / peak_mfma, 4)
            ach = r["bytes"] / sec / 1e9
            return "hbm", round(ach, 1), "GB/s", PEAK_HBM_GBS, round(ach / PEAK_HBM_GBS, 4)

        if args.kernel_table:
            for sym, r in sorted(ops.KernelTimer.summary(detail=True).items(), key=lambda kv: -kv[1]["ms"])[:200]:
                print(f"[kernels] {sym:72s} launches {r['launches']:5d}  {r['ms']:9.3f} ms  {100 * r['ms'] / total_ms:5.1f}%  "
                      f"{r['flops'] / r['ms'] / 1e9 if r['ms'] else 0:8.2f} TFLOP/s  {r['bytes'] / r['ms'] / 1e6 if r['ms'] else 0:9.1f} GB/s",
                      file=sys.stderr)
        # the dominant kernel = the symbol with the largest share of GPU time among ALL launches of the step, whichever call made
        # them (the library times each launch itself, so a call that launches two kernels contributes two rows)
        sym, r = max(table.items(), key=lambda kv: kv[1]["ms"])
        bound, ach, unit, peak, frac = against_roofs(r)
        roofline = {"bound": bound, "achieved": ach, "peak": peak, "unit": unit, "frac": frac, "traffic": None}
        roofline["algorithmic_bytes_per_launch"] = round(r["bytes"] / r["launches"])
        roofline["algorithmic_flop_per_launch"] = round(r["flops"] / r["launches"])
        roofline["traffic"], roofline["traffic_source"] = pmc_traffic(sym, args)
        # per-launch durations are taken with the step on ONE stream (EnhancedCycleGAN drops its side streams while
        # ops.KernelTimer is enabled): on two streams launches overlap and a launch's event-to-event time includes its neighbour
        roofline["measured"] = "HIP events around every kernel launch (mstg_prof_*), instrumented step on one stream"
        roofline.update({"kernel": sym, "launches_per_step": r["launches"], "avg_launch_us": round(1e3 * r["ms"] / r["launches"], 2),
                         "share_of_gpu_time": round(r["ms"] / total_ms, 3), "instrumented_step_gpu_ms": round(total_ms, 2),
                         "launches_in_step": sum(v["launches"] for v in table.values())})
        # the five largest symbols, same arithmetic (so the reader sees what stands behind the dominant one)
        roofline["top"] = []
        for k, v in sorted(table.items(), key=lambda kv: -kv[1]["ms"])[:5]:
            b_, a_, u_, _, f_ = against_roofs(v)
            roofline["top"].append({"kernel": k, "launches": v["launches"], "ms": round(v["ms"], 3), "bound": b_, "achieved": a_, "unit": u_, "frac": f_})
        # the largest OP (C-ABI call incl. its helper launches): algorithmic work of the op / time of all its kernels
        lsym, lr = max(calls.items(), key=lambda kv: kv[1]["ms"])
        b_, a_, u_, _, f_ = against_roofs(lr)
        roofline["largest_call"] = {"name": lsym, "kernels": sorted(lr.get("kernels", ())), "calls_per_step": lr["launches"],
                                    "ms_per_step": round(lr["ms"], 3), "share_of_gpu_time": round(lr["ms"] / total_ms, 3),
                                    "bound": b_, "achieved": a_, "unit": u_, "frac": f_}
        # whole-step view against both roofs (algorithmic work of every timed launch / wall time of the timed region)
        tot_fl, tot_by = sum(v["flops"] for v in table.values()), sum(v["bytes"] for v in table.values())
        roofline["step"] = {"algorithmic_tflop": round(tot_fl / 1e12, 4), "algorithmic_gb": round(tot_by / 1e9, 3),
                            "tflops_over_wall": round(tot_fl / 1e12 / (ms / 1e3), 2), "gbs_over_wall": round(tot_by / 1e9 / (ms / 1e3), 1)}

    cpu = None
    if dp.rank() == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline(args)

    if dp.rank() == 0:
        line = {"metric": metric_label(args), "value": round(value, 2), "unit": "images/sec",
                "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
                "config": {"workload": workload_label(args), "baseline_config": args.config,
                           "per_gpu_batch": args.batch, "images_per_step_per_gpu": images_per_step, "size": args.size,
                           "channels": args.channels, "parallelism": f"dp{world}",
                           "collective": (dist.get_backend() if world > 1 else "none"), "losses_finite": finite},
                "roofline": roofline, "cpu_baseline": cpu}
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if not finite:
        print("[bench] non-finite value in the step's outputs", file=sys.stderr)
        sys.exit(3)


if __name__ == "__main__":
    main()
