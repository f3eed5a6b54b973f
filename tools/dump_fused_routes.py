"""Routing table of the fused MultiScaleBlock and LocalAttention passes: for every case below, under the default switches and under
each switch of SETTINGS, the workspace queries of the passes and -- with a GPU -- the ordered kernel symbols each pass launches
through mstg_hip.ops, as the per-launch profiler reports them (helper launches included).  A library that has the name queries
(mstg_msblock_kernel_name, mstg_window_attn_kernel_name) gets their answers recorded as "names" too.

usage: dump_fused_routes.py [--cpu] [-o FILE]     (--cpu: queries only, no launches; MSTG_LIB selects another build of the library)

Output (what tests/golden/fused_routes.json holds; tests/test_fused_routes.py and tests/test_gpu_ops.py compare against it):
    {"default": {case: row}, "<SWITCH>=<value>[,<SWITCH>=<value>]": {case: row, only where it differs from the default row}, ...}
    row = {"ws": [bytes per pass], "launches": [[symbols of the pass's call, in launch order] per pass]}
    passes: MultiScaleBlock fwd, dgrad, wgrad; attention fwd, bwd.  A width without a fused path has ws 0 and no launches.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multi-style-transfer-gan_amd")]

SETTINGS = ["default", "MSTG_MS_FWD4=0", "MSTG_MS_FWD4=1", "MSTG_MS_FWD4=2", "MSTG_MS_WGRAD_PACKED=0", "MSTG_MS_WGRAD_PF=0",
            "MSTG_MS_WGRAD_PACKED=0,MSTG_MS_WGRAD_PF=0", "MSTG_ATTN_REG=0", "MSTG_ATTN_BIG32=1", "MSTG_ATTN_BLK64=0", "MSTG_ATTN_BLK4=0"]
# (N, H, W, ch, bias_aligned): odd sizes, H < 16 (the other forward route), biases off the 16-byte grid, a width without fused path
MS_CASES = [(2, 21, 37, 16, 1), (1, 16, 16, 32, 1), (2, 9, 20, 64, 1), (1, 8, 8, 32, 1), (1, 16, 16, 16, 0), (1, 16, 16, 8, 1)]
CORE_CASES = [(1, 8, 8, C) for C in (16, 32, 48, 64, 128, 200)]
FUSED_CASES = [(N, H, W, C, norm) for (N, H, W) in ((1, 8, 8), (2, 16, 16)) for C in (16, 32, 64) for norm in (0, 1)] + [
    (1, 8, 8, 8, 0), (1, 8, 8, 8, 1)]


def cases():
    """[(name, family, shape)]"""
    return ([(f"ms N{N} {H}x{W} ch{ch}" + ("" if al else " bias off 16 B"), "ms", (N, H, W, ch, al)) for N, H, W, ch, al in MS_CASES] +
            [(f"attn-core N{N} {H}x{W} C{C}", "core", (N, H, W, C)) for N, H, W, C in CORE_CASES] +
            [(f"attn-fused{' norm' if nm else ''} N{N} {H}x{W} C{C}", "fused", (N, H, W, C, nm)) for N, H, W, C, nm in FUSED_CASES])


def apply_setting(setting, environ=os.environ):
    """Put the switches of `setting` (and no other MSTG_* switch) into `environ` and make the library read them."""
    from mstg_hip import _lib
    for k in [k for k in environ if k.startswith("MSTG_") and k != "MSTG_LIB"]:
        del environ[k]
    if setting != "default":
        environ.update(kv.split("=") for kv in setting.split(","))
    _lib.load().mstg_env_refresh()


def workspaces(family, shape):
    lib = __import__("mstg_hip._lib", fromlist=["load"]).load()
    if family == "ms":
        N, H, W, ch, _ = shape
        return [lib.mstg_msblock_fwd_workspace_bytes(ch), lib.mstg_msblock_dgrad_workspace_bytes(ch),
                lib.mstg_msblock_wgrad_workspace_bytes(N, H, W, ch)]
    if family == "core":
        return [0, 0]
    N, H, W, C, norm = shape
    return [0, (lib.mstg_window_attn_norm_bwd_workspace_bytes if norm else lib.mstg_window_attn_bwd_workspace_bytes)(N, H, W, C)]


def names(family, shape):
    """What the library's name queries answer for the passes of the case."""
    lib = __import__("mstg_hip._lib", fromlist=["load"]).load()
    if family == "ms":
        return [lib.mstg_msblock_kernel_name(ps, *shape).decode() for ps in (0, 1, 2)]
    return [lib.mstg_window_attn_kernel_name(int(family == "fused"), ps, shape[3], shape[4] if family == "fused" else 0).decode()
            for ps in (0, 1)]


def supported(family, shape):
    lib = __import__("mstg_hip._lib", fromlist=["load"]).load()
    return family == "core" or bool((lib.mstg_msblock_fused_supported if family == "ms" else lib.mstg_window_attn_fused_supported)(shape[3]))


def run_case(family, shape):
    """One forward and one backward of the case through mstg_hip.ops with the kernel timer on: [(the call's label, [launched symbols])]
    per pass.  Plain tensors, not Parameters: no pack is kept, so every call shows its helper launches."""
    import torch
    from mstg_hip import ops
    if not supported(family, shape):
        return []
    g = torch.Generator(device="cuda").manual_seed(5)

    def rnd(*s, off=0):  # off: floats between the tensor's first element and the allocation's 16-byte grid
        return torch.randn(s[0] + off, *s[1:], device="cuda", generator=g)[off:].requires_grad_()
    N, H, W, C = shape[:4]
    x = rnd(N, H, W, C)
    ops.KernelTimer.start()
    try:
        if family == "ms":
            wb = []
            for k, _, _ in ops.MSBranchesFn.GEOM:
                wb += [rnd(C // 4, C, k, k), rnd(C // 4, off=0 if shape[4] else 1)]
            y, res = ops.MSBranchesFn.apply(x, *wb)
            (y.sum() + res.sum()).backward()
            npass = 3
        elif family == "core":
            ops.WindowAttnCoreFn.apply(rnd(N, H, W, 3 * C)).sum().backward()
            npass = 2
        else:
            prm = [rnd(3 * C, C, 1, 1), rnd(3 * C), rnd(C, C, 1, 1), rnd(C)]
            if shape[4]:
                stats = torch.stack([torch.zeros(N, C, device="cuda"), torch.ones(N, C, device="cuda")], dim=2).contiguous()
                ops.NormLocalAttentionFn.apply(x, *prm, stats).sum().backward()
            else:
                ops.LocalAttentionFusedFn.apply(x, *prm).sum().backward()
            npass = 2
        torch.cuda.synchronize()
        ks = [nm for nm, _ in ops.KernelTimer.kernels()]
        return [(c[0], ks[c[1]:c[2]]) for c in ops.KernelTimer.calls[:npass]]
    finally:
        ops.KernelTimer.stop()


def rows(gpu):
    """{case: row} under the switches the library last read."""
    lib = __import__("mstg_hip._lib", fromlist=["load"]).load()
    out = {}
    for name, family, shape in cases():
        out[name] = {"ws": workspaces(family, shape)}
        if hasattr(lib, "mstg_msblock_kernel_name"):
            out[name]["names"] = names(family, shape)
        if gpu:
            out[name]["launches"] = [syms for _, syms in run_case(family, shape)]
    return out


def dump(gpu):
    table = {}
    for setting in SETTINGS:
        apply_setting(setting)
        got = rows(gpu)
        table[setting] = got if setting == "default" else {c: row for c, row in got.items() if row != table["default"][c]}
    apply_setting("default")
    return table


if __name__ == "__main__":
    text = json.dumps(dump("--cpu" not in sys.argv), indent=1)
    if "-o" in sys.argv:
        open(sys.argv[sys.argv.index("-o") + 1], "w").write(text + "\n")
    else:
        print(text)
