"""Backward of the MultiScaleBlock branches (csrc/msblock.hip) through the C ABI: mstg_msblock_wgrad and mstg_msblock_dgrad against
fp64 autograd of the four branch convolutions, at the bars tests/test_gpu_ops.py and tests/test_gpu_direct_grads.py hold the
multi-scale kernels to (2e-5 for dx, 1e-4 for the parameter gradients).

The weight-gradient kernels keep the next tile's windows in flight in registers while a tile is multiplied, deal the units to
the waves by a per-workgroup rotation and sum the bias on the waves with the fewest units; the synchronous kernels they replace
are still there behind MSTG_MS_WGRAD_PF=0 and write the same partial slabs, so every case also asks for bitwise equal gradients
from the two (with and without MSTG_MS_WGRAD_PACKED=0, which selects the unit kernel at 16 and 32 channels).  Outputs and
workspaces sit between red zones (guard_helpers.memory_contract): the workspace is handed out at exactly the size the query
reports, NaN-filled, so a slab that no workgroup wrote, or a store outside a slab, shows.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from guard_helpers import memory_contract

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOM = ((1, 0, 1), (3, 1, 1), (3, 2, 2), (3, 4, 4))  # (k, pad, dil) of the four branches
SMALL = [(1, 16, 16), (3, 24, 40), (2, 8, 16)]
# every workgroup walks at least two tiles and the last round is ragged (test_walk_case_covers_the_grid checks it against the plan)
WALK = {16: (50, 60, 56), 32: (50, 60, 56), 64: (13, 60, 56)}
SWITCHES = [(), (("MSTG_MS_WGRAD_PF", "0"),), (("MSTG_MS_WGRAD_PACKED", "0"),), (("MSTG_MS_WGRAD_PACKED", "0"), ("MSTG_MS_WGRAD_PF", "0"))]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()  # raises if the HIP library is missing -- there is no fallback to test instead


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def report(name, err, tol):
    print(f"  [parity] {name:60s} rel-L2 {err:.2e} (tol {tol:.0e})")
    assert err <= tol, f"{name}: {err:.3e} > {tol:.0e}"


@functools.lru_cache(maxsize=None)
def case(ch, N, H, W):
    """Inputs (CPU, fp32) and the fp64 autograd reference of one case: computed once, shared, never written."""
    x, dy, dres = rnd((N, H, W, ch), 5), rnd((N, H, W, ch), 20), rnd((N, H, W, ch), 21)
    wb = []
    for j, (k, _, _) in enumerate(GEOM):
        wb += [rnd((ch // 4, ch, k, k), 6 + j, 0.2), rnd((ch // 4,), 10 + j, 0.2)]
    leaves = [t.double().requires_grad_(True) for t in [x] + wb]
    xc = leaves[0].permute(0, 3, 1, 2)
    outs = [F.conv2d(xc, leaves[1 + 2 * j], leaves[2 + 2 * j], padding=pad, dilation=dil) for j, (_, pad, dil) in enumerate(GEOM)]
    y = torch.cat(outs, 1).permute(0, 2, 3, 1)
    g = torch.autograd.grad((y * dy.double()).sum(), leaves)
    return {"x": x, "dy": dy, "dres": dres, "wb": wb, "dx": g[0], "dwb": list(g[1:])}


def wgrad(ch, N, H, W, c, preset=None):
    """The eight parameter gradients from mstg_msblock_wgrad: fresh outputs, or (preset: eight CPU tensors) added into preset slots."""
    from mstg_hip import _lib, ops
    lib = _lib.load()
    with memory_contract() as mc:
        x, dy = c["x"].to(DEV), c["dy"].to(DEV)
        outs = [torch.empty(t.shape, dtype=torch.float32, device=DEV) for t in c["wb"]]
        if preset is not None:
            for o, s in zip(outs, preset):
                o.copy_(s)
        ws = ops._ws(lib.mstg_msblock_wgrad_workspace_bytes(N, H, W, ch), x.device)
        _lib.check(lib.mstg_msblock_wgrad(x.data_ptr(), dy.data_ptr(), *[o.data_ptr() for o in outs], int(preset is not None), N, H, W, ch,
                                          ws.data_ptr(), ws.numel() * 4, ops._stream()), "mstg_msblock_wgrad")
        res = [o.clone() for o in outs]
        assert mc.outputs == 8 and mc.workspaces == 1 and mc.uploads == 2
    return res


def dgrad(ch, N, H, W, c, with_res):
    from mstg_hip import _lib, ops
    lib = _lib.load()
    with memory_contract() as mc:
        dy = c["dy"].to(DEV)
        dres = c["dres"].to(DEV) if with_res else None
        w = [t.to(DEV) for t in c["wb"][0::2]]
        dx = torch.empty((N, H, W, ch), dtype=torch.float32, device=DEV)
        ws = ops._ws(lib.mstg_msblock_dgrad_workspace_bytes(ch), dy.device)
        _lib.check(lib.mstg_msblock_dgrad(dy.data_ptr(), *[t.data_ptr() for t in w], None if dres is None else dres.data_ptr(), dx.data_ptr(),
                                          N, H, W, ch, ws.data_ptr(), ws.numel() * 4, ops._stream()), "mstg_msblock_dgrad")
        res = dx.clone()
        mc.assert_written(dx)
        assert mc.outputs == 1 and mc.workspaces == 1
    return res


def check_wgrad(name, ch, N, H, W, setenv_refresh):
    from mstg_hip import ops
    c = case(ch, N, H, W)
    names = "w1 b1 w2 b2 w3 b3 w4 b4".split()
    got = {}
    for sw in SWITCHES:
        for k, v in sw:
            setenv_refresh.set(k, v)
        tag = " ".join(f"{k}={v}" for k, v in sw) or "default"
        ops.KernelTimer.start()
        try:
            g = wgrad(ch, N, H, W, c)
            torch.cuda.synchronize()
            kernels = [nm for nm, _ in ops.KernelTimer.kernels()]
        finally:
            ops.KernelTimer.stop()
        packed = ch <= 32 and ("MSTG_MS_WGRAD_PACKED", "0") not in sw
        sym = ("wgrad_msp" if packed else "wgrad_ms") + ("_sync" if ("MSTG_MS_WGRAD_PF", "0") in sw else "") + f"_kernel<{ch}>"
        assert any(sym in k for k in kernels), f"{name} [{tag}]: {sym} did not run: {kernels}"
        for nm, a, b in zip(names, g, c["dwb"]):
            report(f"{name} [{tag}] d{nm}", rel_l2(a, b), 1e-4)
        again = wgrad(ch, N, H, W, c)
        assert all(torch.equal(a, b) for a, b in zip(g, again)), f"{name} [{tag}]: two runs differ"
        got[sw] = g
        for k, _ in sw:
            setenv_refresh.unset(k)
    for new, old in ((SWITCHES[0], SWITCHES[1]), (SWITCHES[2], SWITCHES[3])):
        for nm, a, b in zip(names, got[new], got[old]):
            assert torch.equal(a, b), f"{name}: d{nm} differs between {new or 'default'} and {old}: {int((a != b).sum())} of {a.numel()} elements"
    # accumulate = 1: every element is slot + r with the r of the fresh run
    seeds = [rnd(t.shape, 300 + j) * float(t.abs().max()) for j, t in enumerate(got[()])]
    acc = wgrad(ch, N, H, W, c, preset=seeds)
    for nm, a, s, g in zip(names, acc, seeds, got[()]):
        assert torch.equal(a, s.to(DEV) + g), f"{name}: accumulated d{nm} is not slot + gradient"
    assert all(torch.equal(a, b) for a, b in zip(acc, wgrad(ch, N, H, W, c, preset=seeds))), f"{name}: two accumulating runs differ"


@pytest.mark.parametrize("N,H,W", SMALL)
@pytest.mark.parametrize("ch", [16, 32, 64])
def test_ms_wgrad_small(ch, N, H, W, setenv_refresh):
    check_wgrad(f"ms wgrad ch{ch} N{N} {H}x{W}", ch, N, H, W, setenv_refresh)


def plan(ch, N, H, W):
    """(workgroups of the default launch = partial slabs, tiles) as msblock.hip sizes them."""
    ntiles = N * ((W + 15) // 16) * ((H + 7) // 8)
    ng = ch // 16
    S = max(1, min(768 // ng, ntiles))
    return (min(S * ng, ntiles) if ch <= 32 else S), ntiles, S


@pytest.mark.parametrize("ch", [16, 32, 64])
def test_walk_case_covers_the_grid(ch):
    """The walk cases are sized against the grid the launch uses; the workspace query is that grid times the slab size."""
    from mstg_hip import _lib
    N, H, W = WALK[ch]
    grid, ntiles, S = plan(ch, N, H, W)
    assert ntiles >= 2 * grid and ntiles % grid != 0, (grid, ntiles)
    ng = ch // 16
    unit_slab = ng * (ng + 24) * 256 + ch
    need = S * unit_slab
    if ch <= 32:
        need = max(need, grid * (ng * (ng + 3 * (8 // (16 // (ch // 4)))) * 256 + ch))
    assert _lib.load().mstg_msblock_wgrad_workspace_bytes(N, H, W, ch) == 4 * need


@pytest.mark.parametrize("ch", [16, 32, 64])
def test_ms_wgrad_walks_tiles(ch, setenv_refresh):
    N, H, W = WALK[ch]
    check_wgrad(f"ms wgrad walk ch{ch} N{N} {H}x{W}", ch, N, H, W, setenv_refresh)


@pytest.mark.parametrize("N,H,W", SMALL)
@pytest.mark.parametrize("ch", [16, 32, 64])
def test_ms_dgrad(ch, N, H, W):
    c = case(ch, N, H, W)
    name = f"ms dgrad ch{ch} N{N} {H}x{W}"
    plain = dgrad(ch, N, H, W, c, False)
    report(f"{name} dx", rel_l2(plain, c["dx"]), 2e-5)
    res = dgrad(ch, N, H, W, c, True)
    report(f"{name} dx + dres", rel_l2(res, c["dx"] + c["dres"].double()), 2e-5)
    assert torch.equal(res, plain + c["dres"].to(DEV)), f"{name}: the residual gradient is not added to the finished dx"
    assert torch.equal(plain, dgrad(ch, N, H, W, c, False)) and torch.equal(res, dgrad(ch, N, H, W, c, True)), f"{name}: two runs differ"
