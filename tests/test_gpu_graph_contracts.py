"""Contracts of the fp32 training path that live in Python-side state (mstg_hip/ops.py), on graphs other than the one the shipped
models build.

A. The backward-sums tag.  ConvFn.backward hangs the reductions of the InstanceNorm + ReLU backward on its input gradient
   (``_mstg_bsums``); the norm's backward may use them only while that gradient is still the convolution's alone.  With a second
   consumer of the norm's output autograd adds the other share into the same tensor in place and the attribute stays on it.
   Graphs with two consumers, in both arrival orders, against torch fp64 and against the statistics-pass path (MSTG_NORM_BSUMS=0).
B. The filter-pack cache (``_cached_ws`` / ``_pack_stamp``).  For every cached kind: a hit launches no pack kernel and is
   bit-identical to the uncached run (also the THIRD time: a kernel that scribbles over its own pack shows there), and every kind of
   writer to the weights makes the next launch re-pack.  Hit / miss is read from the kernel list (KernelTimer.kernels()).
C. One layer applied twice in one graph (the generators run each layer at 2N and at N images per step), gradients returned to autograd
   and accumulated in place under ops.direct_param_grads().

References are torch fp64 on the CPU.  Bars: those the suite already holds the same quantities to against torch -- 2e-5 for
convolution outputs and input gradients, 1e-4 for weight and bias gradients (test_gpu_ops.py::test_conv_fwd_bwd), 5e-5 for the input
gradient of InstanceNorm + ReLU and 2e-6 between its two backward paths (test_gpu_normfuse.py).  A stale pack or stale sums are
wrong by O(1): every weight write below is w <- -2 w + noise.
"""
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()  # raises if the HIP library is missing -- there is no fallback to test instead


def _ops():
    from mstg_hip import ops
    return ops


def report(name, err, tol):
    print(f"  [parity] {name:72s} rel-L2 {err:.2e} (tol {tol:.0e})")
    assert err <= tol, f"{name}: {err:.3e} > {tol:.0e}"


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ----------------------------------------------------------------------------------------------------------
# the operations, NHWC, once on the HIP kernels and once in torch (called in fp64 on the CPU)
# ----------------------------------------------------------------------------------------------------------
def t_conv(x, w, b, k, s, p, tr=False, dil=1):
    xc = x.permute(0, 3, 1, 2)
    y = F.conv_transpose2d(xc, w, b, stride=s, padding=p) if tr else F.conv2d(xc, w, b, stride=s, padding=p, dilation=dil)
    return y.permute(0, 2, 3, 1)


def t_norm(x):
    return F.relu(F.instance_norm(x.permute(0, 3, 1, 2), eps=1e-5)).permute(0, 2, 3, 1)


def t_branches(x, wb):
    geom = _ops().MSBranchesFn.GEOM
    return torch.cat([t_conv(x, wb[2 * j], wb[2 * j + 1], k, 1, pad, dil=dil) for j, (k, pad, dil) in enumerate(geom)], dim=-1)


class Hip:
    @staticmethod
    def const(t):
        return t.to(DEV)

    @staticmethod
    def norm(x):
        return _ops().instnorm_act(x, _ops().ACT_RELU)

    @staticmethod
    def conv(x, w, b, k, s, p, tr=False):
        return _ops().conv2d(x, w, b, k, s, p, 1, transposed=tr)

    @staticmethod
    def conv_norm(x, w, b, k, s, p, tr=False):
        """(y, ReLU(IN(y))) with the statistics from the convolution's epilogue"""
        ops = _ops()
        y, stats = ops.conv2d_stats(x, w, b, k, s, p, 1, transposed=tr)
        return y, ops.instnorm_apply(y, stats, ops.ACT_RELU)


class Ref:
    @staticmethod
    def const(t):
        return t.double()

    norm = staticmethod(t_norm)
    conv = staticmethod(t_conv)

    @staticmethod
    def conv_norm(x, w, b, k, s, p, tr=False):
        y = t_conv(x, w, b, k, s, p, tr)
        return y, t_norm(y)


def conv_params(Ci, Co, k, seed, tr=False):
    return [rnd((Ci, Co, k, k) if tr else (Co, Ci, k, k), seed, (Ci * k * k) ** -0.5), rnd((Co,), seed + 1, 0.3)]


@contextlib.contextmanager
def kernel_list(names):
    """Appends the symbols of every kernel the library launches inside the block to `names`."""
    ops = _ops()
    ops.KernelTimer.start()
    try:
        yield
        torch.cuda.synchronize()
        names.extend(nm for nm, _ in ops.KernelTimer.kernels())
    finally:
        ops.KernelTimer.stop()


# ==========================================================================================================
# A. backward sums with more than one consumer
# ==========================================================================================================
def check_norm_graph(name, graph, leaves, kinds, monkeypatch, tagging=1):
    """graph(P, leaves) -> (loss, [intermediates to differentiate as well]); kinds: one of 'dx' (an input gradient that runs through
    the norm's backward), 'dw', 'db' (of a convolution), 'db0' (bias of a convolution that FEEDS an InstanceNorm: exactly zero)
    per leaf and per intermediate; ('db0', j): the gradient of that convolution's output is entry j.  tagging: how many convolutions of
    the graph hang backward sums on their dx (each launches one p32_bsum_finalize_kernel) -- the graph does exercise the tag."""
    ops = _ops()
    monkeypatch.setenv("MSTG_BSUMS_ALL", "1")  # as test_norm_backward_sums_from_the_consumer_convolution: every variant that can
    ops.refresh_env()
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MSTG_NORM_BSUMS", mode)
        t = [v.to(DEV).requires_grad_(True) for v in leaves]
        loss, extra = graph(Hip, t)
        names = []
        with kernel_list(names):
            got[mode] = [v.cpu() for v in torch.autograd.grad(loss, t + extra)]
        assert sum("p32_bsum_finalize_kernel" in nm for nm in names) == (tagging if mode == "1" else 0), (mode, names)
    t64 = [v.double().requires_grad_(True) for v in leaves]
    loss, extra = graph(Ref, t64)
    g64 = torch.autograd.grad(loss, t64 + extra)
    assert len(kinds) == len(g64)
    for j, kind in enumerate(kinds):
        a, a0, r = got["1"][j], got["0"][j], g64[j]
        if kind == "dx":
            report(f"{name}: gradient {j} (dx) vs torch fp64", rel_l2(a, r), 5e-5)
            report(f"{name}: gradient {j} (dx) vs statistics pass", rel_l2(a, a0), 2e-6)
        elif kind in ("dw", "db"):
            report(f"{name}: gradient {j} ({kind}) vs torch fp64", rel_l2(a, r), 1e-4)
        else:
            # sum over the pixels of a gradient that InstanceNorm's backward has made mean-free: the exact value is 0 and a relative
            # error against it means nothing; the convolution-db bar (1e-4) is applied to what the sum is taken over, sum |dy|
            dy = g64[kind[1]]
            scale = float(dy.abs().sum(dim=(0, 1, 2)).max())
            err = float((a.double() - r).abs().max()) / scale
            print(f"  [parity] {name}: gradient {j} (bias in front of a norm, exact value 0) |err| / sum|dy| {err:.2e} (tol 1e-04)")
            assert err <= 1e-4


# N = 3, 40 x 36, 16 -> 32 for the 4x4 stride-2 layer and N = 2, 32 x 32 for the 1x1 layers: the smallest shapes of
# test_norm_backward_sums_from_the_consumer_convolution, more than one tile and more than one image
def _fanout_graph(conv_first, producer):
    m, ga, gb = rnd((3, 40, 36, 16), 61), rnd((3, 20, 18, 32), 62), rnd((3, 40, 36, 16), 63)

    def graph(P, t):
        if producer:
            y, z = P.conv_norm(t[0], t[1], t[2], 4, 2, 1, True)
            w, b, extra = t[3], t[4], [y]
        else:
            z = P.norm(t[0])
            w, b, extra = t[1], t[2], []
        if conv_first:
            a = P.conv(z, w, b, 4, 2, 1)
            c = z * P.const(m)
        else:
            c = z * P.const(m)
            a = P.conv(z, w, b, 4, 2, 1)
        return (a * P.const(ga)).sum() + (c * P.const(gb)).sum(), extra
    return graph


@pytest.mark.parametrize("order", ["conv_created_first", "conv_created_last"])
def test_bsums_tagging_conv_plus_torch_consumer(order, monkeypatch):
    """z = ReLU(IN(x)) feeds a 4x4 stride-2 convolution (which tags its dx with the norm's backward sums) and a plain torch
    multiplication.  The engine runs the later-created consumer first: with the convolution created LAST its tagged dx arrives first
    and the product's gradient is added into it in place (the attribute survives, the sums are stale); created first, its dx is added
    into the other gradient and the attribute is gone."""
    leaves = [rnd((3, 40, 36, 16), 51, 1.3) + 0.2] + conv_params(16, 32, 4, 52)
    check_norm_graph(f"IN -> conv4x4 + torch mul, {order}", _fanout_graph(order == "conv_created_first", False), leaves,
                     ["dx", "dw", "db"], monkeypatch)


@pytest.mark.parametrize("order", ["conv_created_first", "conv_created_last"])
def test_bsums_statistics_from_a_producer(order, monkeypatch):
    """The same graph with the norm applied from a producer's epilogue statistics (conv2d_stats -> instnorm_apply, whose backward is
    InstNormActFn's): a transposed 4x4 layer 32 -> 16, 20 x 18 -> 40 x 36."""
    ops = _ops()
    assert ops.conv_norm_supported(3, 20, 18, 32, 16, 4, 2, 1, 1, 1)
    leaves = [rnd((3, 20, 18, 32), 71, 1.2) + 0.1] + conv_params(32, 16, 4, 72, tr=True) + conv_params(16, 32, 4, 74)
    check_norm_graph(f"convT(stats) -> IN apply -> conv4x4 + torch mul, {order}", _fanout_graph(order == "conv_created_first", True),
                     leaves, ["dx", "dw", ("db0", 5), "dw", "db", "dx"], monkeypatch)


def test_bsums_two_tagging_convolutions(monkeypatch):
    """z feeds a 4x4 stride-2 16 -> 32 layer and a 1x1 16 -> 16 layer: both tag their dx with the same token, the first one's
    attribute arrives on the sum of the two."""
    ga, gc = rnd((3, 20, 18, 32), 82), rnd((3, 40, 36, 16), 83)

    def graph(P, t):
        z = P.norm(t[0])
        a = P.conv(z, t[1], t[2], 4, 2, 1)
        c = P.conv(z, t[3], t[4], 1, 1, 0)
        return (a * P.const(ga)).sum() + (c * P.const(gc)).sum(), []
    leaves = [rnd((3, 40, 36, 16), 81, 1.3) + 0.2] + conv_params(16, 32, 4, 84) + conv_params(16, 16, 1, 86)
    check_norm_graph("IN -> conv4x4 and conv1x1", graph, leaves, ["dx", "dw", "db", "dw", "db"], monkeypatch, tagging=2)


def test_bsums_skip_connection(monkeypatch):
    """out = conv1x1(z) + z, 32 -> 32."""
    g = rnd((2, 32, 32, 32), 92)

    def graph(P, t):
        z = P.norm(t[0])
        return ((P.conv(z, t[1], t[2], 1, 1, 0) + z) * P.const(g)).sum(), []
    leaves = [rnd((2, 32, 32, 32), 91, 1.3) + 0.2] + conv_params(32, 32, 1, 93)
    check_norm_graph("IN -> conv1x1 + skip", graph, leaves, ["dx", "dw", "db"], monkeypatch)


def test_bsums_backward_twice_takes_the_shortcut_both_times(monkeypatch):
    """Single-consumer chain, backward twice over a retained graph: bit-equal gradients, and the second run still gets the norm's
    reductions from the convolution (no norm_partial_kernel<true>)."""
    ops = _ops()
    monkeypatch.setenv("MSTG_BSUMS_ALL", "1")
    ops.refresh_env()
    leaves = [rnd((3, 40, 36, 16), 51, 1.3) + 0.2] + conv_params(16, 32, 4, 52)
    t = [v.to(DEV).requires_grad_(True) for v in leaves]
    y = ops.conv2d(ops.instnorm_act(t[0], ops.ACT_RELU), t[1], t[2], 4, 2, 1)
    loss = (y * rnd(tuple(y.shape), 54).to(DEV)).sum()
    runs = []
    for _ in range(2):
        names = []
        with kernel_list(names):
            g = torch.autograd.grad(loss, t, retain_graph=True)
        runs.append(([v.clone() for v in g], names))
    for (g, names) in runs:
        assert any("p32_bsum_finalize_kernel" in nm for nm in names), names
        assert not any(nm.startswith("norm_partial_kernel<true>") for nm in names), names
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    t64 = [v.double().requires_grad_(True) for v in leaves]
    g64 = torch.autograd.grad((t_conv(t_norm(t64[0]), t64[1], t64[2], 4, 2, 1) * rnd(tuple(y.shape), 54).double()).sum(), t64)
    report("IN -> conv4x4, second backward: dx vs torch fp64", rel_l2(runs[1][0][0], g64[0]), 5e-5)
    report("IN -> conv4x4, second backward: dw vs torch fp64", rel_l2(runs[1][0][1], g64[1]), 1e-4)
    report("IN -> conv4x4, second backward: db vs torch fp64", rel_l2(runs[1][0][2], g64[2]), 1e-4)


# ==========================================================================================================
# B. the pack cache follows the weights
# ==========================================================================================================
class Case:
    """One cached kind on one layer.  tensors: initial parameter values; prep(ps, N) -> state (untimed: inputs, and for the backward
    kinds the forward); go(state, ps) -> output tensors (timed: the launch whose pack is under test); ref(ps64, N) -> the same outputs
    in torch fp64; tols: bar of each output against ref."""

    def __init__(self, name, tensors, prep, go, ref, tols, env=(), expect=""):
        self.name, self.tensors, self.prep, self.go, self.ref, self.tols, self.env = name, tensors, prep, go, ref, tols, env
        self.expect = expect  # a kernel the launch under test must contain: the cached kind really is the one the case names


def _conv_case(name, kind, Ci, Co, k, s, p, dil, tr, H, W, seed, expect=""):
    def xin(N):
        return rnd((N, H, W, Ci), seed + 10 + N, 1.2)

    def gout(shape):
        return rnd(shape, seed + 20 + shape[0])

    def hip_y(x, ps):
        return _ops().conv2d(x, ps[0], ps[1], k, s, p, dil, transposed=tr)

    def ref_y(x, ps):
        return t_conv(x, ps[0], ps[1], k, s, p, tr, dil)
    if kind == "fwd":
        return Case(name, conv_params(Ci, Co, k, seed, tr), lambda ps, N: xin(N).to(DEV), lambda x, ps: [hip_y(x, ps)],
                    lambda ps, N: [ref_y(xin(N).double(), ps)], [2e-5], expect=expect)

    def prep(ps, N):
        x = xin(N).to(DEV).requires_grad_(True)
        y = hip_y(x, ps)
        return x, (y * gout(tuple(y.shape)).to(DEV)).sum()

    def ref(ps, N):
        x = xin(N).double().requires_grad_(True)
        y = ref_y(x, ps)
        return list(torch.autograd.grad((y * gout(tuple(y.shape)).double()).sum(), [x]))
    return Case(name, conv_params(Ci, Co, k, seed, tr), prep, lambda st, ps: list(torch.autograd.grad(st[1], [st[0]])), ref, [2e-5],
                expect=expect)


def _bsums_case():
    """dgrad_bsums: the input gradient of a 4x4 stride-2 16 -> 32 layer behind InstanceNorm + ReLU, 40 x 36.  Outputs: the convolution's
    dx and the norm's (which uses the sums of the same launch; 5e-5 is the suite's bar for that gradient against torch)."""
    def xin(N):
        return rnd((N, 40, 36, 16), 310 + N, 1.3) + 0.2

    def gout(N):
        return rnd((N, 20, 18, 32), 320 + N)

    def prep(ps, N):
        ops = _ops()
        x = xin(N).to(DEV).requires_grad_(True)
        z = ops.instnorm_act(x, ops.ACT_RELU)
        return x, z, (ops.conv2d(z, ps[0], ps[1], 4, 2, 1) * gout(N).to(DEV)).sum()

    def ref(ps, N):
        x = xin(N).double().requires_grad_(True)
        z = t_norm(x)
        return list(torch.autograd.grad((t_conv(z, ps[0], ps[1], 4, 2, 1) * gout(N).double()).sum(), [z, x]))
    return Case("dgrad_bsums k4s2 16->32 40x36", conv_params(16, 32, 4, 300), prep,
                lambda st, ps: list(torch.autograd.grad(st[2], [st[1], st[0]])), ref, [2e-5, 5e-5], env=(("MSTG_BSUMS_ALL", "1"),),
                expect="p32_bsum_finalize_kernel")


def _stats_ref(y):
    return [y, y.mean(dim=(1, 2)), (y.var(dim=(1, 2), unbiased=False) + 1e-5).rsqrt()]


def _stats_case():
    """fwd_norm through conv2d_stats: 4x4 stride-2 16 -> 32 at 40 x 36 (Ho * Wo = 360 >= 256); outputs y, mean, rstd."""
    def xin(N):
        return rnd((N, 40, 36, 16), 410 + N, 1.3) + 0.2

    def go(x, ps):
        y, st = _ops().conv2d_stats(x, ps[0], ps[1], 4, 2, 1)
        return [y, st[..., 0], st[..., 1]]
    return Case("fwd_norm conv2d_stats k4s2 16->32 40x36", conv_params(16, 32, 4, 400), lambda ps, N: xin(N).to(DEV), go,
                lambda ps, N: _stats_ref(t_conv(xin(N).double(), ps[0], ps[1], 4, 2, 1)), [2e-5, 2e-5, 2e-5], expect="p32_norm_finalize_kernel")


def _fusion_case():
    """fwd_norm through the MultiScaleBlock fusion path: 1x1 16 -> 16 on ReLU(IN(cat)), normalised on load, 16 x 16."""
    def xin(N):
        return rnd((N, 16, 16, 16), 510 + N, 1.7) - 0.2

    def go(x, ps):
        y, st = _ops().MSFusionFn.apply(x, ps[0], ps[1])
        return [y, st[..., 0], st[..., 1]]
    return Case("fwd_norm MSFusionFn 1x1 16->16 16x16", conv_params(16, 16, 1, 500), lambda ps, N: xin(N).to(DEV), go,
                lambda ps, N: _stats_ref(t_conv(t_norm(xin(N).double()), ps[0], ps[1], 1, 1, 0)), [2e-5, 2e-5, 2e-5],
                expect="p32_norm_finalize_kernel")


def _ms_params(ch, seed):
    out = []
    for j, (k, _, _) in enumerate(((1, 0, 1), (3, 1, 1), (3, 2, 2), (3, 4, 4))):
        out += [rnd((ch // 4, ch, k, k), seed + 2 * j, (ch * k * k) ** -0.5), rnd((ch // 4,), seed + 2 * j + 1, 0.3)]
    return out


def _ms_case(kind, ch, sizes, seed):
    """ms_fwd / ms_dgrad of MSBranchesFn at every (H, W) of `sizes` in turn on the same parameters (16 x 16 and 8 x 8 are two ms_fwd
    keys: maps below 16 rows go to another kernel, with another pack)."""
    name = f"ms_{kind} ch{ch} " + "+".join(f"{h}x{w}" for h, w in sizes)

    def xin(N, h, w):
        return rnd((N, h, w, ch), seed + 100 + N + h, 1.1)

    def gout(N, h, w, j):
        return rnd((N, h, w, ch), seed + 200 + N + h + j)
    if kind == "fwd":
        return Case(name, _ms_params(ch, seed), lambda ps, N: [xin(N, h, w).to(DEV) for h, w in sizes],
                    lambda xs, ps: [_ops().MSBranchesFn.apply(x, *ps)[0] for x in xs],
                    lambda ps, N: [t_branches(xin(N, h, w).double(), ps) for h, w in sizes], [2e-5] * len(sizes), expect="ms_fwd")

    def prep(ps, N):
        st = []
        for h, w in sizes:
            x = xin(N, h, w).to(DEV).requires_grad_(True)
            y, xr = _ops().MSBranchesFn.apply(x, *ps)
            st.append((x, (y * gout(N, h, w, 0).to(DEV)).sum() + (xr * gout(N, h, w, 1).to(DEV)).sum()))
        return st

    def ref(ps, N):
        out = []
        for h, w in sizes:
            x = xin(N, h, w).double().requires_grad_(True)
            loss = (t_branches(x, ps) * gout(N, h, w, 0).double()).sum() + (x * gout(N, h, w, 1).double()).sum()
            out += list(torch.autograd.grad(loss, [x]))
        return out
    return Case(name, _ms_params(ch, seed), prep, lambda st, ps: [torch.autograd.grad(loss, [x])[0] for x, loss in st], ref,
                [2e-5] * len(sizes), expect="ms_dgrad_kernel")


CASES = {c.name: c for c in [
    _conv_case("fwd igemm k3 16->4 16x24", "fwd", 16, 4, 3, 1, 1, 1, False, 16, 24, 1000, "igemm_"),
    _conv_case("dgrad igemm k3 16->4 16x24", "dgrad", 16, 4, 3, 1, 1, 1, False, 16, 24, 1000, "igemm_"),
    _conv_case("fwd conv_p32 k4s2 16->16 20x36", "fwd", 16, 16, 4, 2, 1, 1, False, 20, 36, 1100, "conv_p32_kernel"),
    _conv_case("dgrad conv_p32 k4s2 16->16 20x36", "dgrad", 16, 16, 4, 2, 1, 1, False, 20, 36, 1100, "conv_p32_kernel"),
    _conv_case("fwd convT 16->16 5x7", "fwd", 16, 16, 4, 2, 1, 1, True, 5, 7, 1200),
    _conv_case("dgrad convT 16->16 5x7", "dgrad", 16, 16, 4, 2, 1, 1, True, 5, 7, 1200),
    _bsums_case(), _stats_case(), _fusion_case(),
    _ms_case("fwd", 16, [(16, 16), (8, 8)], 2000), _ms_case("dgrad", 16, [(16, 16), (8, 8)], 2000),
    _ms_case("fwd", 32, [(16, 16)], 2100), _ms_case("dgrad", 32, [(16, 16)], 2100),
]}
P32_SWITCHABLE = [n for n in CASES if not n.startswith(("dgrad_bsums", "fwd_norm"))]  # those two exist on the persistent kernel only


class Owner:
    """The parameters of one layer as a training script holds them: nn.Parameters, in a module, optionally in a FlatAdam."""

    def __init__(self, case, flat_adam=False, parameters=True):
        self.case = case
        if parameters:
            self.ps = [torch.nn.Parameter(t.to(DEV)) for t in case.tensors]
            self.mod = torch.nn.Module()
            self.mod.ps = torch.nn.ParameterList(self.ps)
        else:
            self.ps = [t.to(DEV).requires_grad_(True) for t in case.tensors]
        self.opt = None
        if flat_adam:
            from mstg_hip.optim import FlatAdam
            self.opt = FlatAdam(self.ps, lr=1.0)  # lr 1: one step moves every weight by about 1, an O(1) change like the others

    def noise(self, j):
        return rnd(tuple(self.ps[j].shape), 900 + j, 0.1).to(DEV)

    def target(self, j):
        return -2.0 * self.ps[j].detach() + self.noise(j)

    def run(self, N, names=None, cached=True):
        """Outputs of the case (on the CPU) at batch size N; names: receives the kernels of the launch under test."""
        before = os.environ.get("MSTG_NO_PACK_CACHE")
        try:
            if not cached:
                os.environ["MSTG_NO_PACK_CACHE"] = "1"  # read per call on the Python side: no refresh, the epoch stays
            st = self.case.prep(self.ps, N)
            with kernel_list(names if names is not None else []):
                outs = self.case.go(st, self.ps)
            return [o.detach().cpu() for o in outs]
        finally:
            if before is None:
                os.environ.pop("MSTG_NO_PACK_CACHE", None)
            else:
                os.environ["MSTG_NO_PACK_CACHE"] = before

    def values(self):
        return [p.detach().cpu().double() for p in self.ps]

    def check_against_torch(self, outs, N, what, values=None):
        ref = self.case.ref(self.values() if values is None else values, N)
        for j, (a, r, tol) in enumerate(zip(outs, ref, self.case.tols)):
            report(f"{self.case.name} [{what}] output {j} vs torch fp64", rel_l2(a, r), tol)


def packs(names):
    return [nm for nm in names if "pack" in nm]  # pack_filter_kernel, p32_pack_kernel, p32i_/p32d_pack_kernel, ms_pack_*_kernel


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def follow(own, write, what, N=2, expect_miss=True, values_change=True):
    """Three runs on unchanged weights (miss, hit, hit), the write, and two more (miss, hit).  Every run is bit-identical to the
    uncached run on the weights of the moment (the convolution, input-gradient and MultiScale kernels have no atomics and a fixed
    summation order) and agrees with torch fp64."""
    case = own.case
    n0, nms = [], [[] for _ in range(5)]
    before = own.values()
    ref = own.run(N, n0, cached=False)
    outs = [own.run(N, nms[i]) for i in range(3)]
    write(own)
    outs.append(own.run(N, nms[3]))
    ref2 = own.run(N, cached=False)
    outs.append(own.run(N, nms[4]))
    marks = ["hit " if not packs(nm) else "miss" for nm in nms]
    print(f"  [pack] {case.name:44s} {what:30s} {marks[0]} {marks[1]} {marks[2]} | write | {marks[3]} {marks[4]}")
    assert packs(n0), f"{case.name}: the uncached run launched no pack kernel: {n0}"
    assert any(case.expect in nm for nm in n0), f"{case.name}: no {case.expect} among {n0}"
    own.check_against_torch(ref, N, "uncached", before)
    for i in range(3):
        assert bool(packs(nms[i])) == (i == 0), f"{case.name}: run {i + 1} on unchanged weights: {marks[i]}, {nms[i]}"
        assert same(outs[i], ref), f"{case.name}: run {i + 1} on unchanged weights differs from the uncached run"
    assert same(outs[3], ref2), f"{case.name}: after {what}: differs from the uncached run on the new weights (stale pack?)"
    if values_change:
        assert not same(ref2, ref), f"{case.name}: {what} did not change the result -- the test could not see a stale pack"
    if expect_miss:
        assert packs(nms[3]), f"{case.name}: no re-pack after {what}: {nms[3]}"
    assert not packs(nms[4]), f"{case.name}: second run after {what} packed again: {nms[4]}"
    assert same(outs[4], ref2), f"{case.name}: second run after {what} differs from the uncached run"
    own.check_against_torch(outs[3], N, f"after {what}")


def _set_env(case, monkeypatch):
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    if case.env:
        _ops().refresh_env()


# ---- writers: each takes the Owner; (flat_adam, function) -------------------------------------------------
def w_copy(own, idx=None):
    with torch.no_grad():
        for j in (range(len(own.ps)) if idx is None else idx):
            own.ps[j].copy_(own.target(j))


def w_load_state_dict(own):
    own.mod.load_state_dict({f"ps.{j}": own.target(j) for j in range(len(own.ps))})


def w_sgd(own):
    opt = torch.optim.SGD(own.ps, lr=1.0)
    for j, p in enumerate(own.ps):
        p.grad = 3.0 * p.detach() - own.noise(j)  # p - 1.0 * grad = -2 p + noise
    opt.step()
    for p in own.ps:
        p.grad = None


def w_flat_adam_step(own):
    own.opt.grad.copy_(rnd((own.opt.numel,), 77).to(DEV))
    own.opt.step()  # a kernel handed raw pointers: seen through PACK_EPOCH only


def w_flat_inplace(own):
    own.opt.flat.mul_(-2.0).add_(rnd((own.opt.numel,), 78, 0.1).to(DEV))  # torch op on the buffer the parameters are views of


def w_rehome(own):
    """module.to(float64).to(float32) with the values changed on the way: p.data is a new tensor twice, no version counter moves, and
    nothing keeps the allocator from handing the second one the block the first one left."""
    own.mod.to(torch.float64)
    for j, p in enumerate(own.ps):
        p.data = -2.0 * p.data + own.noise(j).double()
    own.mod.to(torch.float32)


def w_data_then_bump(own):
    for p in own.ps:
        p.data.mul_(2)  # invisible to the stamp (p._version does not move) ...
    _ops().bump_pack_epoch()  # ... hence the documented remedy


WRITERS = {"p.copy_": (False, w_copy), "load_state_dict": (False, w_load_state_dict), "SGD.step": (False, w_sgd),
           "FlatAdam.step": (True, w_flat_adam_step), "FlatAdam.flat in-place": (True, w_flat_inplace),
           "module.to(f64).to(f32)": (False, w_rehome), "p.data.mul_ + bump_pack_epoch": (False, w_data_then_bump)}


@pytest.mark.parametrize("writer", list(WRITERS))
@pytest.mark.parametrize("case", list(CASES))
def test_pack_cache_hits_and_follows_every_writer(case, writer, monkeypatch):
    case = CASES[case]
    _set_env(case, monkeypatch)
    flat, fn = WRITERS[writer]
    follow(Owner(case, flat_adam=flat), fn, writer)


@pytest.mark.parametrize("case", P32_SWITCHABLE)
def test_pack_cache_refresh_env_after_flipping_p32(case, monkeypatch):
    """ops.refresh_env() after MSTG_P32=0: other kernels with other pack formats take the layers of the persistent kernel (the
    weights stay, so the results need not change; the uncached reference runs under the same switch)."""
    def flip(own):
        monkeypatch.setenv("MSTG_P32", "0")
        _ops().refresh_env()
    follow(Owner(CASES[case]), flip, "MSTG_P32=0 + refresh_env", values_change=False)


@pytest.mark.parametrize("case", ["fwd conv_p32 k4s2 16->16 20x36", "fwd_norm MSFusionFn 1x1 16->16 16x16", "ms_dgrad ch16 16x16+8x8"])
def test_pack_cache_data_rehomed_onto_the_address_it_left(case):
    """p.data replaced by a tensor that lies where the old one lay, with other values -- what module.half().float() gives when the
    allocator hands the block just freed to the next tensor of its size (it prefers to).  No version counter moves and data_ptr is
    the old one, so a stamp of (id, data_ptr, versions) alone cannot tell.  The writer frees the parameter's storage and allocates
    until the address comes back (at most 64 times); a cache that keeps the old storage allocated never lets it come back, and the
    re-homed tensor lands elsewhere."""
    def write(own):
        for j, p in enumerate(own.ps):
            new, shape, ptr = own.target(j), tuple(p.shape), p.data_ptr()
            p.data = torch.empty(0, device=DEV)  # the parameter lets go of its storage
            held = []
            for _ in range(64):
                t = torch.empty(shape, dtype=torch.float32, device=DEV)
                if t.data_ptr() == ptr:
                    break
                held.append(t)
            t.copy_(new)
            p.data = t
    follow(Owner(CASES[case]), write, "p.data = tensor at old address")


BIAS_ONLY = ["fwd igemm k3 16->4 16x24", "fwd conv_p32 k4s2 16->16 20x36", "fwd convT 16->16 5x7", "fwd_norm conv2d_stats k4s2 16->32 40x36",
             "fwd_norm MSFusionFn 1x1 16->16 16x16"]


@pytest.mark.parametrize("case", BIAS_ONLY)
def test_pack_cache_bias_alone_refreshes_the_forward(case, monkeypatch):
    """The forward packs hold the bias too: the stamp covers both owners, though the cache hangs on the weight."""
    follow(Owner(CASES[case]), lambda own: w_copy(own, [1]), "bias only")


@pytest.mark.parametrize("case", ["dgrad igemm k3 16->4 16x24", "dgrad conv_p32 k4s2 16->16 20x36", "dgrad_bsums k4s2 16->32 40x36"])
def test_pack_cache_bias_alone_and_the_input_gradient(case, monkeypatch):
    """The input gradient does not depend on the bias: a re-pack is not required, the result is."""
    case = CASES[case]
    _set_env(case, monkeypatch)
    follow(Owner(case), lambda own: w_copy(own, [1]), "bias only", expect_miss=False, values_change=False)


@pytest.mark.parametrize("case,idx,what", [("ms_fwd ch16 16x16+8x8", 7, "b4 only"), ("ms_fwd ch16 16x16+8x8", 6, "w4 only"),
                                           ("ms_fwd ch32 16x16", 7, "b4 only"), ("ms_fwd ch32 16x16", 6, "w4 only"),
                                           ("ms_dgrad ch16 16x16+8x8", 6, "w4 only"), ("ms_dgrad ch32 16x16", 6, "w4 only")])
def test_pack_cache_every_owner_of_the_multiscale_pack(case, idx, what):
    """The MultiScale packs hang on w1 and hold all eight tensors (ms_fwd) / all four filters (ms_dgrad)."""
    follow(Owner(CASES[case]), lambda own: w_copy(own, [idx]), what)


BATCH = ["fwd conv_p32 k4s2 16->16 20x36", "dgrad conv_p32 k4s2 16->16 20x36", "dgrad_bsums k4s2 16->32 40x36",
         "fwd_norm conv2d_stats k4s2 16->32 40x36", "fwd_norm MSFusionFn 1x1 16->16 16x16"]


@pytest.mark.parametrize("case", BATCH)
def test_pack_cache_batch_size_changes_both_ways(case, monkeypatch):
    """The persistent kernels' keys drop the batch size (one pack serves a generator's 2N and N passes), and the workspaces of
    dgrad_bsums / fwd_norm carry per-image partial sums behind the pack: N = 3, 1, 3 and N = 1, 3, 1 on unchanged weights."""
    case = CASES[case]
    _set_env(case, monkeypatch)
    for seq in ((3, 1, 3), (1, 3, 1)):
        own, row = Owner(case), []
        for i, N in enumerate(seq):
            nm = []
            out = own.run(N, nm)
            row.append(f"N={N} " + ("hit" if not packs(nm) else "miss"))
            assert same(out, own.run(N, cached=False)), f"{case.name}: N sequence {seq}, run {i + 1} differs from the uncached run"
            own.check_against_torch(out, N, f"N sequence {seq}, run {i + 1}")
            if i == 0:
                assert packs(nm)
            if seq == (3, 1, 3) and i == 1:
                assert not packs(nm), f"{case.name}: N=1 after N=3 packed again: {nm}"
        print(f"  [pack] {case.name:44s} " + ", ".join(row))


@pytest.mark.parametrize("case", ["fwd igemm k3 16->4 16x24", "dgrad conv_p32 k4s2 16->16 20x36", "fwd_norm conv2d_stats k4s2 16->32 40x36",
                                  "ms_fwd ch16 16x16+8x8", "ms_dgrad ch32 16x16"])
def test_pack_cache_never_used_for_plain_tensors(case):
    """Weights that are tensors, not nn.Parameters (the discriminator's spectral-norm temporaries): every launch packs."""
    own = Owner(CASES[case], parameters=False)
    ref = own.run(2, cached=False)
    for i in range(3):
        nm = []
        out = own.run(2, nm)
        assert packs(nm), f"{case}: run {i + 1} with plain tensors launched no pack kernel: {nm}"
        assert same(out, ref)
    own.check_against_torch(out, 2, "plain tensors")


@pytest.mark.parametrize("case", ["fwd conv_p32 k4s2 16->16 20x36", "dgrad igemm k3 16->4 16x24", "ms_fwd ch16 16x16+8x8"])
def test_pack_cache_is_per_stream(case):
    """Stream A, B, A, A: a workspace is not shared between streams (launches of the other one may still read it), so each change of
    stream packs into a fresh one; every result is right."""
    own = Owner(CASES[case])
    ref = own.run(2, cached=False)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    row = []
    for s, hit in ((a, False), (b, False), (a, False), (a, True)):
        nm = []
        with torch.cuda.stream(s):
            out = own.run(2, nm)
        row.append("hit" if not packs(nm) else "miss")
        assert same(out, ref), f"{case}: differs from the uncached run on stream {'A' if s is a else 'B'} ({row})"
        assert (not packs(nm)) == hit, f"{case}: {row}"
    own.check_against_torch(out, 2, "streams")
    print(f"  [pack] {case:44s} streams A B A A: " + " ".join(row))


# ==========================================================================================================
# C. one layer twice in one graph
# ==========================================================================================================
def _twice(name, params, hip, ref, xs, gys):
    """hip(x, ps) / ref(x, ps) -> list of outputs; the layer runs on each input of xs (N = 2 and N = 1) in ONE graph."""
    ops = _ops()
    from mstg_hip.optim import FlatAdam
    # torch fp64
    p64 = [t.double().requires_grad_(True) for t in params]
    x64 = [x.double().requires_grad_(True) for x in xs]
    o64 = [o for x in x64 for o in ref(x, p64)]
    g64 = torch.autograd.grad(sum((o * g.double()).sum() for o, g in zip(o64, gys)), x64 + p64)

    def graph(ps):
        xd = [x.to(DEV).requires_grad_(True) for x in xs]
        outs = [o for x in xd for o in hip(x, ps)]
        return xd, outs, sum((o * g.to(DEV)).sum() for o, g in zip(outs, gys))
    # gradients returned to autograd
    ps = [torch.nn.Parameter(t.to(DEV)) for t in params]
    xd, outs, loss = graph(ps)
    got = torch.autograd.grad(loss, xd + ps)
    for j, (a, r) in enumerate(zip(outs, o64)):
        report(f"{name}: output {j}", rel_l2(a, r), 2e-5)
    for j, (a, r) in enumerate(zip(got, g64)):
        report(f"{name}: returned gradient {j} {tuple(a.shape)}", rel_l2(a, r), 2e-5 if j < len(xs) else 1e-4)
    # ... and added into p.grad by the reduce kernels, twice per parameter
    ps2 = [torch.nn.Parameter(t.to(DEV)) for t in params]
    opt = FlatAdam(ps2)
    opt.zero_grad()
    seen = []
    hooks = [p.register_hook(lambda grad, j=j: seen.append(j) if grad is not None else None) for j, p in enumerate(ps2)]
    with ops.direct_param_grads():
        xd2, _, loss2 = graph(ps2)
        loss2.backward()
    for h in hooks:
        h.remove()
    opt.check_views()
    assert not seen, f"{name}: gradients of parameters {seen} came back through autograd under direct_param_grads"
    direct = [x.grad for x in xd2] + [p.grad for p in ps2]
    for j, (a, r, b) in enumerate(zip(direct, g64, got)):
        report(f"{name}: in-place gradient {j} {tuple(a.shape)}", rel_l2(a, r), 2e-5 if j < len(xs) else 1e-4)
        # (0 + g1) + g2 against autograd's g1 + g2 of the same kernels' results: the same fp32 sum
        assert torch.equal(a, b), f"{name}: gradient {j} differs between the in-place and the returned path: {rel_l2(a, b):.2e}"


def test_one_conv_layer_twice_in_one_graph():
    from mstg_hip.layers import HipConv2d
    layer = HipConv2d(16, 32, 4, stride=2, padding=1)

    def hip(x, ps):
        layer.weight, layer.bias = ps[0], ps[1]
        return [layer(x, nhwc=True)]
    xs = [rnd((2, 40, 36, 16), 3001, 1.2), rnd((1, 40, 36, 16), 3002, 1.2)]
    gys = [rnd((2, 20, 18, 32), 3003), rnd((1, 20, 18, 32), 3004)]
    _twice("HipConv2d k4s2 16->32 at N=2 and N=1", conv_params(16, 32, 4, 3005), hip, lambda x, ps: [t_conv(x, ps[0], ps[1], 4, 2, 1)], xs, gys)


def test_one_multiscale_block_twice_in_one_graph():
    xs = [rnd((2, 20, 18, 16), 3101, 1.1), rnd((1, 20, 18, 16), 3102, 1.1)]
    gys = [rnd((2, 20, 18, 16), 3103), rnd((2, 20, 18, 16), 3104), rnd((1, 20, 18, 16), 3105), rnd((1, 20, 18, 16), 3106)]
    _twice("MSBranchesFn ch16 at N=2 and N=1", _ms_params(16, 3110), lambda x, ps: list(_ops().MSBranchesFn.apply(x, *ps)),
           lambda x, ps: [t_branches(x, ps), x], xs, gys)
