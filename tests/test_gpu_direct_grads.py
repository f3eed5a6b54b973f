"""Parameter gradients added straight into p.grad (ops.direct_param_grads, the path EnhancedCycleGAN.train_step and PretrainStep
take) against the gradients the same Function returns to torch.autograd.grad, for every Function that has the path.

The parameters are nn.Parameters of an optim.FlatAdam, so that each .grad is a view into the optimizer's flat gradient buffer; the
WHOLE buffer, pad elements between parameters included, is filled with a seeded random vector s of the gradients' magnitude.  Two
forward + backward runs under direct_param_grads() must leave p.grad == (s_p + g_p) + g_p bit for bit: every reduce epilogue
computes r as it does without `accumulate` and stores *o + r.  The pad elements keep their seed, the input gradients are
bit-identical on the two paths, and -- so that this file stands alone -- the returned gradients g are held to fp64 autograd of the
torch definition at the bars of tests/test_gpu_ops.py::test_conv_fwd_bwd (2e-5 for y and dx, 1e-4 for dw and db).

That a gradient really went in place is seen from a tensor hook on the parameter: autograd hands it None where backward() returned
no gradient.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from test_gpu_ops import CONV_CASES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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


def _loss(outs, gys):
    return sum((o * g).sum() for o, g in zip(outs, gys))


def check_direct(name, fwd, ref, xs, tensors, gys, returned=()):
    """fwd(*inputs, *params) -> list of outputs on the HIP kernels; ref: the same in plain torch (called in fp64 on the CPU, outputs
    in the layout of fwd's).  xs: inputs that are no parameters, tensors: initial parameter values, gys: one output gradient per
    output; returned: indices of parameters whose gradient backward() hands to autograd even under direct_param_grads (autograd then
    adds it to the same .grad view).  Returns the symbols of the kernels launched by the two in-place runs."""
    from mstg_hip import ops
    from mstg_hip.optim import FlatAdam
    ps = [torch.nn.Parameter(t.to(DEV)) for t in tensors]
    opt = FlatAdam(ps)
    gys_d = [g.to(DEV) for g in gys]
    nx = len(xs)
    # (a) the returned path, on detached leaf copies
    leaves = [x.to(DEV).requires_grad_(True) for x in xs] + [p.detach().clone().requires_grad_(True) for p in ps]
    outs = fwd(*leaves)
    g = torch.autograd.grad(_loss(outs, gys_d), leaves)
    gx, gp = g[:nx], g[nx:]
    # (f) ... against fp64 autograd of the torch definition
    leaves64 = [t.double().clone().requires_grad_(True) for t in list(xs) + list(tensors)]
    outs64 = ref(*leaves64)
    g64 = torch.autograd.grad(_loss(outs64, [t.double() for t in gys]), leaves64)
    for j, (a, b) in enumerate(zip(outs, outs64)):
        report(f"{name} output {j}", rel_l2(a, b), 2e-5)
    for j, (a, b) in enumerate(zip(gx, g64[:nx])):
        report(f"{name} d input {j}", rel_l2(a, b), 2e-5)
    for j, (a, b) in enumerate(zip(gp, g64[nx:])):
        report(f"{name} d parameter {j} {tuple(a.shape)}", rel_l2(a, b), 1e-4)
    # the seed: the whole flat buffer, each parameter's stretch (and the pad behind it) at the magnitude of its gradient
    s = rnd((opt.numel,), 4242).to(DEV)
    for o, e, gj in zip(opt.offsets, opt.offsets[1:] + [opt.numel], gp):
        s[o:e] *= float(gj.abs().max()) or 1.0
    opt.grad.copy_(s)
    seen = []
    hooks = [p.register_hook(lambda grad, j=j: seen.append(j) if grad is not None else None) for j, p in enumerate(ps)]
    # (b) twice in place
    ops.KernelTimer.start()
    try:
        with ops.direct_param_grads():
            for _ in range(2):
                xl = [x.to(DEV).requires_grad_(True) for x in xs]
                _loss(fwd(*xl, *ps), gys_d).backward()
                for a, b in zip(xl, gx):  # (e)
                    assert torch.equal(a.grad, b), f"{name}: input gradient differs between the two paths"
        torch.cuda.synchronize()
        names = [nm for nm, _ in ops.KernelTimer.kernels()]
    finally:
        ops.KernelTimer.stop()
        for h in hooks:
            h.remove()
    assert sorted(seen) == sorted(list(returned) * 2), f"{name}: parameters whose gradient came back through autograd: {seen}"
    opt.check_views()
    # (c) p.grad == (s + g) + g, bit for bit
    pad = torch.ones(opt.numel, dtype=torch.bool, device=DEV)
    for j, (p, o, gj) in enumerate(zip(ps, opt.offsets, gp)):
        sp = s[o:o + p.numel()].view_as(p)
        want = (sp + gj) + gj
        assert torch.equal(p.grad, want), (f"{name}: parameter {j} {tuple(p.shape)}: {int((p.grad != want).sum())} of {p.numel()} elements "
                                           f"differ, rel-L2 {rel_l2(p.grad - sp, 2 * gj):.2e}")
        pad[o:o + p.numel()] = False
    # (d) the pad elements keep their seed
    assert torch.equal(opt.grad[pad], s[pad]), f"{name}: a pad element of the flat gradient buffer was written"
    return names


# ----------------------------------------------------------------------------------------------------------
# ConvFn / ConvStatsFn
# ----------------------------------------------------------------------------------------------------------
CASE = {c[0]: c for c in CONV_CASES}

# case -> the weight-gradient kernel family tests/golden/conv_routes.json pins for it
CONV_DIRECT = [
    ("k3 d1 16->4", "wgrad_kernel<"),  # pixel-split
    ("k4s2 8->16", "wgrad_kernel<"),
    ("stem7x7 3->8 nchw-in", "wgrad_kernel<"),
    ("head7x7 8->3 nchw-out tanh", "wgrad_kernel<"),
    ("convT 16->8", "wgrad_kernel<"),  # bias gradient by channel_sum, through autograd
    ("convT 8->3 nchw-out tanh", "wgrad_kernel<"),  # bias gradient by plane_sum_nchw, through autograd
    ("stem7x7 3->16 nchw-in", "wgrad7_kernel<1>"),
    ("head7x7 16->3 nchw-out tanh 8x12 (8-row tiles)", "wgrad7_kernel<2>"),
    ("k4s2 16->32", "wgrad_p32_kernel"),
    ("convT 32->16", "wgrad_p32_kernel"),
    ("p32 k4s2 16->64 2x2", "wgrad_p32_kernel"),
    ("p32 convT 64->16 1x1", "wgrad_p32_kernel"),
    ("k4s2 ragged 20x36", "wgrad_ts_kernel<"),
    ("1x1 16->48", "wgrad_1x1_kernel<1, 1>"),  # one channel block
    ("1x1 128->384 (wgrad in 2x2 channel blocks)", "wgrad_1x1_kernel<"),
    ("1x1 72->200 (uneven channel blocks)", "wgrad_1x1_kernel<"),
]


def _conv_setup(case):
    from mstg_hip import ops
    name, N, H, W, Cin, Cout, k, s, p, d, tr, x_nchw, y_nchw, act = case
    seed = sum(ord(c) for c in name) % 10000
    x = rnd((N, Cin, H, W) if x_nchw else (N, H, W, Cin), seed)
    w = rnd((Cin, Cout, k, k) if tr else (Cout, Cin, k, k), seed + 1, (2.0 / (Cin * k * k)) ** 0.5 * 1.7)
    b = rnd((Cout,), seed + 2, 0.3)
    Ho, Wo = ops.conv_out_hw(H, W, k, s, p, d, tr)
    gy = rnd((N, Cout, Ho, Wo) if y_nchw else (N, Ho, Wo, Cout), seed + 3)

    def fwd(x_, w_, b_):
        return [ops.conv2d(x_, w_, b_, k, s, p, d, transposed=bool(tr), x_nchw=bool(x_nchw), y_nchw=bool(y_nchw), act=act)]

    def ref(x_, w_, b_):
        xc = x_ if x_nchw else x_.permute(0, 3, 1, 2)
        y = F.conv_transpose2d(xc, w_, b_, stride=s, padding=p) if tr else F.conv2d(xc, w_, b_, stride=s, padding=p, dilation=d)
        if act == 3:
            y = torch.tanh(y)
        return [y if y_nchw else y.permute(0, 2, 3, 1)]

    return fwd, ref, x, w, b, gy


@pytest.mark.parametrize("name,family", CONV_DIRECT, ids=[c[0] for c in CONV_DIRECT])
def test_conv_direct_grads(name, family):
    from mstg_hip import _lib, ops
    case = CASE[name]
    _, N, H, W, Cin, Cout, k, s, p, d, tr, x_nchw, y_nchw, act = case
    Ho, Wo = ops.conv_out_hw(H, W, k, s, p, d, tr)
    desc = ops.make_desc(N, H, W, Cin, Ho, Wo, Cout, k, s, p, d, tr, x_nchw, y_nchw, accumulate=1)
    routed = _lib.load().mstg_conv2d_kernel_name(ctypes.byref(desc), 2).decode()
    assert routed.startswith(family), f"{name}: the weight gradient moved to {routed}"
    if family == "wgrad_1x1_kernel<":
        assert not routed.startswith("wgrad_1x1_kernel<1, 1>"), routed  # several channel blocks
    fwd, ref, x, w, b, gy = _conv_setup(case)
    names = check_direct(f"conv {name}", fwd, ref, [x], [w, b], [gy], returned=(1,) if tr else ())
    # the routed kernel and its reduce epilogue ran once per backward -- the 1x1 kernel once per channel block (uneven blocks run
    # other instantiations of it than the first block's, which is the one the name reports)
    blocks = names.count("wgrad_reduce_kernel") // 2
    stem = routed.split("<")[0]
    assert routed in names and sum(n.split("<")[0] == stem for n in names) == 2 * blocks, names
    assert names.count("wgrad_reduce_kernel") == 2 * blocks, names
    assert blocks >= 2 if family == "wgrad_1x1_kernel<" else blocks == 1, names


def test_conv_mixed_grad_slots_fall_back_to_returned():
    """The weight has a .grad and the bias has none: the fused launch cannot deliver one gradient in place and return the other, so
    ConvFn returns both; autograd adds dw to the existing slot and creates the bias's."""
    from mstg_hip import ops
    fwd, _, x, w, b, gy = _conv_setup(CASE["k3 d1 16->4"])
    leaves = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
    g = torch.autograd.grad(_loss(fwd(*leaves), [gy.to(DEV)]), leaves)
    wp, bp = torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(b.to(DEV))
    s = rnd(tuple(w.shape), 7, float(g[1].abs().max())).to(DEV)
    wp.grad = s.clone()
    seen = []
    hooks = [t.register_hook(lambda grad, j=j: seen.append(j) if grad is not None else None) for j, t in enumerate((wp, bp))]
    xl = x.to(DEV).requires_grad_(True)
    with ops.direct_param_grads():
        _loss(fwd(xl, wp, bp), [gy.to(DEV)]).backward()
    for h in hooks:
        h.remove()
    assert sorted(seen) == [0, 1]
    assert torch.equal(xl.grad, g[0])
    assert torch.equal(wp.grad, s + g[1])
    assert torch.equal(bp.grad, g[2])


@pytest.mark.parametrize("tr,N,H,W,Ci,Co", [(0, 3, 40, 36, 16, 32), (1, 3, 9, 11, 64, 32)])
def test_conv_stats_direct_grads(tr, N, H, W, Ci, Co):
    """ConvStatsFn (the convolution whose epilogue takes the following InstanceNorm's statistics): its backward is ConvFn's."""
    from mstg_hip import ops
    assert ops.conv_norm_supported(N, H, W, Ci, Co, 4, 2, 1, 1, tr)
    x = rnd((N, H, W, Ci), 21, 1.5) + 0.3
    w = rnd((Ci, Co, 4, 4) if tr else (Co, Ci, 4, 4), 22, (Ci * 16) ** -0.5)
    b = rnd((Co,), 23, 0.5)
    Ho, Wo = ops.conv_out_hw(H, W, 4, 2, 1, 1, tr)
    gy = rnd((N, Ho, Wo, Co), 24)

    def fwd(x_, w_, b_):
        return [ops.conv2d_stats(x_, w_, b_, 4, 2, 1, 1, transposed=bool(tr))[0]]

    def ref(x_, w_, b_):
        xc = x_.permute(0, 3, 1, 2)
        y = F.conv_transpose2d(xc, w_, b_, stride=2, padding=1) if tr else F.conv2d(xc, w_, b_, stride=2, padding=1)
        return [y.permute(0, 2, 3, 1)]

    names = check_direct(f"conv2d_stats T{tr} {Ci}->{Co}", fwd, ref, [x], [w, b], [gy], returned=(1,) if tr else ())
    assert names.count("wgrad_reduce_kernel") == 2, names


# ----------------------------------------------------------------------------------------------------------
# MSBranchesFn / MSFusionFn
# ----------------------------------------------------------------------------------------------------------
def _ms_branches(N, H, W, ch, reduce_kernel):
    from mstg_hip import _lib, ops
    assert _lib.load().mstg_msblock_fused_supported(ch)
    x = rnd((N, H, W, ch), 5)
    gy, gres = rnd((N, H, W, ch), 20), rnd((N, H, W, ch), 21)  # gres: over the block's residual connection (second output = x)
    tensors = []
    for j, k in enumerate((1, 3, 3, 3)):
        tensors += [rnd((ch // 4, ch, k, k), 6 + j, 0.2), rnd((ch // 4,), 10 + j, 0.2)]

    def fwd(x_, *wb):
        return list(ops.MSBranchesFn.apply(x_, *wb))

    def ref(x_, *wb):
        xc = x_.permute(0, 3, 1, 2)
        outs = [F.conv2d(xc, wb[2 * j], wb[2 * j + 1], padding=pad, dilation=dil) for j, (_, pad, dil) in enumerate(ops.MSBranchesFn.GEOM)]
        return [torch.cat(outs, 1).permute(0, 2, 3, 1), x_]

    names = check_direct(f"msbranches N{N} {H}x{W} ch{ch}", fwd, ref, [x], tensors, [gy, gres])
    reduces = [n for n in names if "reduce_kernel" in n]
    assert reduces == [f"{reduce_kernel}<{ch}>"] * 2, names


@pytest.mark.parametrize("N,H,W,ch,reduce_kernel", [(2, 21, 37, 16, "wgrad_msp_reduce_kernel"), (1, 32, 32, 32, "wgrad_msp_reduce_kernel"),
                                                    (2, 9, 20, 64, "wgrad_ms_reduce_kernel"), (2, 8, 12, 16, "wgrad_msp_reduce_kernel")])
def test_ms_branches_direct_grads(N, H, W, ch, reduce_kernel):
    """All eight parameter gradients of the MultiScaleBlock's branches from the fused one-pass kernel; the last case has H < 16."""
    _ms_branches(N, H, W, ch, reduce_kernel)


def test_ms_branches_direct_grads_unpacked_reduce(setenv_refresh):
    setenv_refresh.set("MSTG_MS_WGRAD_PACKED", "0")
    _ms_branches(2, 21, 37, 16, "wgrad_ms_reduce_kernel")


@pytest.mark.parametrize("N,H,W,Ci,Co,cfg", [(3, 16, 16, 16, 16, (1, 1, 0, 1)), (2, 32, 32, 32, 32, (1, 1, 0, 1)), (2, 64, 64, 16, 32, (4, 2, 1, 1))])
def test_ms_fusion_direct_grads(N, H, W, Ci, Co, cfg):
    """conv(ReLU(InstanceNorm(cat))) with the norm applied while the convolution and its weight gradient stage their tiles: the 1x1
    fusion layer, and the same fold for the stem's norm in front of the first 4x4 stride-2 convolution."""
    from mstg_hip import ops
    k, stride, pad, dil = cfg
    assert ops.ms_fusion_supported(N, H, W, Ci) if k == 1 else ops.norm_conv_supported(N, H, W, Ci, Co, k, stride, pad, dil)
    cat = rnd((N, H, W, Ci), 31, 1.7) - 0.2
    w, b = rnd((Co, Ci, k, k), 32, (Ci * k * k) ** -0.5), rnd((Co,), 33, 0.3)
    Ho, Wo = ops.conv_out_hw(H, W, k, stride, pad, dil, False)
    gy = rnd((N, Ho, Wo, Co), 34)

    def fwd(c_, w_, b_):
        return [ops.MSFusionFn.apply(c_, w_, b_, cfg)[0]]

    def ref(c_, w_, b_):
        z = F.relu(F.instance_norm(c_.permute(0, 3, 1, 2), eps=1e-5))
        return [F.conv2d(z, w_, b_, stride=stride, padding=pad, dilation=dil).permute(0, 2, 3, 1)]

    names = check_direct(f"ms fusion N{N} {H}x{W} {Ci}->{Co} k{k}", fwd, ref, [cat], [w, b], [gy])
    assert names.count("wgrad_reduce_kernel") == 2, names


# ----------------------------------------------------------------------------------------------------------
# NormLocalAttentionFn / LayerNormModFn
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn,N,H,W", [(16, 3, 16, 24), (64, 2, 24, 16)])
def test_norm_local_attention_direct_grads(Cn, N, H, W):
    from mstg_hip import ops
    from oracle import restatement as R
    assert ops.fused_attention_supported(Cn)
    x = rnd((N, H, W, Cn), 1, 2.0) + 0.5
    tensors = [rnd((3 * Cn, Cn, 1, 1), 2, Cn ** -0.5), rnd((3 * Cn,), 3, 0.1), rnd((Cn, Cn, 1, 1), 4, Cn ** -0.5), rnd((Cn,), 5, 0.1)]
    gy = rnd((N, H, W, Cn), 6)

    def fwd(x_, *ps):
        return [ops.NormLocalAttentionFn.apply(x_, *ps)]

    def ref(x_, wqkv, bqkv, wp, bp):
        sd = {"a.qkv.weight": wqkv, "a.qkv.bias": bqkv, "a.proj.weight": wp, "a.proj.bias": bp}
        return [R.local_attention(F.relu(R.instance_norm(x_.permute(0, 3, 1, 2))), sd, "a").permute(0, 2, 3, 1)]

    check_direct(f"norm+attention C{Cn} N{N} {H}x{W}", fwd, ref, [x], tensors, [gy])


@pytest.mark.parametrize("N,L,dim,mod", [(2, 64, 32, True), (1, 1100, 96, False)])
def test_layer_norm_mod_direct_grads(N, L, dim, mod):
    """dgamma and dbeta in place (ln_mod_reduce_kernel's accumulate); the second case has three token chunks and a 64-channel chunk
    half filled."""
    from mstg_hip import ops
    x = rnd((N, L, dim), 1, 2.0) + 0.3
    xs = [x] + ([rnd((N, dim), 4, 0.2), rnd((N, dim), 5, 0.2)] if mod else [])
    tensors = [1 + rnd((dim,), 2, 0.1), rnd((dim,), 3, 0.1)]
    gy = rnd((N, L, dim), 6)

    def fwd(x_, *rest):
        gm, bm = rest[:2] if mod else (None, None)
        return [ops.layer_norm_mod(x_, rest[-2], rest[-1], gm, bm)]

    def ref(x_, *rest):
        y = F.layer_norm(x_, (dim,), rest[-2], rest[-1], 1e-5)
        return [y * (1 + rest[0][:, None]) + rest[1][:, None] if mod else y]

    names = check_direct(f"ln_mod N{N} L{L} dim{dim}", fwd, ref, xs, tensors, [gy])
    assert names.count("ln_mod_reduce_kernel") == 2, names
