"""The small kernels under the train step (csrc/elementwise.hip, the step bookkeeping of csrc/train_f16_plain.hip): per-channel sums,
the global average pool, mean losses, gradient clipping, activations, the loss combination and Adam.

Exact tests: a kernel that only ADDS is fed small integers stored as fp32.  Every partial sum is then an integer below 2**24 and
exact in fp32 whatever the order of the additions, so the result must equal the int64 sum bit for bit: one dropped, doubled or
misaddressed element fails.  Each such test first asserts that precondition (sum |x| < 2**24 per output) on the CPU.  Where a
kernel multiplies the sum once (1 / n, a gradient scale) the expected value is that single fp32 operation reproduced in numpy.

Yardstick tests (Adam): the bar is four times the distance of torch's own fp32 evaluation on the CPU from the fp64 reference on
the same draw, the margin tests/test_gpu_transformer.py::test_generator_with_block_vs_oracle gives one fp32 evaluation over another.
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TWO24 = 2 ** 24
BIG = 2 * 524288 + 5  # the grid is capped at 2048 x 256 threads: the grid-stride loop of the scalar kernels goes round three times


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()  # raises if the HIP library is missing -- there is no fallback to test instead


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def ints(shape, seed, lo, hi):
    """Integers lo..hi (inclusive) stored as fp32."""
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def report(name, err, tol):
    print(f"  [parity] {name:60s} rel-L2 {err:.2e} (tol {tol:.0e})")
    assert err <= tol, f"{name}: {err:.3e} > {tol:.0e}"


def launched(fn):
    """(fn(), [symbol of every kernel the library launched meanwhile]) from the library's own per-launch profiler."""
    from mstg_hip import ops
    ops.KernelTimer.start()
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [nm for nm, _ in ops.KernelTimer.kernels()]
    finally:
        ops.KernelTimer.stop()
    return out, names


def ulps(a, b):
    """Largest distance in units in the last place between two fp32 tensors (CPU), 0 for +0 against -0."""
    def key(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max())


# ----------------------------------------------------------------------------------------------------------
# ops.channel_sum / ops.plane_sum_nchw / ops.spatial_mean
# ----------------------------------------------------------------------------------------------------------
VEC, SCALAR = "channel_sum_partial_v4_kernel", "channel_sum_partial_kernel"

# (P, ctot, coff, C, scale, floats into the buffer at which the view starts, kernel)
CHANNEL_SUM_CASES = [
    (1, 4, 0, 4, 1.0, 0, VEC),
    (3, 64, 16, 32, 1.0, 0, VEC),        # fewer pixels than thread rows
    (1000, 64, 16, 32, 1.0, 0, VEC),
    (1000, 64, 16, 32, 0.25, 0, VEC),
    (5000, 48, 16, 16, 1.0, 0, VEC),
    (4097, 12, 0, 12, 1.0, 0, VEC),      # C / 4 = 3: the 256th thread has no row
    (1027, 260, 0, 260, 1.0, 0, VEC),    # C > 256: 1024 threads
    (2050, 1024, 0, 1024, 1.0, 0, VEC),
    (63, 64, 0, 64, 1.0, 0, VEC),        # rows = 256 / (C / 4) = 16: the 4x-unrolled loop takes 4 * rows pixels a trip;
    (64, 64, 0, 64, 1.0, 0, VEC),        # 4 * rows - 1, 4 * rows, 4 * rows + 1 pixels sit on its boundary with the remainder loop
    (65, 64, 0, 64, 1.0, 0, VEC),
    (500, 3, 0, 3, 1.0, 0, SCALAR),
    (777, 7, 2, 5, 1.0, 0, SCALAR),
    (1000, 32, 2, 16, 1.0, 0, SCALAR),   # misaligned channel offset
    (1000, 64, 16, 32, 1.0, 1, SCALAR),  # an aligned shape on a misaligned pointer
    (1500, 300, 0, 300, 1.0, 0, VEC),    # 300 = 4 * 75: a vector case, whatever its odd look
    (1500, 302, 1, 301, 1.0, 0, SCALAR), # C > 256 on the scalar kernel: 1024 threads, 3 rows
    (70000, 1, 0, 1, 1.0, 0, SCALAR),    # 69 workgroups
]


def _channel_sum(x, P, ctot, coff, C, scale, start, kernel):
    from mstg_hip import ops
    xg = x.to(DEV)[start:]
    assert (xg.data_ptr() % 16 == 0) == (start % 4 == 0)
    out, names = launched(lambda: ops.channel_sum(xg, P, ctot, coff, C, scale))
    assert kernel in names and ({VEC, SCALAR} - {kernel}).pop() not in names, names
    return out.cpu()


@pytest.mark.parametrize("P,ctot,coff,C,scale,start,kernel", CHANNEL_SUM_CASES)
def test_channel_sum_exact(P, ctot, coff, C, scale, start, kernel):
    x = ints((start + P * ctot,), 7 + P + C, -8, 8)
    sl = x[start:].view(P, ctot)[:, coff:coff + C].long()
    assert int(sl.abs().sum(0).max()) < TWO24
    out = _channel_sum(x, P, ctot, coff, C, scale, start, kernel)
    assert torch.equal(out.double(), sl.sum(0).double() * scale)  # scale is a power of two: exact


@pytest.mark.parametrize("P,ctot,coff,C,kernel", [(5000, 48, 16, 16, VEC), (777, 7, 2, 5, SCALAR)])
def test_channel_sum_floats(P, ctot, coff, C, kernel):
    x = rnd((P * ctot,), 11) + 0.5
    out = _channel_sum(x, P, ctot, coff, C, 1.0, 0, kernel)
    report(f"channel_sum {kernel} P{P}", rel_l2(out, x.view(P, ctot)[:, coff:coff + C].double().sum(0)), 1e-6)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 16, 16), (3, 3, 37, 53), (2, 5, 300, 300)])
def test_plane_sum_nchw_exact(shape):
    from mstg_hip import ops
    x = ints(shape, 13, -8, 8)
    assert int(x.long().abs().sum(dim=(0, 2, 3)).max()) < TWO24
    out = ops.plane_sum_nchw(x.to(DEV)).cpu()
    assert torch.equal(out.double(), x.long().sum(dim=(0, 2, 3)).double())


@pytest.mark.parametrize("shape", [(2, 1, 1, 3), (3, 64, 64, 1), (2, 16, 16, 100), (2, 8, 8, 256), (2, 8, 8, 300), (1, 4, 4, 1024)])
def test_spatial_mean_exact(shape):
    """H * W is a power of two: the scale 1 / P is exact, and so is the mean of integers."""
    from mstg_hip import ops
    N, H, W, Cn = shape
    P = H * W
    assert P & (P - 1) == 0
    x = ints(shape, 17, -8, 8)
    assert int(x.long().abs().sum(dim=(1, 2)).max()) < TWO24
    xg = x.to(DEV).requires_grad_(True)
    out = ops.spatial_mean(xg)
    assert torch.equal(out.detach().cpu().double(), x.long().sum(dim=(1, 2)).double() / P)
    # backward: dx[n, h, w, c] = dy[n, c] * float32(1 / float32(P)), one fp32 multiplication
    dy = rnd((N, Cn), 18)
    (dx,) = torch.autograd.grad((out * dy.to(DEV)).sum(), [xg])
    want = torch.from_numpy(dy.numpy() * (np.float32(1.0) / np.float32(P)))
    assert torch.equal(dx.cpu(), want[:, None, None, :].expand(N, H, W, Cn))


def test_spatial_mean_floats_odd_plane():
    from mstg_hip import ops
    x = rnd((3, 15, 15, 100), 19)
    xg = x.to(DEV).requires_grad_(True)
    out = ops.spatial_mean(xg)
    report("spatial mean 15x15 C=100", rel_l2(out, x.double().mean(dim=(1, 2))), 1e-6)
    dy = rnd((3, 100), 20)
    (dx,) = torch.autograd.grad((out * dy.to(DEV)).sum(), [xg])
    want = torch.from_numpy(dy.numpy() * (np.float32(1.0) / np.float32(225)))
    assert torch.equal(dx.cpu(), want[:, None, None, :].expand(3, 15, 15, 100))


# ----------------------------------------------------------------------------------------------------------
# mean losses and their gradients
# ----------------------------------------------------------------------------------------------------------
GOUT = 3.5  # the gradient arriving at the loss (exact in fp32)


def _mean32(S, n):
    """loss_final_kernel: float32(S) * float32(1 / float32(n))."""
    return np.float32(S) * (np.float32(1.0) / np.float32(n))


@pytest.mark.parametrize("n", [1, 2, 255, 257, BIG])
def test_mean_losses_exact(n):
    """l1 / mse / mse-to-constant / masked l1 on values in {-1, 0, 1}: the sum is an exact integer, the value is that integer times
    float32(1 / n), and the gradients are loss_bwd_kernel's / masked_l1_bwd_kernel's own fp32 expression (exact ties give 0, a
    masked-out element gets 0)."""
    from mstg_hip import ops
    a, b = ints((n,), 21 + n % 97, -1, 1), ints((n,), 22 + n % 97, -1, 1)
    m = ints((n,), 23 + n % 97, 0, 1)
    d = (a - b).numpy()
    assert (d == 0).any() or n < 3  # ties are in the draw
    gs = np.float32(GOUT) * np.float32(1.0) / np.float32(n)  # (g * scale) / n as loss_bwd_kernel rounds it
    ag, bg, mg = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True), m.to(DEV)
    # ---- L1
    S = int(np.abs(d).astype(np.int64).sum())
    assert 2 * n < TWO24
    loss = ops.l1_loss(ag, bg)
    assert np.float32(loss.item()) == _mean32(S, n), (loss.item(), S, n)
    da, db = torch.autograd.grad(loss * GOUT, [ag, bg])
    want = (np.sign(d) * gs).astype(np.float32)
    assert torch.equal(da.cpu(), torch.from_numpy(want)) and torch.equal(db.cpu(), torch.from_numpy(-want))
    assert bool((da.cpu()[torch.from_numpy(d == 0)] == 0).all())
    # ---- MSE
    S = int((d.astype(np.int64) ** 2).sum())
    assert 4 * n < TWO24
    loss = ops.mse_loss(ag, bg)
    assert np.float32(loss.item()) == _mean32(S, n), (loss.item(), S, n)
    da, db = torch.autograd.grad(loss * GOUT, [ag, bg])
    want = ((np.float32(2.0) * d) * gs).astype(np.float32)
    assert torch.equal(da.cpu(), torch.from_numpy(want)) and torch.equal(db.cpu(), torch.from_numpy(-want))
    # ---- MSE against a constant (the LSGAN targets)
    for target in (0.0, 1.0):
        dc = a.numpy() - np.float32(target)
        S = int((dc.astype(np.int64) ** 2).sum())
        loss = ops.mse_to_const(ag, target)
        assert np.float32(loss.item()) == _mean32(S, n), (loss.item(), S, n)
        (da,) = torch.autograd.grad(loss * GOUT, [ag])
        assert torch.equal(da.cpu(), torch.from_numpy(((np.float32(2.0) * dc) * gs).astype(np.float32)))
    # ---- masked L1: |a * (1 - m) - b * (1 - m)|, gradient to a only
    w = np.float32(1.0) - m.numpy()
    dm = a.numpy() * w - b.numpy() * w
    S = int(np.abs(dm).astype(np.int64).sum())
    loss = ops.masked_l1_loss(ag, bg, mg)
    assert np.float32(loss.item()) == _mean32(S, n), (loss.item(), S, n)
    (da,) = torch.autograd.grad(loss * GOUT, [ag])
    gm = np.float32(GOUT) / np.float32(n)
    want = ((np.sign(dm) * gm).astype(np.float32) * w).astype(np.float32)
    assert torch.equal(da.cpu(), torch.from_numpy(want))
    assert bool((da.cpu()[m == 1] == 0).all())


@pytest.mark.parametrize("n", [100003, BIG])
def test_clip_grad_norm_flat_integers(n):
    """Integer gradient: the sum of squares is exact, so the returned norm is one fp32 square root away from it (2 ulp), the scaled
    gradient two fp32 operations and one multiplication away from torch's formula (4 ulp); a max_norm above the norm leaves the
    buffer as it was, bit for bit.  (The MI355X run printed 0 ulp for the scaled gradient at both sizes.)"""
    from mstg_hip import ops
    g = ints((n,), 31, -2, 2)
    S = int((g.long() ** 2).sum())
    assert S < TWO24
    norm32 = np.sqrt(np.float32(S))
    for max_norm in (1.0, 1e6):
        assert (max_norm < norm32) == (max_norm == 1.0)
        gg = g.to(DEV)
        norm = ops.clip_grad_norm_flat_(gg, max_norm)
        got = np.float32(norm.item())
        assert ulps(torch.tensor([got]), torch.tensor([norm32])) <= 2, (got, norm32)
        if max_norm < norm32:
            coef = np.float32(max_norm) / (norm32 + np.float32(1e-6))
            assert coef < 1
            d = ulps(gg.cpu(), torch.from_numpy(g.numpy() * coef))
            print(f"  [parity] clip_grad_norm n={n}: scaled gradient within {d} ulp")
            assert d <= 4
        else:
            assert torch.equal(gg.cpu(), g)


# ----------------------------------------------------------------------------------------------------------
# mstg_act_fwd / mstg_act_bwd / mstg_add through the C ABI, on pointers into a larger buffer
# ----------------------------------------------------------------------------------------------------------
EW_SIZES = [1, 2, 3, 4, 5, 6, 7, 1023, 1024, 1025, 1026, 1027, 2097152 + 1203]  # every n & 3 tail; the last takes the float4 loop round twice
SENTINEL = 12345.0


def _out_buffer(n):
    return torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=DEV)


def _tail_untouched(buf, n):
    return bool((buf[n:] == SENTINEL).all())


@pytest.mark.parametrize("n", EW_SIZES)
def test_act_and_add_raw_tails(n):
    """ReLU, LeakyReLU(0.2) and add are single fp32 operations: bit for bit against torch on the CPU; tanh at 1e-6; the 8 floats
    behind the n-th stay as they were."""
    from mstg_hip import _lib, ops
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    x, dy = rnd((n + 8,), 41, 2.0), rnd((n + 8,), 42)
    x[: min(n, 3)] = torch.tensor([0.0, -0.0, 1.0])[: min(n, 3)]
    xg, dyg = x.to(DEV), dy.to(DEV)
    fwd = {ops.ACT_RELU: F.relu, ops.ACT_LEAKY02: lambda t: F.leaky_relu(t, 0.2)}
    for act in (ops.ACT_RELU, ops.ACT_LEAKY02, ops.ACT_TANH):
        y, dx = _out_buffer(n), _out_buffer(n)
        _lib.check(lib.mstg_act_fwd(xg.data_ptr(), y.data_ptr(), n, act, st), "mstg_act_fwd")
        src = y if act == ops.ACT_TANH else xg  # tanh's derivative is taken from the output
        _lib.check(lib.mstg_act_bwd(src.data_ptr(), dyg.data_ptr(), dx.data_ptr(), n, act, st), "mstg_act_bwd")
        assert _tail_untouched(y, n) and _tail_untouched(dx, n), act
        if act == ops.ACT_TANH:
            report(f"tanh n={n} y", rel_l2(y[:n], torch.tanh(x[:n].double())), 1e-6)
            report(f"tanh n={n} dx", rel_l2(dx[:n], dy[:n].double() * (1 - y[:n].cpu().double() ** 2)), 1e-6)
        else:
            xr = x[:n].clone().requires_grad_(True)
            yr = fwd[act](xr)
            (dxr,) = torch.autograd.grad((yr * dy[:n]).sum(), [xr])
            assert torch.equal(y[:n].cpu(), yr.detach()), act
            assert torch.equal(dx[:n].cpu(), dxr), act
    b = rnd((n + 8,), 43, 3.0)
    y = _out_buffer(n)
    _lib.check(lib.mstg_add(xg.data_ptr(), b.to(DEV).data_ptr(), y.data_ptr(), n, st), "mstg_add")
    assert _tail_untouched(y, n)
    assert torch.equal(y[:n].cpu(), x[:n] + b[:n])


# ----------------------------------------------------------------------------------------------------------
# ops.weighted_sum at its limits
# ----------------------------------------------------------------------------------------------------------
def test_weighted_sum_limits():
    from mstg_hip import ops
    vals = rnd((8,), 51, 3.0)
    W = rnd((6, 8), 52, 5.0)
    t = [v.clone().to(DEV).requires_grad_(True) for v in vals]
    total, parts = ops.weighted_sum(t, W[0].tolist(), report=[r.tolist() for r in W[1:]])
    ref = W.double() @ vals.double()
    report("weighted_sum 8 terms x 6 outputs", rel_l2(torch.cat([total.reshape(1), parts]), ref), 1e-6)
    assert parts.shape == (5,) and not parts.requires_grad
    (total * 3.0).backward()
    report("weighted_sum gradient of row 0", rel_l2(torch.stack([v.grad for v in t]), 3.0 * W[0].double()), 1e-6)
    nine = [torch.tensor(1.0, device=DEV) for _ in range(9)]
    with pytest.raises(RuntimeError, match="1..8 terms, 1..6 outputs"):
        ops.weighted_sum(nine, [1.0] * 9)
    with pytest.raises(RuntimeError, match="1..8 terms, 1..6 outputs"):
        ops.weighted_sum(nine[:8], [1.0] * 8, report=[[1.0] * 8] * 6)


# ----------------------------------------------------------------------------------------------------------
# Adam
# ----------------------------------------------------------------------------------------------------------
ADAM_N, LR, BETAS, EPS = 600001, 5e-5, (0.5, 0.999), 1e-8  # n > 2048 * 256: adam_kernel's loop goes round twice
ZEROS, TINY, HUGE, SMALL = (slice(1000 * k, 1000 * (k + 1)) for k in range(4))


def _adam_grads(step):
    g = torch.randn(ADAM_N, generator=torch.Generator().manual_seed(600 + step))
    g[ZEROS] = 0.0
    g[TINY] *= 1e-20
    g[HUGE] *= 1e4
    g[SMALL] *= 1e-6
    return g


@pytest.fixture(scope="module")
def adam_reference():
    """Five steps of torch.optim.Adam from p = m = v = 0 on the CPU, in fp64 and in fp32, on the same gradients."""
    out = {}
    for dtype in (torch.float64, torch.float32):
        p = torch.nn.Parameter(torch.zeros(ADAM_N, dtype=dtype))
        opt = torch.optim.Adam([p], lr=LR, betas=BETAS, eps=EPS)
        for step in range(5):
            p.grad = _adam_grads(step).to(dtype)
            opt.step()
        st = opt.state[p]
        out[dtype] = (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return out


def test_adam_step_flat_from_zero(adam_reference):
    """Five steps from p = m = v = 0, so that p IS the accumulated update (nothing hides behind a parameter of size 1).
    p: within 4x the distance of torch.optim.Adam in fp32 on the CPU from the fp64 run on the same draw (the margin
    test_generator_with_block_vs_oracle gives one fp32 evaluation over another; both figures are printed).
    exp_avg: 1e-6.  exp_avg_sq: 2e-5, derived, not tuned -- the ABI takes beta2 as a float, and 1 - float32(0.999) is 1.29e-5 short of
    0.001 (relative), which scales every (1 - beta2) * g^2 term of the fp32 kernel against the fp64 reference's.
    The MI355X run printed: torch fp32 at 7.96e-08 (so the bar for p was 3.2e-07), adam_kernel's p at 6.70e-08, exp_avg at 3.14e-08,
    exp_avg_sq at 1.28e-05; a misplaced eps sits at 4e-2."""
    from mstg_hip import ops
    p, m, v = (torch.zeros(ADAM_N, device=DEV) for _ in range(3))
    for step in range(5):
        ops.adam_step_flat(p, _adam_grads(step).to(DEV), m, v, LR, BETAS[0], BETAS[1], EPS, step + 1)
    p64, m64, v64 = adam_reference[torch.float64]
    d32 = rel_l2(adam_reference[torch.float32][0], p64)
    print(f"  [parity] torch.optim.Adam fp32 (CPU) vs fp64, accumulated update: {d32:.2e}")
    short = abs((1.0 - float(np.float32(0.999))) - 1e-3) / 1e-3
    assert 1.2e-5 < short < 1.4e-5  # the figure the exp_avg_sq bar is derived from
    report("adam accumulated update (5 steps from 0)", rel_l2(p, p64), 4.0 * d32)
    report("adam exp_avg", rel_l2(m, m64), 1e-6)
    report("adam exp_avg_sq", rel_l2(v, v64), 2e-5)
    for t in (p, m, v):  # a zero gradient leaves everything at exactly 0
        assert bool((t[ZEROS] == 0).all())
    assert bool(torch.isfinite(p).all())


def test_adam_step_flat_mask():
    """mask (uint8, about half ones): a masked-out element keeps p, m, v bit for bit; the others get the unmasked step."""
    from mstg_hip import ops
    p0, m0, v0 = rnd((ADAM_N,), 61), rnd((ADAM_N,), 62, 0.1), rnd((ADAM_N,), 63) ** 2
    mask = torch.randint(0, 2, (ADAM_N,), generator=torch.Generator().manual_seed(64), dtype=torch.uint8)
    assert 0.45 < float(mask.float().mean()) < 0.55
    runs = []
    for use_mask in (True, False):
        p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        for step in range(2):
            ops.adam_step_flat(p, _adam_grads(step).to(DEV), m, v, LR, BETAS[0], BETAS[1], EPS, step + 3,
                               mask=mask.to(DEV) if use_mask else None)
        runs.append((p.cpu(), m.cpu(), v.cpu()))
    on = mask.bool()
    for got, full, before in zip(runs[0], runs[1], (p0, m0, v0)):
        assert torch.equal(got[~on], before[~on])
        assert torch.equal(got[on], full[on])
        assert not torch.equal(full[~on], before[~on])  # the unmasked step did move them


def _flat_adam_pair(step_count):
    """Two FlatAdams over equal parameters, gradients and moments.  |p| >= 0.5: an update of ~lr that differs in its last bits
    then moves p by less than one ulp of p (no cancellation against a parameter near zero)."""
    from mstg_hip.optim import FlatAdam
    shapes = [(16, 3, 7, 7), (16,), (5, 3), (4097,)]
    opts = []
    for _ in range(2):
        ps = []
        for i, s in enumerate(shapes):
            r = rnd(s, 70 + i)
            ps.append(torch.nn.Parameter((torch.sign(r) * (0.5 + 0.5 * r.abs()) + (r == 0)).to(DEV)))
        opt = FlatAdam(ps, lr=LR, betas=BETAS)
        opt.grad.copy_(rnd((opt.numel,), 75).to(DEV))
        opt.exp_avg.copy_(rnd((opt.numel,), 76, 0.3).to(DEV))
        opt.exp_avg_sq.copy_((rnd((opt.numel,), 77) ** 2).to(DEV))
        opt.step_count = step_count
        opts.append(opt)
    return opts


def test_guarded_adam_step_vs_flat_adam():
    """train_adam_kernel at step_base 3 + 2 good steps on the device against FlatAdam.step() at step 5.  The two kernels share the
    update expression but take the bias corrections from pow() on the device and on the host, and the compiler may contract
    b2 * v + (1 - b2) * g * g differently in each: the project promises no bits here, so 4 ulp (with beta1 = 0.5 both products of
    exp_avg are exact; the MI355X run printed 0 ulp for all three).  With `last step ok` = 0 the step is a no-op, bit for bit."""
    from mstg_hip import train_plain
    guarded, plain = _flat_adam_pair(3)
    plain.step_count = 4
    plain.step()
    istate = torch.tensor([0, 2, 1], dtype=torch.int32, device=DEV)
    train_plain.guarded_adam_step(guarded, istate)
    assert istate.tolist() == [0, 2, 1]
    for name, a, b in (("p", guarded.flat, plain.flat), ("exp_avg", guarded.exp_avg, plain.exp_avg),
                       ("exp_avg_sq", guarded.exp_avg_sq, plain.exp_avg_sq)):
        d = ulps(a.cpu(), b.cpu())
        print(f"  [parity] guarded adam {name}: within {d} ulp of FlatAdam.step()")
        assert d <= 4, name
    skipped, untouched = _flat_adam_pair(3)
    assert not torch.equal(guarded.flat, untouched.flat)  # the good step did move the parameters
    train_plain.guarded_adam_step(skipped, torch.tensor([1, 2, 0], dtype=torch.int32, device=DEV))
    for a, b in ((skipped.flat, untouched.flat), (skipped.exp_avg, untouched.exp_avg), (skipped.exp_avg_sq, untouched.exp_avg_sq),
                 (skipped.grad, untouched.grad)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("norm", [1.0, 3.4e38, float("inf"), float("-inf"), float("nan")])
def test_scale_update(norm):
    """train_scale_update_kernel: a finite norm counts a good step and leaves the loss scale; a non-finite one counts a skipped
    step, halves the scale, doubles its reciprocal and clears `last step ok`."""
    import math
    from mstg_hip import train_plain
    fstate = torch.tensor([1024.0, 1.0 / 1024.0, 7.0], dtype=torch.float32, device=DEV)  # a third float that nobody may touch
    for last_ok in (0, 1):
        fstate[:2] = torch.tensor([1024.0, 1.0 / 1024.0])
        istate = torch.tensor([3, 7, last_ok], dtype=torch.int32, device=DEV)
        train_plain.scale_update(torch.tensor([norm], dtype=torch.float32, device=DEV), fstate, istate)
        if math.isfinite(norm):
            assert istate.tolist() == [3, 8, 1] and fstate.tolist() == [1024.0, 1.0 / 1024.0, 7.0]
        else:
            assert istate.tolist() == [4, 7, 0] and fstate.tolist() == [512.0, 1.0 / 512.0, 7.0]
