"""Grouped discriminator passes: G forwards of one layer / one EnhancedDiscriminator as one launch chain must be BITWISE the G
separate calls they stand for (torch.equal everywhere: the grouped launches replicate the single-group plan, no summation order
changes).  Outputs and workspaces sit between red zones, workspaces are handed out at exactly the queried size
(guard_helpers.memory_contract)."""
import ctypes

import pytest
import torch

from guard_helpers import memory_contract

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()  # raises if the HIP library is missing -- there is no fallback to test instead


def _rand(shape, gen, scale=1.0):
    return ((torch.rand(shape, generator=gen) * 2 - 1) * scale).to(DEV)


def d_layers(C):
    """(name, Cin, Cout, k, stride, pad, x_nchw, act) of EnhancedDiscriminator(channels=C), in forward order"""
    from mstg_hip.ops import ACT_LEAKY02, ACT_NONE
    return [("3->C nchw-in leaky", 3, C, 4, 2, 1, 1, ACT_LEAKY02), ("C->2C", C, 2 * C, 4, 2, 1, 0, ACT_NONE),
            ("2C->4C", 2 * C, 4 * C, 4, 2, 1, 0, ACT_NONE), ("4C->8C", 4 * C, 8 * C, 4, 2, 1, 0, ACT_NONE),
            ("8C->8C k3", 8 * C, 8 * C, 3, 1, 1, 0, ACT_NONE), ("8C->1 k4s1", 8 * C, 1, 4, 1, 1, 0, ACT_NONE)]


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("HW", [(64, 64), (64, 96)])
@pytest.mark.parametrize("C", [8, 16])
def test_grouped_layers_equal_separate_calls(C, HW, N, G):
    """Every layer shape of the discriminator, forward and input gradient (the image-side one included), grouped against G calls of
    mstg_conv2d_fwd / _dgrad with the same filters.  Group 1's filter is all zeros in every layer: a launch that read another
    group's filter (or wrote another group's output) cannot pass.  Every one of these layers must take the grouped route."""
    from mstg_hip import _lib, ops
    lib = _lib.load()
    gen = torch.Generator().manual_seed(100 * C + 10 * N + G + HW[1])
    H, W = HW
    with memory_contract() as mc:
        for name, Cin, Cout, k, s, p, x_nchw, act in d_layers(C):
            Ho, Wo = ops.conv_out_hw(H, W, k, s, p, 1, False)
            d = ops.make_desc(N, H, W, Cin, Ho, Wo, Cout, k, s, p, 1, 0, x_nchw, 0, act=act)
            # the input gradient's descriptor carries no activation: ConvFn.backward applies its derivative first
            db = ops.make_desc(N, H, W, Cin, Ho, Wo, Cout, k, s, p, 1, 0, x_nchw, 0)
            assert lib.mstg_conv2d_grouped_kernel_name(ctypes.byref(d), 0), (name, "forward is not on a grouped route")
            assert lib.mstg_conv2d_grouped_kernel_name(ctypes.byref(db), 1), (name, "input gradient is not on a grouped route")
            ws_ = [_rand((Cout, Cin, k, k), gen, 0.2) for _ in range(G)]
            ws_[1] = torch.zeros((Cout, Cin, k, k), device=DEV)
            bias = _rand((Cout,), gen, 0.5)
            if x_nchw:  # the first layer reads separate image tensors
                xs = [_rand((N, Cin, H, W), gen) for _ in range(G)]
            else:       # inner layers read one batched buffer
                xb = _rand((G * N, H, W, Cin), gen)
                xs = [xb[g * N:(g + 1) * N] for g in range(G)]
            y = torch.empty((G * N, Ho, Wo, Cout), dtype=torch.float32, device=DEV)
            y_ref = torch.empty((G * N, Ho, Wo, Cout), dtype=torch.float32, device=DEV)
            ys = [y[g * N:(g + 1) * N] for g in range(G)]
            ops._conv_grouped(0, d, xs, ws_, [bias] * G, ys)
            for g in range(G):
                ops.conv_fwd_raw(d, xs[g], ws_[g], bias, y_ref[g * N:(g + 1) * N])
            assert torch.equal(y, y_ref), (name, "forward")
            assert not torch.equal(y[:N], y[N:2 * N])  # the zero filter's group differs from its neighbour: the groups are not one copy
            dyb = _rand((G * N, Ho, Wo, Cout), gen)
            dys = [dyb[g * N:(g + 1) * N] for g in range(G)]
            dxs = [torch.empty_like(x) for x in xs]
            dxr = [torch.empty_like(x) for x in xs]
            ops._conv_grouped(1, db, dys, ws_, None, dxs)
            for g in range(G):
                ops.conv_dgrad_raw(db, dys[g], ws_[g], dxr[g])
            for g in range(G):
                assert torch.equal(dxs[g], dxr[g]), (name, "dgrad", g)
            assert float(dxs[1].abs().max()) == 0.0, (name, "zero filter, non-zero input gradient")
            if s == 2:
                H, W = Ho, Wo
        assert mc.workspaces > 0 and mc.outputs > 0


def _norm_split(lib, N, plan_N, HW, C):
    """rows per image of the plan, from the workspace query: N * (split + 1) rows of 2 C floats"""
    nbytes = lib.mstg_norm_workspace_bytes_plan(N, plan_N, HW, C)
    assert nbytes % (8 * N * C) == 0
    return nbytes // (8 * N * C) - 1


# (plan_N, G, H, W, C, split of the plan, split a plain call on G * plan_N images would take)
NORM_CASES = [(1, 3, 64, 64, 16, 16, 16),     # the tail-layer shape at batch 1
              (32, 2, 96, 96, 4, 32, 16),     # split <= 32: every apply workgroup re-adds the rows; the batched plan would differ
              (8, 3, 128, 128, 8, 64, 42)]    # split > 32: norm_stats_kernel / norm_sums_kernel; the batched plan would differ


@pytest.mark.parametrize("plan_N,G,H,W,C,split,split_all", NORM_CASES)
def test_norm_plan_entries_equal_per_group_calls(plan_N, G, H, W, C, split, split_all):
    from mstg_hip import _lib, ops
    lib = _lib.load()
    N = G * plan_N
    assert _norm_split(lib, N, plan_N, H * W, C) == split == _norm_split(lib, plan_N, plan_N, H * W, C)
    assert _norm_split(lib, N, N, H * W, C) == split_all
    assert lib.mstg_norm_workspace_bytes_plan(plan_N, plan_N, H * W, C) == lib.mstg_norm_workspace_bytes(plan_N, H * W, C)
    gen = torch.Generator().manual_seed(7 + plan_N)
    with memory_contract() as mc:
        x = _rand((N, H, W, C), gen) + 0.3
        dy = _rand((N, H, W, C), gen)
        y, stats = ops.norm_fwd_plan_raw(x, ops.ACT_LEAKY02, plan_N)
        dx = torch.empty_like(x)
        ops.norm_bwd_plan_raw(x, stats, dy, dx, ops.ACT_LEAKY02, plan_N)
        for g in range(G):
            sl = slice(g * plan_N, (g + 1) * plan_N)
            xg = x[sl].clone().requires_grad_(True)
            yg = ops.instnorm_act(xg, ops.ACT_LEAKY02)
            yg.backward(dy[sl])
            assert torch.equal(yg.detach(), y[sl]), ("forward", g)
            assert torch.equal(xg.grad, dx[sl]), ("backward", g)
        assert mc.workspaces >= 2 + 2 * G


def _two_discriminators(C, seed):
    import enhanced_generator as eg
    torch.manual_seed(seed)
    a = eg.EnhancedDiscriminator(channels=C).to(DEV)
    b = eg.EnhancedDiscriminator(channels=C).to(DEV)
    b.load_state_dict(a.state_dict())
    with torch.no_grad():  # biases start at zero: give them values, or a swapped bias would go unseen
        for (pa, pb) in zip(a.parameters(), b.parameters()):
            if pa.dim() == 1:
                pa.uniform_(-0.3, 0.3)
                pb.copy_(pa)
    return a, b


def _assert_same_state(a, b):
    for ma, mb in zip(a._sn_convs(), b._sn_convs()):
        assert torch.equal(ma.weight_u, mb.weight_u) and torch.equal(ma.weight_v, mb.weight_v)
        assert torch.equal(ma.weight, mb.weight)  # the filter set of the last forward


def test_forward_grouped_generator_phase_equals_sequence():
    """[fake with grad, real under no_grad, fake with grad] with frozen weights, as the generator phase runs it: scores, structure
    maps, u / v of all seven convolutions and the fake image's gradient."""
    from mstg_hip import ops
    Dg, Ds = _two_discriminators(8, 21)
    for D in (Dg, Ds):
        for p in D.parameters():
            p.requires_grad_(False)
    gen = torch.Generator().manual_seed(22)
    real = _rand((2, 3, 64, 64), gen)
    fake_g = _rand((2, 3, 64, 64), gen).requires_grad_(True)
    fake_s = fake_g.detach().clone().requires_grad_(True)
    assert Dg.can_group((fake_g, real, fake_g))
    with memory_contract(check_inputs=False):  # the power iterations write u and v in place
        (_, st3), (sc1, _), (_, st2) = Dg.forward_grouped((fake_g, fake_g, real), needs_grad=(True, True, False), sets=(2, 0, 1))
        assert not st2.requires_grad
        (ops.mse_to_const(sc1, 1.0) + 0.5 * ops.l1_loss(st2, st3)).backward()
    r1, _ = Ds(fake_s)
    with torch.no_grad():
        _, r2 = Ds(real)
    _, r3 = Ds(fake_s)
    (ops.mse_to_const(r1, 1.0) + 0.5 * ops.l1_loss(r2, r3)).backward()
    assert torch.equal(sc1, r1) and torch.equal(st2, r2) and torch.equal(st3, r3)
    assert sc1.shape == r1.shape and st3.shape == r3.shape
    _assert_same_state(Dg, Ds)
    assert torch.equal(fake_g.grad, fake_s.grad)


def test_forward_grouped_discriminator_phase_equals_sequence():
    """Two groups whose weights take gradients (the discriminator phase), group 0 with both heads in the loss and group 1 with the
    score alone: outputs, u / v, the input gradient and every parameter gradient."""
    from mstg_hip import ops
    Dg, Ds = _two_discriminators(8, 31)
    gen = torch.Generator().manual_seed(32)
    xa_g = _rand((3, 3, 64, 96), gen).requires_grad_(True)
    xb = _rand((3, 3, 64, 96), gen)
    xa_s = xa_g.detach().clone().requires_grad_(True)
    tgt = None

    def loss(sa, ta, sb):
        return ops.mse_to_const(sa, 1.0) + ops.l1_loss(ta, tgt) + ops.mse_to_const(sb, 0.0)

    with memory_contract(check_inputs=False):
        (sa, ta), (sb, tb) = Dg.forward_grouped((xa_g, xb))
        tgt = torch.zeros_like(ta.detach())
        loss(sa, ta, sb).backward()
    ra, rta = Ds(xa_s)
    rb, rtb = Ds(xb)
    loss(ra, rta, rb).backward()
    assert torch.equal(sa, ra) and torch.equal(sb, rb) and torch.equal(ta, rta) and torch.equal(tb, rtb)
    _assert_same_state(Dg, Ds)
    assert torch.equal(xa_g.grad, xa_s.grad)
    for (n, pg), (_, ps) in zip(Dg.named_parameters(), Ds.named_parameters()):
        assert pg.grad is not None and ps.grad is not None, n
        assert torch.equal(pg.grad, ps.grad), n


def test_forward_grouped_runs_the_sequence_where_it_cannot_group(monkeypatch):
    """eval mode, MSTG_D_GROUPED=0 and unequal shapes take the sequential forwards (and say so through can_group)."""
    Dg, Ds = _two_discriminators(8, 41)
    gen = torch.Generator().manual_seed(42)
    a, b = _rand((1, 3, 64, 64), gen), _rand((1, 3, 64, 64), gen)
    assert Dg.can_group((a, b)) and not Dg.can_group((a, _rand((1, 3, 64, 96), gen))) and not Dg.can_group((a,))
    monkeypatch.setenv("MSTG_D_GROUPED", "0")
    assert not Dg.can_group((a, b))
    out = Dg.forward_grouped((a, b))
    ref = [Ds(a), Ds(b)]
    for (s, t), (rs, rt) in zip(out, ref):
        assert torch.equal(s, rs) and torch.equal(t, rt)
    _assert_same_state(Dg, Ds)
    monkeypatch.delenv("MSTG_D_GROUPED")
    Dg.eval()
    assert not Dg.can_group((a, b))


def _three_steps(grouped, streams, monkeypatch):
    import enhanced_train
    monkeypatch.setenv("MSTG_D_GROUPED", "1" if grouped else "0")
    torch.manual_seed(3)
    m = enhanced_train.EnhancedCycleGAN(channels=16, num_transformer_blocks=0, device=torch.device(DEV))
    m.two_streams = streams
    g = torch.Generator().manual_seed(5)
    a = (torch.rand((4, 3, 64, 64), generator=g) * 2 - 1).to(DEV)
    b = (torch.rand((4, 3, 64, 64), generator=g) * 2 - 1).to(DEV)
    losses = torch.stack([m.train_step_async(a, b) for _ in range(3)])
    return losses, m.g_optimizer.flat.clone(), m.d_optimizer.flat.clone()


def test_train_step_grouped_is_bit_identical(monkeypatch):
    """Three steps of the CycleGAN with MSTG_D_GROUPED=0 and 1, on two streams and on one: losses and both optimizers' flat buffers."""
    ref = _three_steps(False, True, monkeypatch)
    for grouped, streams in ((True, True), (True, False)):
        got = _three_steps(grouped, streams, monkeypatch)
        for name, x, y in zip(("losses", "generator parameters", "discriminator parameters"), got, ref):
            assert torch.equal(x, y), (grouped, streams, name)
