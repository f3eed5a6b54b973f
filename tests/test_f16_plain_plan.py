"""CPU: the fp16 inference planner of the plain CycleGAN Generator (csrc/infer_f16_plain.hip, mstg_hip/infer_plain.py) accepts the
eight layers of Generator(8 / 16 / 32 / 64), refuses what no kernel serves, and the BatchNorm fold is the arithmetic of
F.batch_norm in eval mode.  No kernel is launched here."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


def layers_of(Cw):
    """(kind, Cin, Cout, src_nchw_f32, dst_nchw) of Generator(Cw): encoder.0/2/5/8, decoder.0/3/6/9"""
    return [(0, 3, Cw, 1, 0), (0, Cw, 2 * Cw, 0, 0), (0, 2 * Cw, 4 * Cw, 0, 0), (0, 4 * Cw, 8 * Cw, 0, 0),
            (1, 8 * Cw, 4 * Cw, 0, 0), (1, 4 * Cw, 2 * Cw, 0, 0), (1, 2 * Cw, Cw, 0, 0), (1, Cw, 3, 0, 1)]


@pytest.mark.parametrize("Cw", [8, 16, 32, 64])
def test_every_layer_has_a_plan(lib, Cw):
    from mstg_hip.infer_plain import plain_desc
    for kind, Cin, Cout, stem, head in layers_of(Cw):
        d = plain_desc(kind, 2, 32, 48, Cin, Cout, 4, stem, head)
        n = lib.mstg_f16_plain_plan_bytes(C.byref(d))
        assert n > 0, (kind, Cin, Cout, lib.mstg_last_error().decode())
        assert n >= 2 * Cout * 4 + Cin * Cout * 16 * 2  # scale + shift in fp32, every filter element in fp16


def test_other_multiples_of_eight_have_a_plan(lib):
    from mstg_hip.infer_plain import plain_desc
    for kind, Cin, Cout in ((0, 24, 48), (1, 48, 24), (0, 512, 512), (1, 512, 512)):
        assert lib.mstg_f16_plain_plan_bytes(C.byref(plain_desc(kind, 1, 16, 16, Cin, Cout))) > 0


@pytest.mark.parametrize("args,what", [
    (dict(kind=0, Cin=64, Cout=64, K=3), b"K must be 4"),
    (dict(kind=1, Cin=64, Cout=64, K=2), b"K must be 4"),
    (dict(kind=0, Cin=520, Cout=64), b"512"),
    (dict(kind=0, Cin=1024, Cout=64), b"512"),
    (dict(kind=1, Cin=64, Cout=1024), b"512"),
    (dict(kind=0, Cin=12, Cout=64), b"multiple of 8"),
    (dict(kind=1, Cin=20, Cout=64), b"multiple of 8"),
    (dict(kind=0, Cin=3, Cout=64), b"multiple of 8"),                      # 3 channels, but not declared as the fp32 stem
    (dict(kind=1, Cin=3, Cout=64, src_nchw_f32=1), b"stem"),               # the stem is a Conv2d
    (dict(kind=0, Cin=4, Cout=64, src_nchw_f32=1), b"stem"),
    (dict(kind=0, Cin=64, Cout=12), b"multiple of 8"),
    (dict(kind=1, Cin=64, Cout=8, dst_nchw=1), b"head"),
    (dict(kind=2, Cin=64, Cout=64), b"kind"),
])
def test_unsupported_layers_refused_with_a_message(lib, args, what):
    from mstg_hip.infer_plain import plain_desc
    kw = dict(N=1, H=16, W=16)
    kw.update(args)
    d = plain_desc(**kw)
    assert lib.mstg_f16_plain_plan_bytes(C.byref(d)) == 0
    assert what in lib.mstg_last_error(), lib.mstg_last_error()


def test_host_side_validation(lib):
    from mstg_hip.infer_plain import plain_desc
    d = plain_desc(0, 1, 16, 16, 64, 64)
    assert lib.mstg_f16_plain_fwd(C.byref(d), None, None, None, None) == -1      # null pointers
    assert lib.mstg_f16_plain_pack(C.byref(d), None, None, None, None, 0, None) == -1
    assert lib.mstg_f16_plain_pack(C.byref(d), 1, None, None, 1, 16, None) == -1  # blob too small
    assert b"blob" in lib.mstg_last_error()
    d = plain_desc(0, 1, 15, 16, 64, 64)
    assert lib.mstg_f16_plain_fwd(C.byref(d), 1, 1, 1, None) == -1
    assert b"even" in lib.mstg_last_error()
    d = plain_desc(1, 1, 16, 16, 64, 64)
    d.Ho = 16
    assert lib.mstg_f16_plain_fwd(C.byref(d), 1, 1, 1, None) == -1
    assert b"Ho" in lib.mstg_last_error()
    d = plain_desc(0, 1, 16, 16, 1024, 64)
    assert lib.mstg_f16_plain_fwd(C.byref(d), 1, 1, 1, None) == -5


ACTS = {"none": lambda t: t, "leaky": lambda t: F.leaky_relu(t, 0.2), "relu": F.relu, "tanh": torch.tanh}


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("act", sorted(ACTS))
def test_fold_batchnorm_is_eval_batchnorm(transposed, act):
    """act(conv_nobias(x) * scale + shift) == act(F.batch_norm(conv(x) + bias, training=False)) to 1e-5 relative L2 in fp32, with
    gamma of either sign and exactly zero, and running_var over more than two decades."""
    from mstg_hip.infer_plain import fold_batchnorm
    g = torch.Generator().manual_seed(7 + transposed)
    Cin, Cout, eps = 16, 24, 1e-5
    x = torch.randn((3, Cin, 12, 10), generator=g)
    w = torch.randn((Cin, Cout, 4, 4) if transposed else (Cout, Cin, 4, 4), generator=g) * (2.0 / (Cin * 16)) ** 0.5
    b = torch.randn((Cout,), generator=g) * 0.3
    gamma = torch.randn((Cout,), generator=g)
    gamma[::7] = 0.0
    assert (gamma > 0).any() and (gamma < 0).any() and (gamma == 0).any()
    beta = torch.randn((Cout,), generator=g) * 0.5
    mean = torch.randn((Cout,), generator=g)
    var = torch.exp(torch.empty(Cout).uniform_(-3.0, 3.0, generator=g))
    conv = (lambda t, bias: F.conv_transpose2d(t, w, bias, 2, 1)) if transposed else (lambda t, bias: F.conv2d(t, w, bias, 2, 1))
    ref = ACTS[act](F.batch_norm(conv(x, b), mean, var, gamma, beta, training=False, eps=eps))
    scale, shift = fold_batchnorm(b, gamma, beta, mean, var, eps)
    assert scale.dtype == shift.dtype == torch.float32 and scale.shape == shift.shape == (Cout,)
    got = ACTS[act](conv(x, None) * scale[None, :, None, None] + shift[None, :, None, None])
    err = rel_l2(got, ref)
    print(f"  [fold] transposed={transposed} act={act}: rel-L2 {err:.2e}")
    assert err <= 1e-5
    # a convolution without a bias folds like a zero bias
    s0, h0 = fold_batchnorm(None, gamma, beta, mean, var, eps)
    assert torch.equal(s0, scale) and rel_l2(h0, beta - mean * scale) <= 1e-6


def test_generator_has_the_inference_methods():
    import plain_generator
    g = plain_generator.Generator(channels=8)
    assert callable(g.half_inference) and callable(g.graph_inference)
    assert g.half_inference() is g and g.graph_inference() is g
    assert g.half_inference(False) is g and g.graph_inference(False) is g
    for Cw in (8, 16, 32, 64, 24):
        plain_generator.Generator(channels=Cw).half_inference()


@pytest.mark.parametrize("Cw", [12, 128, 4, 72])
def test_unserved_widths_raise_at_call_time(Cw):
    import plain_generator
    g = plain_generator.Generator(channels=Cw)
    with pytest.raises(RuntimeError, match="channels"):
        g.half_inference()
    assert not getattr(g, "_half_enabled", False)
    g.half_inference(False)  # switching it off is always possible


def test_half_inference_has_no_cpu_path():
    import plain_generator
    g = plain_generator.Generator(channels=8).half_inference().eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        g(torch.zeros(1, 3, 16, 16))
