"""CPU: the mixed-precision multi-style loss (csrc/style_f16.hip, mstg_hip/style_f16.py, style_loss.py precision="mixed") plans and
routes every layer of the supported grid, refuses by name what no kernel serves, and the CPU emulation the GPU tests measure
against (tests/style_f16_ref.py) rounds like torch's casts and has the exact-zero property.  No kernel is launched here."""
import ctypes as C
import re

import pytest
import torch

import style_f16_ref as E

WIDTHS = (16, 32, 48, 64, 80, 128, 256, 512)


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


def expected_route(N, H, W, Cout, stem):
    """the rule csrc/style_f16.hip documents: 16 NT channels by width; 128-pixel tiles when they give 512 blocks"""
    NT = 4 if Cout > 32 else (2 if Cout > 16 else 1)
    ntn = -(-Cout // (16 * NT))
    M = N * H * W
    MT = 2 if -(-M // 128) * ntn >= 512 else 1
    return MT, NT, int(stem)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "bf16"])
def test_every_layer_of_the_grid_has_a_plan_and_a_route(lib, dtype):
    from mstg_hip.style_f16 import conv_desc, kernel_name
    tag = "bf16" if dtype else "f16"
    seen = set()
    for Cin in WIDTHS:
        for Cout in WIDTHS:
            n = lib.mstg_style16_conv_plan_bytes(C.byref(conv_desc(dtype, 1, 8, 8, Cin, Cout)))
            assert n >= Cout * 4 + 9 * Cin * Cout * 2, (Cin, Cout, lib.mstg_last_error().decode())
            for N, H, W in ((1, 1, 1), (2, 5, 7), (2, 32, 32), (4, 128, 128), (32, 512, 512)):
                name = kernel_name(conv_desc(dtype, N, H, W, Cin, Cout))
                MT, NT, stem = expected_route(N, H, W, Cout, False)
                assert name == f"style_conv16_kernel<{tag},{MT},{NT},{stem}>", (N, H, W, Cin, Cout, name)
                seen.add(name)
    for Cw in (16, 64, 512):  # the boundary forms
        stem, grad = conv_desc(dtype, 2, 16, 24, 3, Cw, stem=1), conv_desc(dtype, 2, 16, 24, Cw, 3, image_grad=1)
        assert lib.mstg_style16_conv_plan_bytes(C.byref(stem)) >= Cw * 4 + 9 * 4 * Cw * 2
        assert lib.mstg_style16_conv_plan_bytes(C.byref(grad)) >= 16 * 4 + 9 * Cw * 16 * 2
        assert re.fullmatch(rf"style_conv16_kernel<{tag},[12],[124],1>", kernel_name(stem))
        assert re.fullmatch(rf"style_conv16_kernel<{tag},[12],1,0>", kernel_name(grad))
    assert len(seen) == 6, seen  # both pixel tiles x three channel tiles are reached


def test_the_full_width_stack_is_served(lib):
    """VGG16 up to relu4_3 at 32 x 512 x 512: every forward layer and every input gradient has a plan and takes 128-pixel tiles"""
    from mstg_hip.style_f16 import conv_desc, kernel_name
    cin, hw = 3, 512
    for c in E.R.VGG_CFG:
        if c == "M":
            hw //= 2
            continue
        fwd = conv_desc(0, 32, hw, hw, cin, c, stem=int(cin == 3), relu=1)
        bwd = conv_desc(1, 32, hw, hw, c, cin, image_grad=int(cin == 3), flip=1)
        for d in (fwd, bwd):
            assert lib.mstg_style16_conv_plan_bytes(C.byref(d)) > 0, lib.mstg_last_error().decode()
            assert ",2," in kernel_name(d)
        cin = c


@pytest.mark.parametrize("kw,what", [
    (dict(Cin=24, Cout=64), b"Cin must be a multiple of 16"),
    (dict(Cin=8, Cout=64), b"Cin must be a multiple of 16"),
    (dict(Cin=528, Cout=64), b"Cin must be a multiple of 16 up to 512"),
    (dict(Cin=64, Cout=40), b"Cout must be a multiple of 16"),
    (dict(Cin=64, Cout=1024), b"Cout must be a multiple of 16 up to 512"),
    (dict(Cin=3, Cout=64), b"Cin must be a multiple of 16"),        # 3 channels, but not declared as the fp32 stem
    (dict(Cin=4, Cout=64, stem=1), b"stem"),
    (dict(Cin=64, Cout=3), b"Cout must be a multiple of 16"),       # 3 channels, but not declared as the image gradient
    (dict(Cin=64, Cout=4, image_grad=1), b"image gradient"),
    (dict(Cin=3, Cout=3, stem=1, image_grad=1), b"different layers"),
    (dict(Cin=64, Cout=64, dtype=2), b"dtype"),
])
def test_unsupported_layers_are_refused_by_name(lib, kw, what):
    from mstg_hip.style_f16 import conv_desc
    args = dict(dtype=0, N=1, H=8, W=8)
    args.update(kw)
    d = conv_desc(**args)
    assert lib.mstg_style16_conv_plan_bytes(C.byref(d)) == 0
    assert what in lib.mstg_last_error(), lib.mstg_last_error()
    assert lib.mstg_style16_conv_kernel_name(C.byref(d)) is None
    assert lib.mstg_style16_conv_fwd(C.byref(d), 1, 1, None, 1, None) == -5
    assert lib.mstg_style16_conv_pack(C.byref(d), 1, None, 1, 1 << 30, None) == -5


def test_host_side_validation(lib):
    from mstg_hip.style_f16 import conv_desc
    d = conv_desc(0, 1, 8, 8, 64, 64)
    assert lib.mstg_style16_conv_fwd(C.byref(d), None, None, None, None, None) == -1
    assert lib.mstg_style16_conv_pack(C.byref(d), 1, None, 1, 16, None) == -1 and b"blob" in lib.mstg_last_error()
    assert lib.mstg_style16_conv_fwd(C.byref(conv_desc(0, 0, 8, 8, 64, 64)), 1, 1, None, 1, None) == -1
    assert lib.mstg_style16_conv_fwd(C.byref(conv_desc(1, 1, 8, 8, 64, 3, image_grad=1)), 1, 1, 1, 1, None) == -1
    assert b"mask" in lib.mstg_last_error()
    assert lib.mstg_style16_maxpool_fwd(1, 1, 1, 1, 7, 8, 16, None) == -1 and b"even" in lib.mstg_last_error()
    assert lib.mstg_style16_maxpool_fwd(1, 1, 1, 1, 8, 8, 12, None) != 0 and b"multiple of 8" in lib.mstg_last_error()
    assert lib.mstg_style16_maxpool_bwd(1, 1, None, 1, 1, 8, 9, 16, None) == -1
    assert lib.mstg_style16_gram_workspace_bytes(2, 64, 24) == 0 and b"multiple of 16" in lib.mstg_last_error()
    assert lib.mstg_style16_gram_workspace_bytes(2, 64, 1024) == 0 and b"512" in lib.mstg_last_error()
    assert lib.mstg_style16_gram_workspace_bytes(2, 64 * 64, 64) == 2 * 64 * 64 * 4
    assert lib.mstg_style16_gram_workspace_bytes(1, 512 * 512, 64) == 16 * 64 * 64 * 4  # 16 slabs at most
    assert lib.mstg_style16_gram_bwd_workspace_bytes(2, 48) == 2 * 48 * 48 * 4
    assert lib.mstg_style16_gram_fwd(1, 1, 2, 64, 64, 1.0, 1, 16, None) != 0 and b"workspace" in lib.mstg_last_error()
    assert lib.mstg_style16_gram_bwd(1, 1, None, 1, 2, 64, 64, 1.0, 1, 16, None) != 0 and b"workspace" in lib.mstg_last_error()
    assert lib.mstg_style16_gram_bwd(1, 1, None, 1, 2, 64, 40, 1.0, 1, 1 << 20, None) == -5


def test_python_refusals_by_name():
    import style_loss as sl
    from mstg_hip import style_f16
    with pytest.raises(ValueError, match="precision"):
        sl.VGGFeatures(width_div=4, precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        sl.MultiStyleGramLoss(sl.VGGFeatures(width_div=4), [], (), precision="bf16")
    with pytest.raises(ValueError, match="VGGFeatures"):
        sl.MultiStyleGramLoss(sl.VGGFeatures(width_div=4), [], (), precision="mixed")
    with pytest.raises(RuntimeError, match="multiple of 16"):   # widths 8, 16, 32, 64
        sl.VGGFeatures(width_div=8, precision="mixed")
    with pytest.raises(RuntimeError, match="multiple of 16"):
        style_f16.check_channels([64, 72])
    with pytest.raises(RuntimeError, match="up to 512"):
        style_f16.check_channels([1024])
    sl.VGGFeatures(width_div=8)                                   # the fp32 path serves them
    feats = sl.VGGFeatures(width_div=4, precision="mixed")
    for shape in ((1, 3, 20, 32), (1, 3, 32, 36), (1, 3, 4, 8)):
        with pytest.raises(RuntimeError, match="multiples of 8"):
            feats(torch.zeros(shape))
    with pytest.raises(RuntimeError, match=r"\(N,3,H,W\)"):
        feats(torch.zeros(1, 4, 32, 32))
    with pytest.raises(RuntimeError, match="GPU"):                # no CPU path, no fall-back
        feats(torch.zeros(1, 3, 32, 32))
    assert sl.VGGFeatures(width_div=4).precision == "fp32"
    assert [k for k in feats.state_dict()] == [k for k in sl.VGGFeatures(width_div=4).state_dict()]


def test_emulation_rounding_is_the_casts_rounding():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(200000, generator=g) * torch.exp(torch.empty(200000).uniform_(-40.0, 12.0, generator=g))
    ties16 = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 65504.0, 65519.0, 65520.0, 1e6,
                           -65520.0, 0.0, -0.0, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, float("inf"), -float("inf")])
    tiesb = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1e-38, 1e-40, 3.3e38, 3.4e38, -3.4e38, 0.0, -0.0, float("inf")])
    for t in (x, ties16, tiesb):
        a, b = E.round_fp16(t), t.half().double()
        assert torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))
        a, b = E.round_bf16(t), t.bfloat16().double()
        assert torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))
    assert E.round_fp16(torch.tensor(1e-9)).item() == 0.0 and E.round_bf16(torch.tensor(1e-9)).item() != 0.0  # why the backward is bf16
    assert torch.isnan(E.round_fp16(torch.tensor(float("nan")))).all()


def test_emulation_scores_a_style_against_itself_as_exactly_zero():
    sd, _, styles = E.loss_inputs()
    ref = styles[1][:1]
    out = E.emulate(sd, ref, [ref], (1.0,))
    assert float(out["loss"]) == 0.0
    assert float(out["dy"].abs().max()) == 0.0
    # and not because everything is zero: against another style the loss and the gradient are there
    other = E.emulate(sd, ref, [styles[2][:1]], (1.0,))
    assert float(other["loss"]) > 0.0 and float(other["dy"].abs().max()) > 0.0
