"""fp16 inference at channels=32 and 64 (stage widths up to 256; csrc/infer_f16_wide.hip for the layers with more than 64 input or
output channels).  Same references and bars as test_gpu_f16.py: per kernel against fp32 torch on the CPU evaluated on the same
fp16-rounded operands (2e-3 relative L2; 5e-3 for LocalAttention), whole generator against this build's fp32 path (3e-2 at the
taps and pre-tanh, 2e-2 on the image)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from f16_helpers import DEV, _lib_loaded, h, nhwc, norm_relu, report, rnd, stats_of  # noqa: F401

pytestmark = pytest.mark.gpu


CONV_CASES = [
    # name, kind, N, H, W, Cin, Cout, K, stride, pad, normalise-on-load
    ("stem 7x7 3->32 (NCHW fp32 image)", 0, 2, 32, 48, 3, 32, 7, 1, 3, False),
    ("stem 7x7 3->64 (NCHW fp32 image)", 0, 1, 40, 24, 3, 64, 7, 1, 3, False),
    ("k4 s2 64->128 + norm on load", 0, 2, 32, 48, 64, 128, 4, 2, 1, True),
    ("k4 s2 64->128", 0, 1, 40, 24, 64, 128, 4, 2, 1, False),
    ("k4 s2 128->256 + norm on load", 0, 2, 16, 32, 128, 256, 4, 2, 1, True),
    ("k4 s2 128->256 ragged output 11x7", 0, 1, 22, 14, 128, 256, 4, 2, 1, True),
    ("convT 256->128 + norm on load", 1, 2, 8, 12, 256, 128, 4, 2, 1, True),
    ("convT 128->64 ragged 20x36", 1, 1, 20, 36, 128, 64, 4, 2, 1, False),
    ("convT 128->64 + norm on load", 1, 1, 16, 16, 128, 64, 4, 2, 1, True),
    ("1x1 128->128 + norm on load", 0, 2, 24, 20, 128, 128, 1, 1, 0, True),
    ("1x1 256->256 + norm on load", 0, 1, 17, 33, 256, 256, 1, 1, 0, True),
    ("1x1 256->256", 0, 1, 16, 16, 256, 256, 1, 1, 0, False),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_f16_wide_conv(case):
    from mstg_hip.infer import _PackedConv
    name, kind, N, H, W, Cin, Cout, K, s, p, norm = case
    image = Cin == 3
    w = rnd((Cin, Cout, K, K) if kind == 1 else (Cout, Cin, K, K), 1, (2.0 / (Cin * K * K)) ** 0.5)
    b = rnd((Cout,), 2, 0.1)
    x = rnd((N, Cin, H, W), 3) * 1.5 + 0.3
    pc = _PackedConv(kind, [w.to(DEV)], [b.to(DEV)], Cin, Cout, K, s, p, src_nchw_f32=int(image))
    xin, xr = (x.to(DEV), h(x)) if image else (nhwc(x), h(x))
    st = None
    if norm:
        st = stats_of(xr)
        xr = h(norm_relu(xr, st))
    y, ost = pc(xin, in_stats=None if st is None else st.to(DEV).contiguous(), want_stats=True)
    ref = F.conv_transpose2d(xr, h(w), b, stride=2, padding=1) if kind == 1 else F.conv2d(xr, h(w), b, stride=s, padding=p)
    assert y.shape == (ref.shape[0], ref.shape[2], ref.shape[3], Cout)
    report(name + " y", rel_l2(y.float().permute(0, 3, 1, 2), ref), 2e-3)
    rst = stats_of(ref)
    report(name + " mean", float((ost[..., 0].cpu() - rst[..., 0]).abs().max() / rst[..., 0].abs().max().clamp_min(1e-3)), 2e-3)
    report(name + " rstd", rel_l2(ost[..., 1], rst[..., 1]), 2e-3)


@pytest.mark.parametrize("Cin", [32, 64])
def test_f16_head_tanh_nchw_wide_input(Cin):
    from mstg_hip.infer import _PackedConv
    from mstg_hip.ops import ACT_TANH
    N, H, W = 2, 24, 40
    w, b, x = rnd((3, Cin, 7, 7), 1, 0.03), rnd((3,), 2, 0.1), rnd((N, Cin, H, W), 3)
    pc = _PackedConv(0, [w.to(DEV)], [b.to(DEV)], Cin, 3, 7, 1, 3, dst_nchw=1, act=ACT_TANH)
    y, _ = pc(nhwc(x))
    ref = torch.tanh(F.conv2d(h(x), h(w), b, padding=3))
    assert y.shape == (N, 3, H, W) and y.dtype == torch.float16
    report(f"head 7x7 {Cin}->3 tanh NCHW", rel_l2(y.float(), ref), 2e-3)


@pytest.mark.parametrize("ch,N,H,W,norm", [(128, 2, 24, 40, False), (128, 1, 20, 12, True), (256, 1, 16, 20, True), (256, 2, 9, 13, False)])
def test_f16_wide_msblock_branches(ch, N, H, W, norm):
    from mstg_hip.infer import _PackedConv
    c4 = ch // 4
    ws = [rnd((c4, ch, 1, 1), 11, (2.0 / ch) ** 0.5)] + [rnd((c4, ch, 3, 3), 12 + i, (2.0 / (9 * ch)) ** 0.5) for i in range(3)]
    bs = [rnd((c4,), 20 + i, 0.1) for i in range(4)]
    x = rnd((N, ch, H, W), 5) + 0.2
    pc = _PackedConv(2, [w.to(DEV) for w in ws], [b.to(DEV) for b in bs], ch, ch, 3, 1, 4)
    xr, st = h(x), None
    if norm:
        st = stats_of(xr)
        xr = h(norm_relu(xr, st))
    y, ost = pc(nhwc(x), in_stats=None if st is None else st.to(DEV).contiguous(), want_stats=True)
    outs = [F.conv2d(xr, h(ws[0]), bs[0])] + [F.conv2d(xr, h(ws[i]), bs[i], padding=d, dilation=d) for i, d in ((1, 1), (2, 2), (3, 4))]
    ref = torch.cat(outs, dim=1)
    report(f"msblock branches ch{ch} {H}x{W} y", rel_l2(y.float().permute(0, 3, 1, 2), ref), 2e-3)
    report(f"msblock branches ch{ch} {H}x{W} rstd", rel_l2(ost[..., 1], stats_of(ref)[..., 1]), 2e-3)


@pytest.mark.parametrize("C_,N,H,W,norm", [(128, 2, 16, 24, True), (128, 1, 8, 8, False), (256, 1, 8, 12, True), (256, 2, 4, 20, False),
                                           # more windows than persistent waves: every wave walks several
                                           (128, 2, 64, 260, True), (256, 1, 128, 132, False)])
def test_f16_wide_local_attention(C_, N, H, W, norm):
    from mstg_hip.infer import _PackedAttention
    from oracle import restatement as R
    import enhanced_generator as eg
    m = eg.LocalAttention(C_, window_size=4)
    sd = {"p.qkv.weight": rnd((3 * C_, C_, 1, 1), 1, (1.0 / C_) ** 0.5), "p.qkv.bias": rnd((3 * C_,), 2, 0.1),
          "p.proj.weight": rnd((C_, C_, 1, 1), 3, (1.0 / C_) ** 0.5), "p.proj.bias": rnd((C_,), 4, 0.1)}
    m.load_state_dict({k[2:]: v for k, v in sd.items()})
    m.to(DEV)
    pa = _PackedAttention(m)
    x = rnd((N, C_, H, W), 5) * 1.3 + 0.2
    xr, st = h(x), None
    if norm:
        st = stats_of(xr)
        xr = h(norm_relu(xr, st))
    y = pa(nhwc(x), in_stats=None if st is None else st.to(DEV).contiguous())
    sdr = {k: (h(v) if k.endswith("weight") else v) for k, v in sd.items()}
    ref = R.local_attention(xr, sdr, "p", 4)
    report(f"LocalAttention fp16 C{C_} {H}x{W}", rel_l2(y.float().permute(0, 3, 1, 2), ref), 5e-3)


@pytest.mark.parametrize("C_", [128, 256])
def test_f16_wide_norm_residual(C_):
    from mstg_hip import infer
    x, r = rnd((2, C_, 12, 20), 1) * 2 + 0.5, rnd((2, C_, 12, 20), 2)
    st = stats_of(h(x))
    y = infer.norm_residual(nhwc(x), nhwc(r), st.to(DEV).contiguous())
    report(f"norm + relu + residual fp16 C{C_}", rel_l2(y.float().permute(0, 3, 1, 2), norm_relu(h(x), st) + h(r)), 1e-3)


@pytest.mark.parametrize("kind,cin,cout,k,s,p,hw", [(0, 64, 128, 4, 2, 1, (40, 24)), (0, 128, 256, 4, 2, 1, (18, 22)),
                                                    (1, 256, 128, 4, 2, 1, (12, 20)), (1, 128, 64, 4, 2, 1, (9, 17)),
                                                    (0, 256, 256, 1, 1, 0, (13, 21))])
def test_f16_wide_conv_residual_operand_vs_separate_pass(kind, cin, cout, k, s, p, hw):
    from mstg_hip import infer
    g = torch.Generator().manual_seed(451)
    N, (H, W) = 2, hw
    w = (torch.randn((cin, cout, k, k) if kind == 1 else (cout, cin, k, k), generator=g) * 0.05).to(DEV)
    b = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    f = torch.randn((N, H, W, cin), generator=g).half().to(DEV)
    a = torch.randn((N, H, W, cin), generator=g).half().to(DEV)
    ff = f.float()
    stats = torch.stack([ff.mean(dim=(1, 2)), (ff.var(dim=(1, 2), unbiased=False) + 1e-5).rsqrt()], dim=-1).contiguous()
    conv = infer._PackedConv(kind, [w], [b], cin, cout, k, s, p)
    y_fold, st_fold = conv(f, in_stats=stats, want_stats=True, residual=a)
    y_pass, st_pass = conv(infer.norm_residual(f, a, stats), want_stats=True)
    assert torch.equal(y_fold, y_pass) and torch.equal(st_fold, st_pass)


def _pair(seed, channels, blocks=0):
    import enhanced_generator as eg
    from oracle import restatement as R
    spec = R.generator_spec_with_blocks(channels, blocks) if blocks else R.generator_spec(channels)
    m = eg.EnhancedGenerator(channels=channels, num_transformer_blocks=blocks)
    m.load_state_dict(R.make_state_dict(spec, seed))
    return m.to(DEV).eval()


@pytest.mark.parametrize("channels,shape", [(32, (2, 3, 64, 64)), (32, (1, 3, 48, 80)), (64, (2, 3, 64, 64)), (64, (1, 3, 256, 256))])
def test_f16_wide_generator_vs_fp32_path(channels, shape):
    from oracle import restatement as R
    m = _pair(401, channels)
    x = R.make_input(shape, 402).to(DEV)
    t32, t16 = {}, {}
    with torch.no_grad():
        y32 = m.forward_taps(x, t32)
        m.half_inference()
        y16 = m.forward_taps(x, t16)
        m.half_inference(False)
        y32b = m(x)
    assert y16.dtype == torch.float16 and y16.shape == y32.shape and torch.isfinite(y16).all()
    assert torch.equal(y32, y32b)
    for k in ("down1", "down2", "up1", "up2", "pre_tanh"):
        assert torch.isfinite(t16[k]).all()
        report(f"c{channels} fp16 vs fp32 {shape[2]}x{shape[3]} tap {k}", rel_l2(t16[k].float(), t32[k]), 3e-2)
    report(f"c{channels} fp16 vs fp32 {shape[2]}x{shape[3]} out", rel_l2(y16.float(), y32), 2e-2)


def test_f16_generate_new_image_model_vs_fp32_path():
    """generate_new_image.py's model: EnhancedGenerator(channels=64, num_transformer_blocks=3), at 256x256."""
    from oracle import restatement as R
    m = _pair(421, 64, blocks=3)
    x = R.make_input((1, 3, 256, 256), 422).to(DEV)
    t32, t16 = {}, {}
    with torch.no_grad():
        y32 = m.forward_taps(x, t32)
        m.half_inference()
        y16 = m.forward_taps(x, t16)
        y16b = m(x)
        m.half_inference(False)
    assert y16.dtype == torch.float16 and torch.isfinite(y16).all() and torch.equal(y16, y16b)
    for k in ("down2", "up1", "up2", "pre_tanh"):
        report(f"c64+3 blocks fp16 vs fp32 256x256 tap {k}", rel_l2(t16[k].float(), t32[k]), 3e-2)
    report("c64+3 blocks fp16 vs fp32 256x256 out", rel_l2(y16.float(), y32), 2e-2)


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 48, 80), (1, 3, 256, 256)])
def test_f16_wide_residual_folded_into_next_layer_is_bit_identical(shape, monkeypatch):
    from oracle import restatement as R
    m = _pair(441, 64)
    x = R.make_input(shape, 442).to(DEV)
    m.half_inference()
    with torch.no_grad():
        y_fold = m(x)
        monkeypatch.setenv("MSTG_F16_FOLD_RESIDUAL", "0")
        y_pass = m(x)
        y_taps = m.forward_taps(x, {})
    assert torch.isfinite(y_fold).all() and torch.equal(y_fold, y_pass) and torch.equal(y_fold, y_taps)


def test_f16_wide_batch64_1024():
    """channels=64 at batch 64, 1024x1024 (one activation tensor holds 2^32 elements): finite, samples 0 / 63 equal the batch-1
    results of the same images, batch 1 within 2e-2 of the fp32 path."""
    from oracle import restatement as R
    m = _pair(421, 64)
    x1 = R.make_input((1, 3, 1024, 1024), 422).to(DEV)
    with torch.no_grad():
        y32 = m(x1)
        m.half_inference()
        y1 = m(x1)
        report("c64 1024x1024 fp16 vs fp32 path, batch 1", rel_l2(y1.float(), y32), 2e-2)
        del y32
        g = torch.Generator().manual_seed(423)
        x = torch.rand((64, 3, 1024, 1024), generator=g) * 2 - 1
        x[0], x[63] = x1[0].cpu(), x1[0].cpu().flip(-1)
        xd = x.to(DEV)
        y = m(xd)
        y63 = m(xd[63:64])
    assert torch.isfinite(y).all()
    report("c64 fp16 sample 0 of batch 64 vs batch 1", rel_l2(y[0:1].float(), y1.float()), 1e-3)
    report("c64 fp16 sample 63 of batch 64 vs batch 1", rel_l2(y[63:64].float(), y63.float()), 1e-3)


def test_f16_wide_graph_inference_matches_eager():
    from oracle import restatement as R
    m = _pair(431, 64)
    m.half_inference()
    x = R.make_input((1, 3, 256, 256), 432).to(DEV)
    x2 = R.make_input((2, 3, 64, 80), 433).to(DEV)
    with torch.no_grad():
        y_eager, y2_eager = m(x), m(x2)
        m.graph_inference()
        y_graph, y2_graph = m(x), m(x2)
        assert torch.equal(y_eager, y_graph) and torch.equal(y2_eager, y2_graph)
        assert torch.equal(m(x), y_eager)
        m.graph_inference(False)


def test_f16_other_widths_still_raise():
    import enhanced_generator as eg
    for c in (8, 48):
        with pytest.raises(RuntimeError, match="channels=16"):
            eg.EnhancedGenerator(channels=c, num_transformer_blocks=0).to(DEV).half_inference()
