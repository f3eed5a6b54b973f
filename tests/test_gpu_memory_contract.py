"""The memory contract of include/mstg_hip.h on the hot path: the existing parity tests, run again inside guard_helpers.memory_contract.

Each case calls an existing test body as a plain function (the way test_kernel_selection_switches_keep_parity calls
test_conv_fwd_bwd), so its reference and its tolerance are that test's own; a NaN left in a result fails its relative L2.  What the
guard adds: every output and workspace the Python layer allocates and every tensor the test uploads sits between two 64 KiB red
zones of NaNs (a store outside the tensor), the workspace is exactly as large as its query said (an under-reporting query),
outputs and workspaces start as NaNs and are never recycled memory (a read of what nobody wrote), uploads are compared with their
host copy afterwards (a mutated input), and -- align16 -- every one of them starts 16 bytes past a 256-byte boundary (a hidden
alignment assumption).  Both alignments run for every case.

Shapes are the smallest of each table that still reach ragged tiles, several images per wave and the fall-back routes; nothing that
captures a graph is wrapped.  The fp16 files allocate their workspaces with torch.empty, so they count as outputs: ``workspaces``
is asserted only for the families that go through ops._ws.  The 8-bit image side has its own file, test_gpu_memory_contract_image.py.
"""
import types

import pytest
import torch

import test_gpu_f16 as t16
import test_gpu_f16_block as t16b
import test_gpu_f16_plain as t16p
import test_gpu_f16_train as t16t
import test_gpu_f16_wide as t16w
import test_gpu_models as tmod
import test_gpu_normfuse as tnf
import test_gpu_ops as tops
import test_gpu_reductions as tred
import test_gpu_transformer as ttr
from f16_helpers import ACT_NONE, ACT_TANH, LAYER_CASES, STEM_HEAD_CASES
from guard_helpers import MemoryContractError, memory_contract

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mstg_hip import _lib
    _lib.load()  # raises if the HIP library is missing -- there is no fallback to test instead


# The only cases that run with check_inputs=False: the operation's contract is to write an argument the test uploaded.
# wrapped test -> what it writes in place
WRITES_AN_ARGUMENT = {
    "test_spectral_norm_fused_vs_torch": "the power iteration updates the uploaded u and v in place (training mode)",
    "test_spectral_norm_group_vs_single": "u and v of all seven weights are updated in place; gradients go into .grad (direct_param_grads)",
    "test_batchnorm_act": "BatchNorm in training mode updates the uploaded running_mean / running_var",
    "test_batchnorm_training_forward_and_backward": "fp16 BatchNorm in training mode updates the uploaded running statistics",
    "test_flat_adam_matches_torch": "Adam writes the parameters (and FlatAdam re-homes them into its flat buffer)",
    "test_train_step_vs_reference_golden": "the train step runs Adam on every uploaded parameter and spectral norm on u / v",
}


def _by_name(table, names):
    index = {c[0]: c for c in table}
    return [index[n] for n in names]  # KeyError if a table entry was renamed: the selection below must follow it


GUARD_CONV = _by_name(tops.CONV_CASES, [
    "head7x7 16->3 nchw-out tanh 8x12 (8-row tiles)", "k4s2 ragged 20x36", "convT ragged 5x7", "k3 d4 8->2", "k3 d1 ragged 13x21 4->5",
    "1x1 72->200 (uneven channel blocks)", "k4s1p1 64->1 (D head)", "p32 k4s2 16->16 ragged 20x36 N3", "p32 k4s2 16->64 2x2",
    "p32 convT 16->64 ragged 5x7", "p32 convT 64->16 1x1", "p32 1x1 64->16 5x7", "p32 1x1 32->32 ragged 37x53 N3",
    "w7 stem7x7 3->16 nchw-in ragged 37x53 N3", "w7 head7x7 16->3 nchw-out ragged 37x53 N3", "w7 stem7x7 1->16 nchw-in 16x16",
    "img k4s2 3->64 nchw-in ragged 36x20 N3", "img k4s2 3->24 nchw-in 2x2", "img k4s2 1->16 nchw-in 18x30"])
GUARD_STREAM = _by_name(tops.STREAM_CASES, ["stream ragged 37x53 16->20", "stream k3 d2 32->8 (two chunks)"])

# test_kernel_selection_switches_keep_parity runs four representatives (a 7x7 head, a 4x4 stride-2, a 1x1, a 3x3) under every switch;
# these are their small, ragged counterparts in GUARD_CONV
REPRESENTATIVES = ("head7x7 16->3 nchw-out tanh 8x12 (8-row tiles)", "k4s2 ragged 20x36", "1x1 72->200 (uneven channel blocks)",
                   "k3 d1 ragged 13x21 4->5")
# every switch of test_kernel_name_is_the_launched_kernel and test_kernel_selection_switches_keep_parity that re-routes a convolution pass
CONV_SWITCHES = ["MSTG_P32=0", "MSTG_P32_TH=4", "MSTG_P32_TH=8", "MSTG_P32_TH=16", "MSTG_P32_WLDS=0", "MSTG_P32_WLDS=1", "MSTG_WGRAD_OLD=1",
                 "MSTG_WGRAD_1X1=0", "MSTG_WGRAD_PLAIN=1", "MSTG_NO_DPACK=1", "MSTG_CONV_IMG=0", "MSTG_STREAM=1f", "MSTG_IGEMM=h", "MSTG_WGLOB=0",
                 "MSTG_PF=2"]
MS_SWITCHES = ["MSTG_MS_UNFUSED=1", "MSTG_MS_WGRAD_PACKED=0", "MSTG_MS_FWD4=0", "MSTG_MS_FWD4=1", "MSTG_MS_FWD4=2"]


def conv_cases_of(switch):
    """test_kernel_selection_switches_keep_parity's own filter, applied to GUARD_CONV"""
    k = switch.split("=")[0]
    out = []
    for case in GUARD_CONV:
        n = case[0]
        if (n in REPRESENTATIVES
                or (k.startswith("MSTG_P32") and n.startswith(("p32", "convT", "k4s2", "w7", "stem7x7", "head7x7")))
                or (k == "MSTG_CONV_IMG" and (n.startswith("img") or "D stem" in n))
                or (k == "MSTG_WGRAD_OLD" and n.startswith(("p32 k4s2", "p32 convT", "convT", "k4s2")))):
            out.append(case)
    return out


CASES = []


def case(ident, key, fn, ws=False, env=()):
    """ident: pytest id; key: name of the wrapped test (the key of WRITES_AN_ARGUMENT); fn(fx) runs it, fx.monkeypatch / fx.gold_dir are
    the fixtures it may need; ws: the family allocates through ops._ws; env: switches set (and read by the library) before the call"""
    CASES.append(pytest.param(key, fn, ws, tuple(env), id=ident))


# ---- fp32 convolution --------------------------------------------------------------------------------------------------------------
for c in GUARD_CONV:
    case(f"conv-{c[0]}", "test_conv_fwd_bwd", lambda fx, c=c: tops.test_conv_fwd_bwd(c), ws=True)
for sw in CONV_SWITCHES:
    for c in conv_cases_of(sw):
        case(f"conv-{sw}-{c[0]}", "test_conv_fwd_bwd", lambda fx, c=c: tops.test_conv_fwd_bwd(c), ws=True, env=[sw])
for c in GUARD_STREAM:  # sets MSTG_STREAM=1f and MSTG_P32=0 itself and asserts that the streaming kernel is the one that runs
    case(f"conv-{c[0]}", "test_conv_stream_kernel", lambda fx, c=c: tops.test_conv_stream_kernel(c, fx.monkeypatch), ws=True)

# ---- multi-scale block -------------------------------------------------------------------------------------------------------------
for sw in [None] + MS_SWITCHES:
    for shape in ((2, 21, 37, 16), (2, 9, 20, 64), (1, 16, 16, 8), (1, 8, 8, 128)):
        case(f"msblock-{sw or 'default'}-{shape}", "test_conv_channel_slices_and_accumulate",
             lambda fx, s=shape: tops.test_conv_channel_slices_and_accumulate(*s), ws=True, env=[sw] if sw else [])
case("normfuse-ms-fusion-folded", "test_ms_fusion_folded_norm_vs_chain", lambda fx: tnf.test_ms_fusion_folded_norm_vs_chain(3, 16, 16, 16), ws=True)
case("normfuse-ms-fusion-stats-apply", "test_ms_fusion_output_statistics_and_apply",
     lambda fx: tnf.test_ms_fusion_output_statistics_and_apply(3, 32, 32, 16), ws=True)
case("normfuse-conv-epilogue-stats", "test_conv_epilogue_statistics", lambda fx: tnf.test_conv_epilogue_statistics(0, 1, 32, 32, 16, 16), ws=True)
case("normfuse-conv-epilogue-stats-bias", "test_conv_epilogue_statistics_bias_dominated_channels",
     lambda fx: tnf.test_conv_epilogue_statistics_bias_dominated_channels(), ws=True)
case("normfuse-stem-fold", "test_stem_norm_folded_into_stride2_conv_vs_chain",
     lambda fx: tnf.test_stem_norm_folded_into_stride2_conv_vs_chain(3, 32, 48, 16, 32), ws=True)
case("normfuse-backward-sums", "test_norm_backward_sums_from_the_consumer_convolution",
     lambda fx: tnf.test_norm_backward_sums_from_the_consumer_convolution(1, 2, 32, 32, 32, 16, 4, fx.monkeypatch), ws=True)

# ---- norms -------------------------------------------------------------------------------------------------------------------------
for shape in ((3, 7, 9, 32, 2), (2, 2, 2, 64, 2), (2, 16, 16, 4, 0), (1, 96, 96, 24, 1)):
    for residual in (False, True):
        case(f"instnorm-{shape}-res{int(residual)}", "test_instnorm_act", lambda fx, s=shape, r=residual: tops.test_instnorm_act(*s, r), ws=True)
case("batchnorm-(2, 16, 16, 16, 2)", "test_batchnorm_act", lambda fx: tops.test_batchnorm_act(2, 16, 16, 16, 2), ws=True)

# ---- attention ---------------------------------------------------------------------------------------------------------------------
CORE = ((1, 4, 8, 16), (2, 8, 12, 8), (1, 4, 4, 200), (1, 8, 4, 48))
FUSED = ((3, 4, 4, 16), (1, 4, 4, 64), (2, 8, 12, 64), (1, 16, 16, 32))
NORM_ATTN = ((16, 3, 16, 24), (32, 1, 8, 8), (64, 1, 4, 4))  # the smallest case of each width
for s in CORE:
    case(f"attn-core-{s}", "test_window_attention_core", lambda fx, s=s: tops.test_window_attention_core(*s))
case("attn-window2", "test_local_attention_other_window_sizes",
     lambda fx: tops.test_local_attention_other_window_sizes(8, 2, (2, 8, 6, 10)), ws=True)
for s in FUSED:
    case(f"attn-fused-{s}", "test_local_attention_fused_vs_oracle", lambda fx, s=s: tops.test_local_attention_fused_vs_oracle(*s), ws=True)
for s in NORM_ATTN:
    case(f"attn-norm-{s}", "test_norm_attention_fused_vs_chain_and_torch",
         lambda fx, s=s: tnf.test_norm_attention_fused_vs_chain_and_torch(*s), ws=True)
# the switches, on the cases they affect (the selection of test_kernel_selection_switches_keep_parity, at these shapes)
for s in FUSED:
    case(f"attn-MSTG_ATTN_REG=0-fused-{s}", "test_local_attention_fused_vs_oracle",
         lambda fx, s=s: tops.test_local_attention_fused_vs_oracle(*s), ws=True, env=["MSTG_ATTN_REG=0"])
for s in NORM_ATTN:
    case(f"attn-MSTG_ATTN_REG=0-norm-{s}", "test_norm_attention_fused_vs_chain_and_torch",
         lambda fx, s=s: tnf.test_norm_attention_fused_vs_chain_and_torch(*s), ws=True, env=["MSTG_ATTN_REG=0"])
case("attn-MSTG_ATTN_BLK64=0-core-(1, 8, 4, 48)", "test_window_attention_core", lambda fx: tops.test_window_attention_core(1, 8, 4, 48),
     env=["MSTG_ATTN_BLK64=0"])
case("attn-MSTG_ATTN_BLK4=0-core-(1, 4, 4, 200)", "test_window_attention_core", lambda fx: tops.test_window_attention_core(1, 4, 4, 200),
     env=["MSTG_ATTN_BLK4=0"])
case("attn-MSTG_ATTN_BIG32=1-fused-(1, 16, 16, 32)", "test_local_attention_fused_vs_oracle",
     lambda fx: tops.test_local_attention_fused_vs_oracle(1, 16, 16, 32), ws=True, env=["MSTG_ATTN_BIG32=1"])
case("attn-MSTG_ATTN_BIG32=1-norm-(32, 1, 8, 8)", "test_norm_attention_fused_vs_chain_and_torch",
     lambda fx: tnf.test_norm_attention_fused_vs_chain_and_torch(32, 1, 8, 8), ws=True, env=["MSTG_ATTN_BIG32=1"])

# ---- spectral norm -----------------------------------------------------------------------------------------------------------------
for s in ((16, 3, 4, 4), (128, 64, 4, 4), (128, 128, 3, 3), (1, 128, 4, 4), (24, 8, 1, 1)):
    case(f"spectral-{s}", "test_spectral_norm_fused_vs_torch", lambda fx, s=s: tops.test_spectral_norm_fused_vs_torch(s), ws=True)
case("spectral-group", "test_spectral_norm_group_vs_single", lambda fx: tops.test_spectral_norm_group_vs_single(), ws=True)

# ---- losses, style, element-wise ---------------------------------------------------------------------------------------------------
case("losses-act-pool", "test_losses_act_pool", lambda fx: tops.test_losses_act_pool(), ws=True)
case("maxpool-gram", "test_maxpool_and_gram_vs_torch", lambda fx: tops.test_maxpool_and_gram_vs_torch(), ws=True)
case("weighted-sum-direct-attention-grads", "test_weighted_loss_sum_and_direct_attention_grads",
     lambda fx: tops.test_weighted_loss_sum_and_direct_attention_grads(), ws=True)
case("flat-adam", "test_flat_adam_matches_torch", lambda fx: tops.test_flat_adam_matches_torch())
for c in tred.CHANNEL_SUM_CASES[:2]:
    case(f"channel-sum-{c[:4]}", "test_channel_sum_exact", lambda fx, c=c: tred.test_channel_sum_exact(*c), ws=True)
for s in ((1, 1, 1, 1), (2, 3, 16, 16)):
    case(f"plane-sum-{s}", "test_plane_sum_nchw_exact", lambda fx, s=s: tred.test_plane_sum_nchw_exact(s), ws=True)
for s in ((2, 1, 1, 3), (3, 64, 64, 1)):
    case(f"spatial-mean-{s}", "test_spatial_mean_exact", lambda fx, s=s: tred.test_spatial_mean_exact(s))


def _act_and_add_tails(n):
    """test_act_and_add_raw_tails keeps 8 sentinel floats behind its outputs in a buffer torch.full made, which the guard does not
    reach; this driver calls the same three C entries on outputs of exactly n floats from torch.empty, so that the red zone stands where
    the sentinels stood.  Same references and bars: ReLU, LeakyReLU(0.2) and add bit for bit against torch on the CPU, tanh at 1e-6."""
    import torch.nn.functional as F
    from conftest import rel_l2
    from mstg_hip import _lib, ops
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    x, dy, b = tred.rnd((n,), 41, 2.0), tred.rnd((n,), 42), tred.rnd((n,), 43, 3.0)
    x[: min(n, 3)] = torch.tensor([0.0, -0.0, 1.0])[: min(n, 3)]
    xg, dyg, bg = x.to(DEV), dy.to(DEV), b.to(DEV)
    fwd = {ops.ACT_RELU: F.relu, ops.ACT_LEAKY02: lambda t: F.leaky_relu(t, 0.2)}
    for act in (ops.ACT_RELU, ops.ACT_LEAKY02, ops.ACT_TANH):
        y, dx = torch.empty(n, dtype=torch.float32, device=DEV), torch.empty(n, dtype=torch.float32, device=DEV)
        _lib.check(lib.mstg_act_fwd(xg.data_ptr(), y.data_ptr(), n, act, st), "mstg_act_fwd")
        src = y if act == ops.ACT_TANH else xg  # tanh's derivative is taken from the output
        _lib.check(lib.mstg_act_bwd(src.data_ptr(), dyg.data_ptr(), dx.data_ptr(), n, act, st), "mstg_act_bwd")
        if act == ops.ACT_TANH:
            tred.report(f"tanh n={n} y", rel_l2(y, torch.tanh(x.double())), 1e-6)
            tred.report(f"tanh n={n} dx", rel_l2(dx, dy.double() * (1 - y.cpu().double() ** 2)), 1e-6)
        else:
            xr = x.clone().requires_grad_(True)
            yr = fwd[act](xr)
            (dxr,) = torch.autograd.grad((yr * dy).sum(), [xr])
            assert torch.equal(y.cpu(), yr.detach()) and torch.equal(dx.cpu(), dxr), act
    y = torch.empty(n, dtype=torch.float32, device=DEV)
    _lib.check(lib.mstg_add(xg.data_ptr(), bg.data_ptr(), y.data_ptr(), n, st), "mstg_add")
    assert torch.equal(y.cpu(), x + b)


for n in (1, 2):
    case(f"mean-losses-{n}", "test_mean_losses_exact", lambda fx, n=n: tred.test_mean_losses_exact(n), ws=True)
for n in tred.EW_SIZES[:7] + [1025, 1027]:  # every n & 3 tail below one float4 and just above a full block; the 2M case stays in the original
    case(f"act-add-tails-{n}", "_act_and_add_tails", lambda fx, n=n: _act_and_add_tails(n))

# ---- transformer -------------------------------------------------------------------------------------------------------------------
for s in ((1, 3, 4, 4), (3, 3, 20, 36)):
    case(f"structure-map-{s}", "test_structure_map_borders", lambda fx, s=s: ttr.test_structure_map_borders(s))
for c in ttr.LN_EDGES:
    case(f"ln-mod-{c}", "test_layer_norm_mod_edges_vs_fp64", lambda fx, c=c: ttr.test_layer_norm_mod_edges_vs_fp64(*c), ws=True)
for c in ((2, 130, 2, 16), (3, 5, 1, 8), (2, 127, 1, 64), (1, 65, 4, 32), (2, 15, 4, 8)):
    case(f"flash-ragged-{c}", "test_flash_attention_ragged_tiles_of_several_images",
         lambda fx, c=c: ttr.test_flash_attention_ragged_tiles_of_several_images(*c))
case("flash-single-token", "test_flash_attention_single_token", lambda fx: ttr.test_flash_attention_single_token())
case("flash-large-logits", "test_flash_attention_large_logits", lambda fx: ttr.test_flash_attention_large_logits())

# ---- fp16 inference ----------------------------------------------------------------------------------------------------------------
for c in t16.CONV_CASES:
    case(f"f16-conv-{c[0]}", "test_f16_conv", lambda fx, c=c: t16.test_f16_conv(c))
case("f16-msblock-(16, 1, 8, 8)", "test_f16_msblock_branches", lambda fx: t16.test_f16_msblock_branches(16, 1, 8, 8))
for c in ((16, 2, 16, 24, True), (32, 1, 8, 72, True), (64, 1, 8, 8, False), (16, 1, 4, 260, False)):
    for reg in ("1", "0"):
        case(f"f16-attn-{c}-reg{reg}", "test_f16_local_attention", lambda fx, c=c, reg=reg: t16.test_f16_local_attention(*c, reg, fx.monkeypatch))
case("f16-norm-residual", "test_f16_norm_residual", lambda fx: t16.test_f16_norm_residual())
case("f16-head-tanh-nchw", "test_f16_head_tanh_nchw", lambda fx: t16.test_f16_head_tanh_nchw())
for c in t16w.CONV_CASES:
    if "ragged" in c[0] or (c[3], c[4]) == (17, 33):
        case(f"f16-wide-conv-{c[0]}", "test_f16_wide_conv", lambda fx, c=c: t16w.test_f16_wide_conv(c))
case("f16-wide-msblock-(256, 2, 9, 13)", "test_f16_wide_msblock_branches", lambda fx: t16w.test_f16_wide_msblock_branches(256, 2, 9, 13, False))
SMALL_LAYERS = [c for c in LAYER_CASES if "64x64" not in c[0]]
assert len(SMALL_LAYERS) == len(LAYER_CASES) - 2
for c in SMALL_LAYERS:
    case(f"f16-plain-layer-{c[0]}", "test_plain_layer", lambda fx, c=c: t16p.test_plain_layer(c))
for c in STEM_HEAD_CASES[:3]:
    case(f"f16-plain-stem-{c[0]}", "test_plain_stem", lambda fx, c=c: t16p.test_plain_stem(c))
    for act in (ACT_TANH, ACT_NONE):
        case(f"f16-plain-head-{c[0]}-act{act}", "test_plain_head", lambda fx, c=c, act=act: t16p.test_plain_head(c, act))
for c in t16b.LIN[:5]:  # dim 64: one of each epilogue and output type
    case(f"f16-token-gemm-{c}", "test_token_gemm", lambda fx, c=c: t16b.test_token_gemm(*c))
for struct in (True, False):
    for x_f16 in (True, False):
        case(f"f16-ln-mod-64-{struct}-{x_f16}", "test_ln_mod", lambda fx, s=struct, x=x_f16: t16b.test_ln_mod(64, s, x))
for c in ((256, 2, 48), (64, 3, 240)):
    case(f"f16-token-mean-{c}", "test_token_mean", lambda fx, c=c: t16b.test_token_mean(*c))
for D in (16, 32, 64):
    case(f"f16-flash-D{D}-N1-L48", "test_flash_attention_f16", lambda fx, D=D: t16b.test_flash_attention_f16(D, 1, 48))

# ---- fp16 training -----------------------------------------------------------------------------------------------------------------
for c in SMALL_LAYERS:
    case(f"f16-train-wgrad-{c[0]}", "test_wgrad_layer", lambda fx, c=c: t16t.test_wgrad_layer(c))
for c in _by_name(t16t.BN_CASES, ["8 ch leaky", "512 ch relu, 8 values per channel"]):  # 4096 elements each, the two smallest
    case(f"f16-train-bn-{c[0]}", "test_batchnorm_training_forward_and_backward", lambda fx, c=c: t16t.test_batchnorm_training_forward_and_backward(c))
case("f16-train-head-loss", "test_head_loss_and_its_gradient", lambda fx: t16t.test_head_loss_and_its_gradient())
case("f16-train-stem-act-bwd", "test_stem_activation_backward", lambda fx: t16t.test_stem_activation_backward())

# ---- whole model: red zones and finite results; parity is the original tests' business ---------------------------------------------
case("model-generator-fwd-bwd", "test_generator_backward_is_deterministic", lambda fx: tmod.test_generator_backward_is_deterministic(), ws=True)
case("model-train-step", "test_train_step_vs_reference_golden", lambda fx: tmod.test_train_step_vs_reference_golden(fx.gold_dir), ws=True)


@pytest.mark.parametrize("align16", [False, True], ids=["align256", "align16"])
@pytest.mark.parametrize("key,fn,ws,env", CASES)
def test_memory_contract(key, fn, ws, env, align16, monkeypatch, gold_dir):
    from mstg_hip import ops
    for sw in env:
        monkeypatch.setenv(*sw.split("="))
    ops.refresh_env()
    fx = types.SimpleNamespace(monkeypatch=monkeypatch, gold_dir=gold_dir)
    with memory_contract(align16=align16, check_inputs=key not in WRITES_AN_ARGUMENT) as mc:
        fn(fx)
    print(f"  [guard] outputs {mc.outputs} workspaces {mc.workspaces} uploads {mc.uploads} passthrough {mc.passthrough}")
    assert mc.outputs >= 1 and mc.uploads >= 1, (mc.outputs, mc.uploads)
    if ws:
        assert mc.workspaces >= 1


def test_exemptions_name_wrapped_tests():
    keys = {p.values[0] for p in CASES}
    assert set(WRITES_AN_ARGUMENT) <= keys, set(WRITES_AN_ARGUMENT) - keys


@pytest.mark.parametrize("align16", [False, True], ids=["align256", "align16"])
def test_guard_sees_a_store_past_the_end_on_the_device(align16):
    """The guard's self-check: one float stored just past a small torch.empty, through a view of the buffer the helper itself owns --
    no kernel misbehaves and nothing outside that buffer is touched."""
    with pytest.raises(MemoryContractError, match=r"AFTER output \(5, 3\) torch.float32 allocated at .*test_gpu_memory_contract.py.*byte offset 60 "):
        with memory_contract(align16=align16) as mc:
            t = torch.empty((5, 3), dtype=torch.float32, device=DEV)
            assert t.is_cuda and t.data_ptr() % 256 == (16 if align16 else 0) and bool(torch.isnan(t).all())
            t.zero_()
            buf, off = mc.raw(t)
            buf[off + 60:off + 64].view(torch.float32)[0] = 1.0
    assert mc.outputs == 1
    with memory_contract(align16=align16) as mc:  # and the same sequence without the store passes
        torch.empty((5, 3), dtype=torch.float32, device=DEV).zero_()
        x = torch.ones(7).to(DEV)
        assert x.data_ptr() % 256 == (16 if align16 else 0)
    assert (mc.outputs, mc.uploads) == (1, 1)
