"""CPU: the arithmetic contract of the mixed-precision training attention (include/mstg_hip.h, csrc/flash_f16_train.hip) as
tests/flash_f16_train_ref.py emulates it, against float64 attention; the refusals of the Python surface that need no device; the
host-side validation of the three C entries.  No kernel is launched here.

Bars: 2e-3 on the forward (the project's per-kernel fp16 bar) and 8e-3 on the gradients (its bf16 bar, tests/test_gpu_style_f16.py).
The emulation measured, relative L2 against the yardstick: out 0.9e-4 .. 1.9e-4, dqkv 2.4e-3 .. 2.9e-3, dq and dk 2.5e-3 .. 3.4e-3,
dv 2.1e-3 .. 2.4e-3; with the incoming gradient scaled by 1e-7 the same 2.4e-3 .. 2.9e-3 -- bf16 keeps fp32's range, fp16 would
flush it."""
import pytest
import torch

import flash_f16_train_ref as ref

SHAPES = [(2, 130, 2, 16), (1, 65, 4, 32), (2, 127, 1, 64), (3, 5, 1, 16)]


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.mark.parametrize("gscale", [1.0, 1e-7])
@pytest.mark.parametrize("N,L,heads,D", SHAPES)
def test_emulation_against_the_yardstick(N, L, heads, D, gscale):
    from mstg_hip import ops
    assert "mixed" in ops.ATTENTION_PRECISIONS and D in ops.MIXED_ATTENTION_WIDTHS  # the contract under test exists in the package
    dim = heads * D
    qkv, gy = ref.rnd((N, L, 3 * dim), 1, 0.8), ref.rnd((N, L, dim), 2) * gscale
    yr, lr, gr = ref.yardstick(qkv, gy, heads)
    ye, le, ge = ref.emulate(qkv, gy, heads)
    d = {"out": ref.rel_l2(ye, yr), "lse": ref.rel_l2(le, lr), "dqkv": ref.rel_l2(ge, gr)}
    for (k, a), b in zip(ref.thirds(ge).items(), ref.thirds(gr).values()):
        d[k] = ref.rel_l2(a, b)
    print(f"  [emulation] N{N} L{L} heads{heads} D{D} gy x {gscale:g}: " + " ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert d["out"] <= 2e-3
    assert d["lse"] <= 2e-5
    for k in ("dqkv", "dq", "dk", "dv"):
        assert d[k] <= 8e-3, (k, d[k])
        assert d[k] >= 1e-4, (k, d[k])  # the roundings are really applied: a float64 copy of the yardstick would sit at 1e-16
    assert all(float(t.abs().max()) > 0 for t in ref.thirds(ge).values())


def test_unknown_precision_is_a_value_error():
    from mstg_hip import ops
    qkv = torch.zeros(1, 4, 48)
    with pytest.raises(ValueError, match="precision"):
        ops.flash_attention(qkv, 1, precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        ops.check_attention_precision("bf16")
    assert ops.check_attention_precision("fp32", 8) == "fp32" and ops.check_attention_precision("mixed", 16) == "mixed"


def test_mixed_refuses_head_width_8_by_name():
    import enhanced_generator as eg
    from mstg_hip import ops
    from structural_transformer import StructuralTransformerBlock
    with pytest.raises(RuntimeError, match="head width 8"):
        ops.flash_attention(torch.zeros(1, 4, 3 * 32), 4, precision="mixed")
    blk = StructuralTransformerBlock(32)  # 4 heads of width 8
    assert blk.attention_precision == "fp32" and "attention_precision" not in blk.state_dict()
    blk.attention_precision = "mixed"
    with pytest.raises(RuntimeError, match="head width 8"):
        blk(torch.zeros(1, 16, 32), torch.zeros(1, 32), torch.zeros(1, 3, 16, 16))
    g = eg.EnhancedGenerator(8, 1)
    with pytest.raises(RuntimeError, match="head width 8"):
        g.set_attention_precision("mixed")
    assert g.transformer_blocks[0].attention_precision == "fp32"
    with pytest.raises(ValueError):
        g.set_attention_precision("half")
    g16 = eg.EnhancedGenerator(16, 1)
    keys = list(g16.state_dict())
    assert g16.set_attention_precision("mixed") is g16 and g16.transformer_blocks[0].attention_precision == "mixed"
    assert list(g16.state_dict()) == keys


def test_environment_switch_is_validated(monkeypatch):
    from mstg_hip import ops
    monkeypatch.delenv("MSTG_ATTN_PRECISION", raising=False)
    assert ops.attention_precision_from_env(None) == "fp32"
    monkeypatch.setenv("MSTG_ATTN_PRECISION", "mixed")
    assert ops.attention_precision_from_env(None) == "mixed" and ops.attention_precision_from_env("fp32") == "fp32"
    monkeypatch.setenv("MSTG_ATTN_PRECISION", "fast")
    with pytest.raises(ValueError):
        ops.attention_precision_from_env(None)


def test_host_side_validation(lib):
    one = 256  # any non-null address: validation returns before a launch
    assert lib.mstg_f16_attn_cast_qkv(None, one, one, 1, 64, 4, 16, None) == -1
    assert lib.mstg_f16_attn_cast_qkv(one, None, one, 1, 64, 4, 16, None) == -1
    assert lib.mstg_f16_flash_attn_train_fwd(None, one, one, 1, 64, 4, 16, None) == -1
    assert lib.mstg_f16_flash_attn_train_fwd(one, one, None, 1, 64, 4, 16, None) == -1
    assert lib.mstg_f16_flash_attn_train_fwd(one, one, one, 1, 0, 4, 16, None) == -1
    assert lib.mstg_f16_flash_attn_train_bwd(one, one, one, None, one, one, 1 << 20, 1, 64, 4, 16, None) == -1
    assert lib.mstg_f16_flash_attn_train_bwd(one, one, one, one, one, None, 1 << 20, 1, 64, 4, 16, None) == -1
    for D in (8, 24, 128):
        assert lib.mstg_f16_attn_cast_qkv(one, one, one, 1, 64, 4, D, None) == -5
        assert str(D).encode() in lib.mstg_last_error()
        assert lib.mstg_f16_flash_attn_train_fwd(one, one, one, 1, 64, 4, D, None) == -5
        assert f"head width {D}".encode() in lib.mstg_last_error()
        assert lib.mstg_f16_flash_attn_train_bwd(one, one, one, one, one, one, 1 << 20, 1, 64, 4, D, None) == -5
        assert f"head width {D}".encode() in lib.mstg_last_error()
    assert lib.mstg_f16_flash_attn_train_fwd(one, one, one, 65536, 64, 4, 16, None) == -5  # the grid limits of the fp32 path
    need = lib.mstg_f16_flash_attn_train_bwd_workspace_bytes(2, 130, 2, 16)
    assert need >= 2 * 2 * 130 * 4 + 2 * 130 * 32 * 2
    assert lib.mstg_f16_flash_attn_train_bwd(one, one, one, one, one, one, need - 1, 2, 130, 2, 16, None) != 0
    assert b"workspace" in lib.mstg_last_error()
