"""CPU: the fp16 StructuralTransformerBlock kernels (csrc/infer_f16_block.hip, mstg_hip/infer_block.py) are declared and exported,
plan every Linear layer of the blocks of EnhancedGenerator(16 / 32 / 64), and refuse what no kernel serves with a message, through
host-side validation.  No kernel is launched here."""
import ctypes as C

import pytest
import torch

ENTRY_POINTS = ("mstg_f16_linear_plan_bytes", "mstg_f16_linear_pack", "mstg_f16_linear_fwd", "mstg_f16_ln_mod_fwd",
                "mstg_f16_token_mean_workspace_bytes", "mstg_f16_token_mean", "mstg_f16_flash_attn_fwd")


@pytest.fixture(scope="module")
def lib():
    from mstg_hip import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_entry_points_declared_and_exported(lib):
    import os
    from mstg_hip import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "mstg_hip.h")).read()
    for name in ENTRY_POINTS:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None


def layers_of(dim):
    """(Cin, Cout) of the qkv, proj, fc1, fc2 layers of StructuralTransformerBlock(dim)"""
    return [(dim, 3 * dim), (dim, dim), (dim, 2 * dim), (2 * dim, dim)]


@pytest.mark.parametrize("dim", [64, 128, 256])
def test_every_block_layer_has_a_plan(lib, dim):
    for Cin, Cout in layers_of(dim):
        n = lib.mstg_f16_linear_plan_bytes(Cin, Cout)
        assert n > 0, (Cin, Cout, lib.mstg_last_error().decode())
        assert n >= Cout * 4 + Cin * Cout * 2  # fp32 bias, every filter element in fp16


@pytest.mark.parametrize("Cin,Cout,what", [(32, 64, b"Cin"), (96, 64, b"Cin"), (1024, 64, b"Cin"), (64, 48, b"Cout"),
                                           (64, 800, b"Cout"), (64, 0, b"Cout"), (128, 832, b"Cout")])
def test_unsupported_linear_shapes_refused_with_a_message(lib, Cin, Cout, what):
    assert lib.mstg_f16_linear_plan_bytes(Cin, Cout) == 0
    assert what in lib.mstg_last_error(), lib.mstg_last_error()


def test_host_side_validation(lib):
    # token GEMM
    assert lib.mstg_f16_linear_fwd(None, None, None, None, 1, 16, 64, 64, 0, 1, None) == -1          # null pointers
    assert lib.mstg_f16_linear_pack(None, None, 64, 64, None, 0, None) == -1
    assert lib.mstg_f16_linear_pack(1, None, 64, 64, 1, 16, None) == -1                              # blob too small
    assert b"blob" in lib.mstg_last_error()
    assert lib.mstg_f16_linear_fwd(1, 1, None, 1, 1, 16, 64, 96, 0, 1, None) == -5
    assert b"Cout" in lib.mstg_last_error()
    assert lib.mstg_f16_linear_fwd(1, 1, None, 1, 1, 16, 64, 64, 1, 1, None) == -5                   # ReLU: not a block epilogue
    assert b"act" in lib.mstg_last_error()
    assert lib.mstg_f16_linear_fwd(1, 1, None, 1, 0, 16, 64, 64, 0, 1, None) == -1
    # LayerNorm + modulation
    assert lib.mstg_f16_ln_mod_fwd(1, 1, None, None, None, 1, 1, None, None, 1, 1, 16, 96, 1e-5, None) == -5
    assert b"dim" in lib.mstg_last_error()
    assert lib.mstg_f16_ln_mod_fwd(1, 1, 1, None, None, 1, 1, None, None, 1, 1, 16, 64, 1e-5, None) == -1
    assert b"struct_proj" in lib.mstg_last_error()
    assert lib.mstg_f16_ln_mod_fwd(1, 0, None, None, None, 1, 1, None, 1, 1, 1, 16, 64, 1e-5, None) == -1
    assert b"structure map" in lib.mstg_last_error()
    assert lib.mstg_f16_ln_mod_fwd(None, 1, None, None, None, None, None, None, None, None, 1, 16, 64, 1e-5, None) == -1
    # token mean
    assert lib.mstg_f16_token_mean_workspace_bytes(2, 4096, 64) > 0
    assert lib.mstg_f16_token_mean(1, 1, 2, 4096, 64, 1, 16, None) == -4
    assert b"workspace" in lib.mstg_last_error()
    assert lib.mstg_f16_token_mean(1, 1, 2, 4096, 48, 1, 1 << 20, None) == -5
    # flash attention: head widths 16 / 32 / 64
    for D in (8, 4, 128, 24):
        assert lib.mstg_f16_flash_attn_fwd(1, 1, 1, 64, 4, D, None) == -5
        assert f"head width {D}".encode() in lib.mstg_last_error(), lib.mstg_last_error()
    assert lib.mstg_f16_flash_attn_fwd(None, 1, 1, 64, 4, 16, None) == -1
    assert lib.mstg_f16_flash_attn_fwd(1, 1, 0, 64, 4, 16, None) == -1


def test_block_plan_refuses_head_width_8_before_touching_the_gpu():
    from mstg_hip.infer_block import HalfBlock, check_block
    from structural_transformer import StructuralTransformerBlock
    blk = StructuralTransformerBlock(dim=32)  # 4 heads of width 8: the fp32 kernels serve it, the fp16 ones do not
    with pytest.raises(RuntimeError, match="head width 8"):
        HalfBlock(blk)
    with pytest.raises(RuntimeError, match="head width 8"):
        check_block(StructuralTransformerBlock(64, num_heads=8))
    for dim in (64, 128, 256):
        check_block(StructuralTransformerBlock(dim))


def test_generator_switch_validated_at_call_time():
    import enhanced_generator as eg
    from structural_transformer import StructuralTransformerBlock
    for C_ in (16, 32, 64):
        m = eg.EnhancedGenerator(channels=C_, num_transformer_blocks=1)
        assert m.half_inference(fp16_blocks=True) is m
        assert m.half_inference(True, False) is m and m.half_inference(False) is m
    m0 = eg.EnhancedGenerator(channels=16, num_transformer_blocks=0)
    assert m0.half_inference(fp16_blocks=True) is m0  # no blocks: accepted, no effect
    m = eg.EnhancedGenerator(channels=16, num_transformer_blocks=1)
    m.transformer_blocks[0] = StructuralTransformerBlock(64, num_heads=8)
    m.half_inference()  # the fp32 blocks serve head width 8
    with pytest.raises(RuntimeError, match="head width 8"):
        m.half_inference(fp16_blocks=True)
    assert not m._half_blocks


def test_half_inference_with_blocks_has_no_cpu_path():
    import enhanced_generator as eg
    m = eg.EnhancedGenerator(channels=16, num_transformer_blocks=1).half_inference(fp16_blocks=True).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 3, 16, 16))
