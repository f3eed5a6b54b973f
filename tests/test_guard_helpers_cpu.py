"""The test of the tests: guard_helpers.memory_contract on CPU tensors (the helper takes the device as a parameter).  Every kind of
violation it promises to see is produced here by plain torch stores into the buffer the helper owns, and a clean sequence passes."""
import pytest
import torch

import guard_helpers as G
from guard_helpers import MemoryContractError, memory_contract


def _poke(mc, t, byte_offset, value=1.0):
    """store one float at ``byte_offset`` relative to the first byte of ``t``, through the owning buffer"""
    buf, off = mc.raw(t)
    buf[off + byte_offset:off + byte_offset + 4].view(torch.float32)[0] = value


def test_clean_sequence_passes_and_counts():
    with memory_contract(device="cpu") as mc:
        a = torch.empty((3, 5), dtype=torch.float32)
        b = torch.zeros(7, dtype=torch.float16, device="cpu")
        c = torch.empty_like(a)
        d = torch.zeros_like(b, dtype=torch.int32)
        s = torch.empty((), dtype=torch.float32)
        e = torch.empty(0)
        x = torch.arange(6.0).to("cpu")
        a.fill_(1.0), c.copy_(a), s.fill_(2.0)
        for t in (a, c, s):
            mc.assert_written(t)
        assert a.shape == (3, 5) and c.dtype == torch.float32 and s.dim() == 0 and e.numel() == 0
        assert float(b.float().abs().sum()) == 0.0 and d.dtype == torch.int32 and int(d.abs().sum()) == 0
        assert torch.equal(x, torch.arange(6.0))
        assert all(t.is_contiguous() and t.data_ptr() % 256 == 0 for t in (a, b, c, d, s, x))
    assert (mc.outputs, mc.workspaces, mc.uploads, mc.passthrough) == (6, 0, 1, 0)


def test_fill_is_nan_in_fp32_and_fp16_and_patterns_differ():
    with memory_contract(device="cpu") as mc:
        a, hq = torch.empty(8, dtype=torch.float32), torch.empty(8, dtype=torch.float16)
        assert bool(torch.isnan(a).all()) and bool(torch.isnan(hq).all())
        assert mc.first_unwritten(a) == 0 and mc.first_unwritten(hq) == 0
        x = torch.ones(4).to("cpu")
        buf, off = mc.raw(x)
        zone = buf[off - 16:off]
        assert bool(torch.isnan(zone.view(torch.float32)).all()) and bool(torch.isnan(zone.view(torch.float16)).all())
        assert zone.view(torch.int32)[0].item() == G.FILL_IN != G.FILL_OUT
        a.zero_(), hq.zero_()


@pytest.mark.parametrize("where,offset", [("before", -4), ("after", 0), ("far end before", -G.RED_ZONE), ("far end after", G.RED_ZONE - 4)])
@pytest.mark.parametrize("role", ["output", "upload"])
def test_store_in_a_red_zone_is_reported(where, offset, role):
    with pytest.raises(MemoryContractError) as ei:
        with memory_contract(device="cpu") as mc:
            t = torch.zeros((2, 5), dtype=torch.float32) if role == "output" else torch.ones((2, 5)).to("cpu")
            _poke(mc, t, offset if offset < 0 else t.numel() * 4 + offset)
    msg = str(ei.value)
    assert ("BEFORE" if offset < 0 else "AFTER") in msg and role in msg and "(2, 5)" in msg and "torch.float32" in msg
    assert __file__.rsplit("/", 1)[-1] in msg  # the call site
    assert f"byte offset {offset if offset < 0 else 40 + offset} " in msg


def test_store_just_past_an_odd_sized_half_tensor():
    """3 fp16 elements end 2 bytes short of a 4-byte word: the red zone starts at the tensor's last byte, not at the next word."""
    with pytest.raises(MemoryContractError, match="byte offset 6 "):
        with memory_contract(device="cpu") as mc:
            t = torch.zeros(3, dtype=torch.float16)
            buf, off = mc.raw(t)
            buf[off + 6:off + 8].view(torch.float16)[0] = 1.0


def test_unwritten_empty_is_nan_and_located():
    with memory_contract(device="cpu") as mc:
        y = torch.empty((4, 6), dtype=torch.float32)
        y[:3].fill_(0.5)  # the last row is never written
        assert mc.first_unwritten(y) == 18
        with pytest.raises(MemoryContractError, match="element 18 .*never written"):
            mc.assert_written(y)
        ref = torch.full((4, 6), 0.5)
        err = float((y - ref).norm() / ref.norm())  # what the parity tests compute: a NaN left in a result fails them
        assert not err <= 1e-3
        y[3].fill_(0.5)
        mc.assert_written(y)


def test_mutated_upload_is_reported_unless_exempt():
    src = torch.arange(12.0).reshape(3, 4)
    with pytest.raises(MemoryContractError, match=r"INPUT CHANGED: upload \(3, 4\).*\(element 5\)"):
        with memory_contract(device="cpu"):
            x = src.to("cpu")
            assert x.data_ptr() != src.data_ptr()
            x[1, 1] = -1.0
    with memory_contract(device="cpu", check_inputs=False) as mc:
        x = src.to("cpu")
        x[1, 1] = -1.0
    assert mc.uploads == 1 and float(src[1, 1]) == 5.0


def test_align16_is_16_and_not_32_byte_aligned():
    with memory_contract(device="cpu", align16=True) as mc:
        ts = [torch.empty(5), torch.zeros((2, 3), dtype=torch.float16), torch.empty_like(torch.ones(9)), torch.ones(3).to("cpu")]
        for t in ts:
            assert t.data_ptr() % 256 == 16
        for t in ts[:3]:
            t.zero_()
    assert mc.outputs == 3 and mc.uploads == 1


def test_workspace_has_no_slack():
    from mstg_hip import ops
    real = ops._ws
    assert real(100, "cpu").numel() * 4 > 100  # the real one always gives more than asked
    with memory_contract(device="cpu") as mc:
        for asked, got in ((0, 16), (16, 16), (100, 100), (101, 104), (4096, 4096)):
            ws = ops._ws(asked, "cpu")
            assert ws.dtype == torch.float32 and ws.numel() * 4 == got and bool(torch.isnan(ws).all())
        assert mc.workspaces == 5 and mc.outputs == 0
    assert ops._ws is real
    with pytest.raises(MemoryContractError, match=r"AFTER workspace \(25,\)"):
        with memory_contract(device="cpu") as mc:
            ws = ops._ws(100, "cpu")
            _poke(mc, ws, 100)  # the first byte the real _ws would still have owned


def test_pass_through_is_recorded_with_its_call_site():
    with memory_contract(device="cpu") as mc:
        out = torch.empty(3)
        a = torch.empty(3, out=out)
        b = torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
        c = torch.empty_like(torch.ones(4, 6).t())
        d = torch.zeros_like(torch.ones(4, 6).t())
        e = torch.ones(2, requires_grad=True).to("cpu", torch.float64)  # autograd tracks it
        out.zero_()
    assert mc.outputs == 1 and mc.uploads == 0 and mc.passthrough == 5
    assert [p[0] for p in mc.passed] == ["torch.empty", "torch.empty", "torch.empty_like", "torch.zeros_like", "Tensor.to"]
    assert all(p[1][0] == __file__ for p in mc.passed) and e.requires_grad and not d.is_contiguous()
    assert not c.is_contiguous() and a.data_ptr() == out.data_ptr() and b.is_contiguous(memory_format=torch.channels_last)


def test_library_pass_through_is_a_violation(tmp_path):
    """an unguarded allocation on the guarded device from a file under mstg_hip/ fails the context"""
    pkg = tmp_path / "mstg_hip"
    pkg.mkdir()
    src = pkg / "fake_layer.py"
    src.write_text("import torch\n\ndef alloc():\n    return torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)\n")
    scope = {}
    exec(compile(src.read_text(), str(src), "exec"), scope)
    with pytest.raises(MemoryContractError, match=r"UNGUARDED allocation by the library: torch.empty at .*fake_layer.py:4"):
        with memory_contract(device="cpu"):
            scope["alloc"]()


def test_everything_is_restored_after_an_exception():
    from mstg_hip import ops
    before = (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like, torch.Tensor.to, torch.Tensor.cuda, ops._ws)
    in_dict = ("to" in vars(torch.Tensor), "cuda" in vars(torch.Tensor))
    with pytest.raises(ZeroDivisionError):
        with memory_contract(device="cpu") as mc:
            assert torch.empty is not before[0] and torch.Tensor.to is not before[4] and ops._ws is not before[6]
            t = torch.zeros(4)
            _poke(mc, t, 16)  # a violation too: the block's own exception is the one that is reported
            1 / 0
    assert (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like, torch.Tensor.to, torch.Tensor.cuda, ops._ws) == before
    assert ("to" in vars(torch.Tensor), "cuda" in vars(torch.Tensor)) == in_dict
    with pytest.raises(RuntimeError, match="does not nest"):
        with memory_contract(device="cpu"):
            with memory_contract(device="cpu"):
                pass
    assert torch.empty is before[0] and ops._ws is before[6]
    with memory_contract(device="cpu") as mc:  # and it is usable again
        torch.zeros(2)
    assert mc.outputs == 1
