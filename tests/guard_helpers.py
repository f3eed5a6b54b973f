"""Red zones around every tensor the project's Python layer allocates and every tensor a test uploads.

``memory_contract()`` is a context manager.  While it is active

* ``torch.empty`` / ``torch.empty_like`` / ``torch.zeros`` / ``torch.zeros_like`` for the guarded device (contiguous layout, plain
  arguments) and ``mstg_hip.ops._ws`` return tensors that live inside a buffer this module owns::

      [ red zone 64 KiB | interior | red zone 64 KiB ]

  The interior starts 256-byte aligned, or -- ``align16=True`` -- 16 bytes past a 256-byte boundary: 16-byte aligned and not
  32-byte aligned, the least include/mstg_hip.h promises.  Red zones and the interior of ``empty`` allocations hold the byte 0xFF
  (a quiet NaN as fp32 and as fp16), ``zeros`` get a zero interior;
* ``Tensor.to`` / ``Tensor.cuda`` from a CPU tensor to a contiguous tensor on the guarded device return a guarded copy whose red
  zones hold a SECOND NaN pattern (0x7FC17FC1), so that a value copied from past the end of an input to past the end of an output
  does not recreate the output's own pattern; a host clone of the uploaded bits is kept;
* the patched ``_ws`` hands out exactly ``max(nbytes, 16)`` rounded up to 4 bytes -- none of the 4 to 7 bytes of slack of the real
  one.  An entry that then answers MSTG_E_WORKSPACE has a workspace query that under-reports: fix the library, not this file;
* anything else those functions are asked for (another device, pinned memory, another memory format, ``out=``, a non-contiguous
  ``empty_like``, an upload that autograd tracks) is passed through unchanged and recorded with its call site.

On exit every patch is restored (also after an exception), the device is synchronised, and -- unless the block itself raised --
a ``MemoryContractError`` names, with shape, dtype, role, call site and the first bad byte offset relative to the tensor,

* every red zone that no longer holds its pattern;
* with ``check_inputs=True`` every uploaded tensor that is not bit-identical to its host clone;
* every pass-through allocation on the guarded device that came from a file under ``mstg_hip/``.

``outputs`` / ``workspaces`` / ``uploads`` / ``passthrough`` count what happened, so that a test can assert the guard engaged.
``first_unwritten(t)`` / ``assert_written(t)`` look for elements of an ``empty`` tensor that still hold the fill; a parity test
needs neither, a NaN left in a result fails its relative L2 by itself.

Limits
* 64 KiB is a choice, not a measurement: it covers a 32-pixel x 64-channel fp32 tile row eight times over.  A store further out
  than 64 KiB from the tensor is NOT detected.
* Allocations made inside ATen are not reached: ``clone``, ``contiguous``, ``torch.tensor(..., device=)``, autograd's own buffers
  (the gradient a backward receives, ``.grad``).  Nothing further is patched.
* Do not use it around HIP graph capture (``torch.cuda.graph``): the fills would be captured.
* The patches are process-wide, because autograd runs ``backward()`` on another thread; contexts do not nest.
* Every guarded buffer stays alive until the context exits, so nothing inside it ever receives recycled memory.
"""
import os
import sys

import torch

RED_ZONE = 64 * 1024
FILL_OUT = 0xFFFFFFFF  # the byte 0xFF: outputs, workspaces and their red zones
FILL_IN = 0x7FC17FC1   # red zones of uploaded inputs
_HERE = os.path.abspath(__file__)
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__)) + os.sep
_ACTIVE = [None]


class MemoryContractError(AssertionError):
    pass


def _as_i32(pattern):
    return pattern - (1 << 32) if pattern >= (1 << 31) else pattern


def _site():
    """(file, line) of the nearest caller outside this module and outside torch."""
    f = sys._getframe(2)
    while f is not None:
        fn = os.path.abspath(f.f_code.co_filename)
        if fn != _HERE and not fn.startswith(_TORCH_DIR):
            return fn, f.f_lineno
        f = f.f_back
    return "?", 0


def _plain_size(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    if all(type(a) is int and a >= 0 for a in args):
        return tuple(args)
    return None


class _Record:
    __slots__ = ("buf", "off", "nbytes", "shape", "dtype", "role", "site", "pattern", "host")

    def describe(self):
        return f"{self.role} {tuple(self.shape)} {self.dtype} allocated at {self.site[0]}:{self.site[1]}"


class memory_contract:
    def __init__(self, align16=False, check_inputs=True, device="cuda:0"):
        self.align16, self.check_inputs, self.device = bool(align16), bool(check_inputs), torch.device(device)
        self.outputs = self.workspaces = self.uploads = self.passthrough = 0
        self.passed = []  # (what, site, device type or None)
        self._records, self._expect, self._saved = [], {}, []

    # ------------------------------------------------------------------------------------------------------ allocation
    def _on_device(self, dev):
        if dev is None:
            dev = torch.get_default_device()
        return torch.device(dev).type == self.device.type

    def _alloc(self, shape, dtype, role, site, pattern, device=None, zero=False):
        nbytes = dtype.itemsize
        for s in shape:
            nbytes *= s
        total = (RED_ZONE + 272 + nbytes + RED_ZONE + 7) // 4 * 4
        buf = self._orig["empty"](total, dtype=torch.uint8, device=device if device is not None else self.device)
        buf.view(torch.int32).fill_(_as_i32(pattern))
        want = 16 if self.align16 else 0
        off = RED_ZONE + (want - (buf.data_ptr() + RED_ZONE)) % 256
        interior = buf[off:off + nbytes]
        if zero:
            interior.zero_()
        r = _Record()
        r.buf, r.off, r.nbytes, r.shape, r.dtype, r.role, r.site, r.pattern, r.host = buf, off, nbytes, tuple(shape), dtype, role, site, pattern, None
        self._records.append(r)
        t = interior.view(dtype).view(tuple(shape))
        assert nbytes == 0 or (t.data_ptr() % 256 == want and t.data_ptr() == buf.data_ptr() + off)
        return t, r

    def _pass(self, what, site, result):
        self.passthrough += 1
        dev = result.device.type if isinstance(result, torch.Tensor) else None
        self.passed.append((what, site, dev))
        return result

    def _new(self, name, zero):
        orig = self._orig[name]

        def fn(*args, **kw):
            size = _plain_size(args)
            extra = {k: v for k, v in kw.items() if k not in ("dtype", "device", "requires_grad")}
            plain = (size is not None and (extra.get("pin_memory", False) is False) and extra.get("layout", torch.strided) is torch.strided
                     and extra.get("memory_format", torch.contiguous_format) is torch.contiguous_format
                     and set(extra) <= {"pin_memory", "layout", "memory_format"})
            if not plain or not self._on_device(kw.get("device")):
                return self._pass(f"torch.{name}", _site(), orig(*args, **kw))
            dtype = kw.get("dtype") or torch.get_default_dtype()
            t, _ = self._alloc(size, dtype, "output", _site(), FILL_OUT, kw.get("device"), zero)
            self.outputs += 1
            return t.requires_grad_() if kw.get("requires_grad") else t
        return fn

    def _like(self, name, zero):
        orig = self._orig[name]

        def fn(x, *args, **kw):
            extra = set(kw) - {"dtype", "device", "requires_grad", "memory_format"}
            plain = (not args and not extra and type(x) in (torch.Tensor, torch.nn.Parameter) and x.layout is torch.strided
                     and x.is_contiguous() and kw.get("memory_format", torch.preserve_format) in (torch.preserve_format, torch.contiguous_format))
            dev = kw.get("device") if plain and kw.get("device") is not None else (x.device if plain else None)
            if not plain or not self._on_device(dev):
                return self._pass(f"torch.{name}", _site(), orig(x, *args, **kw))
            t, _ = self._alloc(tuple(x.shape), kw.get("dtype") or x.dtype, "output", _site(), FILL_OUT, dev, zero)
            self.outputs += 1
            return t.requires_grad_() if kw.get("requires_grad") else t
        return fn

    def _ws(self, nbytes, device):
        n = (max(int(nbytes), 16) + 3) // 4
        t, _ = self._alloc((n,), torch.float32, "workspace", _site(), FILL_OUT, device)
        self.workspaces += 1
        return t

    def upload(self, src, result=None, site=None):
        """A guarded copy of ``result`` (default: of the CPU tensor ``src`` itself) on the guarded device."""
        site = site or _site()
        r = src if result is None else result
        t, rec = self._alloc(tuple(r.shape), r.dtype, "upload", site, FILL_IN, r.device if r.device.type == self.device.type else None)
        t.copy_(r)
        rec.host = r.detach().cpu().clone()
        self.uploads += 1
        return t

    def _moved(self, name):
        orig = self._orig[name]

        def fn(x, *args, **kw):
            r = orig(x, *args, **kw)
            named = name == "cuda" or "device" in kw or any(isinstance(a, (str, torch.device, int, torch.Tensor)) and not isinstance(a, bool) for a in args)
            if not (isinstance(x, torch.Tensor) and isinstance(r, torch.Tensor) and x.device.type == "cpu" and named
                    and r.device.type == self.device.type):
                return r  # not an upload at all (a dtype change, a move between other devices)
            if type(r) is not torch.Tensor or r.requires_grad or r.layout is not torch.strided or not r.is_contiguous():
                return self._pass(f"Tensor.{name}", _site(), r)
            return self.upload(x, r, _site())
        return fn

    # ------------------------------------------------------------------------------------------------------ lookups for tests
    def _find(self, t):
        p = t.data_ptr()
        for r in self._records:
            if r.buf.data_ptr() + r.off == p and r.nbytes == t.numel() * t.element_size():
                return r
        raise KeyError("not a tensor this guard allocated")

    def raw(self, t):
        """(the owning uint8 buffer, byte offset of ``t`` in it): for a test that writes into the red zone it owns."""
        r = self._find(t)
        return r.buf, r.off

    def first_unwritten(self, t):
        """Index of the first element of an ``empty`` tensor that still holds the fill (every byte 0xFF), or None."""
        r = self._find(t)
        it = r.dtype.itemsize
        words = r.buf[r.off:r.off + r.nbytes].view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[it])
        bad = (words == -1).nonzero()
        return int(bad[0]) if bad.numel() else None

    def assert_written(self, t):
        i = self.first_unwritten(t)
        if i is not None:
            raise MemoryContractError(f"element {i} of {self._find(t).describe()} was never written")

    # ------------------------------------------------------------------------------------------------------ enter / exit
    def __enter__(self):
        if _ACTIVE[0] is not None:
            raise RuntimeError("memory_contract does not nest")
        _ACTIVE[0] = self
        self._orig = {n: getattr(torch, n) for n in ("empty", "empty_like", "zeros", "zeros_like")}
        self._orig["to"], self._orig["cuda"] = torch.Tensor.to, torch.Tensor.cuda
        try:
            from mstg_hip import ops
        except ImportError:
            ops = None

        def patch(obj, name, new):
            had = name in vars(obj)
            self._saved.append((obj, name, had, vars(obj).get(name)))
            setattr(obj, name, new)
        try:
            patch(torch, "empty", self._new("empty", False))
            patch(torch, "zeros", self._new("zeros", True))
            patch(torch, "empty_like", self._like("empty_like", False))
            patch(torch, "zeros_like", self._like("zeros_like", True))
            patch(torch.Tensor, "to", self._moved("to"))
            patch(torch.Tensor, "cuda", self._moved("cuda"))
            if ops is not None:
                patch(ops, "_ws", self._ws)
        except BaseException:
            self._restore()
            raise
        return self

    def _restore(self):
        while self._saved:
            obj, name, had, old = self._saved.pop()
            if had:
                setattr(obj, name, old)
            else:
                delattr(obj, name)
        _ACTIVE[0] = None

    def __exit__(self, etype, exc, tb):
        try:
            if self.device.type == "cuda":
                torch.cuda.synchronize()
        finally:
            self._restore()
        if etype is None:
            problems = self.violations()
            self._records = []
            if problems:
                raise MemoryContractError(f"{len(problems)} violation(s) of the memory contract:\n  " + "\n  ".join(problems[:20]))
        self._records = []
        return False

    # ------------------------------------------------------------------------------------------------------ checks
    def _expected(self, pattern, device, phase):
        key = (pattern, str(device))
        if key not in self._expect:
            e = self._orig["empty"](RED_ZONE + 8, dtype=torch.uint8, device=device)
            e.view(torch.int32).fill_(_as_i32(pattern))
            self._expect[key] = e
        return self._expect[key][phase:phase + RED_ZONE]

    def violations(self):
        out, flags = [], []
        for r in self._records:
            front = r.buf[r.off - RED_ZONE:r.off]
            end = r.off + r.nbytes
            back = r.buf[end:end + RED_ZONE]
            fe, be = self._expected(r.pattern, r.buf.device, (r.off - RED_ZONE) % 4), self._expected(r.pattern, r.buf.device, end % 4)
            flags.append(torch.stack([front.ne(fe).any(), back.ne(be).any()]))
        bad = torch.stack(flags).cpu().tolist() if flags else []
        for r, (f, b) in zip(self._records, bad):
            if f:
                i = int(r.buf[r.off - RED_ZONE:r.off].ne(self._expected(r.pattern, r.buf.device, (r.off - RED_ZONE) % 4)).nonzero()[0])
                out.append(f"store BEFORE {r.describe()}: byte offset {i - RED_ZONE} (element {(i - RED_ZONE) // r.dtype.itemsize})")
            if b:
                end = r.off + r.nbytes
                i = int(r.buf[end:end + RED_ZONE].ne(self._expected(r.pattern, r.buf.device, end % 4)).nonzero()[0])
                out.append(f"store AFTER {r.describe()}: byte offset {r.nbytes + i} (element {(r.nbytes + i) // r.dtype.itemsize}, "
                           f"{i} bytes past the end)")
        if self.check_inputs:
            for r in self._records:
                if r.host is None:
                    continue
                now = r.buf[r.off:r.off + r.nbytes].cpu()
                was = r.host.reshape(-1).view(torch.uint8)
                if not torch.equal(now, was):
                    i = int(now.ne(was).nonzero()[0])
                    out.append(f"INPUT CHANGED: {r.describe()}: first at byte offset {i} (element {i // r.dtype.itemsize})")
        for what, site, dev in self.passed:
            if dev == self.device.type and (os.sep + "mstg_hip" + os.sep) in site[0]:
                out.append(f"UNGUARDED allocation by the library: {what} at {site[0]}:{site[1]}")
        return out
