"""A test-only guarded allocator: guard bands round what a product module
allocates, to catch the store a kernel should not make.

A store past the end of an output or workspace does not fault (torch's caching
allocator packs blocks and rounds each to 512 B) and does not change the value
under test: it corrupts whichever tensor sits next door.  ``GuardedTorch``
stands in for the module-level name ``torch`` of one product module
(``guard(monkeypatch, mpvae_ops)``); its ``empty``, ``empty_like``, ``zeros``
and ``zeros_like`` carve their result out of a larger ``uint8`` arena

    [ front guard 0xA5 | body (nbytes) | slack to 512 B, back guard 0xA5 ]

and every other attribute is torch's own.  The body of ``empty*`` is filled
with 0xFF (NaN in fp32 and fp64: the poison of ``HipShardBackend._buf``), that
of ``zeros*`` with 0.  ``front`` and ``back`` are multiples of 512, so the body
keeps the 512-B alignment the allocator gives (kernels that pick a path by
pointer alignment take the one they take in production).

``check()`` counts the guard bytes that no longer hold 0xA5, and the bytes of
every tensor registered as an input (``alloc_like``) that changed.  A write
beyond the guards is not seen.
"""
from typing import NamedTuple, Optional

import torch as _torch

GUARD_BYTE = 0xA5
POISON_BYTE = 0xFF
ALIGN = 512
# on the GPU: back covers one 256-row output tile at the widest row pitch of the
# suite's shapes (256 x 4120 B at L = 1030, 1.03 MiB); on the CPU 64 KiB each
GPU_FRONT, GPU_BACK = 256 << 10, 2 << 20
CPU_FRONT = CPU_BACK = 64 << 10

_PASS = object()   # a call form this helper does not guard


def _round_up(n, m):
    return (n + m - 1) // m * m


class Offender(NamedTuple):
    shape: tuple
    dtype: object
    offset: int      # bytes relative to the body's start; negative: before the buffer
    where: str       # "guard" or "input"


class Report(NamedTuple):
    n_buffers: int
    n_bad_bytes: int
    first: Optional[Offender]


class _Record:
    def __init__(self, arena, nbytes, shape, dtype, role):
        self.arena, self.nbytes, self.shape, self.dtype, self.role = \
            arena, nbytes, tuple(shape), dtype, role
        self.snapshot = None
        self.own = False     # allocated by the test (alloc_like), not by the product


class GuardedTorch:
    """torch, but for empty / empty_like / zeros / zeros_like (see the module
    docstring).  ``records`` lists the guarded buffers in allocation order."""

    def __init__(self, real_torch, front, back):
        if front % ALIGN or back % ALIGN or front < 0 or back < 0:
            raise ValueError(f"front and back must be multiples of {ALIGN} (got {front}, {back})")
        self._torch, self.front, self.back = real_torch, int(front), int(back)
        self.records = []

    def __getattr__(self, name):   # everything not defined here is torch's own
        return getattr(self._torch, name)

    # ------------------------------------------------------------ allocation
    def _alloc(self, shape, dtype, device, fill, role="output"):
        t = self._torch
        shape = tuple(int(n) for n in shape)
        numel = 1
        for n in shape:
            numel *= n
        nbytes = numel * t.empty((), dtype=dtype).element_size()
        total = self.front + _round_up(nbytes, ALIGN) + self.back
        arena = t.empty(total, dtype=t.uint8, device=device)
        arena.fill_(GUARD_BYTE)
        body = arena[self.front:self.front + nbytes]
        body.fill_(fill)
        self.records.append(_Record(arena, nbytes, shape, dtype, role))
        return body.view(dtype).view(shape)

    def _shape_of(self, size):
        """The shape of torch.empty(*size) for an int, several ints, a tuple, a
        list or a torch.Size; _PASS for anything else."""
        if len(size) == 1 and isinstance(size[0], (tuple, list)):
            size = tuple(size[0])
        if not all(isinstance(n, int) and not isinstance(n, bool) for n in size):
            return _PASS
        return tuple(size)

    def _new(self, name, fill, size, kw):
        shape = self._shape_of(size) if size else _PASS
        if shape is _PASS or set(kw) - {"dtype", "device"}:
            return getattr(self._torch, name)(*size, **kw)
        dtype = kw.get("dtype")
        return self._alloc(shape, self._torch.get_default_dtype() if dtype is None else dtype,
                           kw.get("device"), fill)

    def _like(self, name, fill, args, kw):
        t = self._torch
        fmt = kw.get("memory_format", t.preserve_format)
        if (len(args) != 1 or not isinstance(args[0], t.Tensor)
                or set(kw) - {"dtype", "device", "memory_format"}
                or fmt not in (t.preserve_format, t.contiguous_format)
                or not args[0].is_contiguous() or args[0].layout != t.strided):
            return getattr(t, name)(*args, **kw)
        src = args[0]
        dtype = kw.get("dtype")
        device = kw.get("device")
        return self._alloc(src.shape, src.dtype if dtype is None else dtype,
                           src.device if device is None else device, fill)

    def empty(self, *size, **kw):
        return self._new("empty", POISON_BYTE, size, kw)

    def zeros(self, *size, **kw):
        return self._new("zeros", 0, size, kw)

    def empty_like(self, *args, **kw):
        return self._like("empty_like", POISON_BYTE, args, kw)

    def zeros_like(self, *args, **kw):
        return self._like("zeros_like", 0, args, kw)

    def alloc_like(self, tensor, role="input"):
        """A copy of `tensor` (contiguous, same dtype and device, no autograd
        history) in a guarded arena.  role "input": check() also holds its body
        bitwise unchanged; role "output": a tensor of the test's that the call
        under test may write (its guards alone are checked)."""
        if role not in ("input", "output"):
            raise ValueError(role)
        src = tensor.detach()
        out = self._alloc(src.shape, src.dtype, src.device, 0, role)
        out.copy_(src)
        rec = self.records[-1]
        rec.own = True
        if role == "input":
            rec.snapshot = rec.arena[self.front:self.front + rec.nbytes].clone()
        return out

    # ----------------------------------------------------------------- check
    def _regions(self, rec):
        f, n = self.front, rec.nbytes
        return rec.arena[:f], rec.arena[f + n:], rec.arena[f:f + n]

    def check(self):
        """Report(n_buffers, n_bad_bytes, first offender): the guard bytes that
        are not 0xA5 any more plus the changed bytes of the registered inputs,
        counted where the buffers live and read with one copy per device."""
        t = self._torch
        if t.cuda.is_available() and any(r.arena.is_cuda for r in self.records):
            t.cuda.synchronize()
        counts = {}
        for i, rec in enumerate(self.records):
            front, back, body = self._regions(rec)
            c = (front != GUARD_BYTE).sum() + (back != GUARD_BYTE).sum()
            if rec.snapshot is not None:
                c = c + (body != rec.snapshot).sum()
            counts.setdefault(rec.arena.device, []).append((i, c))
        bad = [0] * len(self.records)
        for items in counts.values():
            for (i, _), n in zip(items, t.stack([c for _, c in items]).tolist()):
                bad[i] = n
        n_bad = sum(bad)
        first = None
        if n_bad:
            rec = self.records[next(i for i, n in enumerate(bad) if n)]
            first = self._first_offence(rec)
        return Report(len(self.records), n_bad, first)

    def _first_offence(self, rec):
        front, back, body = self._regions(rec)
        hit = (front != GUARD_BYTE).nonzero()
        if hit.numel():
            return Offender(rec.shape, rec.dtype, int(hit[0]) - self.front, "guard")
        hit = (back != GUARD_BYTE).nonzero()
        if hit.numel():
            return Offender(rec.shape, rec.dtype, rec.nbytes + int(hit[0]), "guard")
        hit = (body != rec.snapshot).nonzero()
        return Offender(rec.shape, rec.dtype, int(hit[0]), "input")

    def assert_clean(self, min_buffers=0, what=""):
        """check() found nothing, over at least `min_buffers` guarded buffers
        (the test's own alloc_like tensors not counted)."""
        rep = self.check()
        assert rep.n_bad_bytes == 0, (what, rep)
        n = sum(1 for r in self.records if not r.own)
        assert n >= min_buffers, (what, f"{n} guarded allocations, expected >= {min_buffers}")
        return rep


def sizes_for(device):
    """(front, back) guard sizes for a device."""
    return (GPU_FRONT, GPU_BACK) if _torch.device(device).type == "cuda" else (CPU_FRONT, CPU_BACK)


def guard(monkeypatch, *modules, device="cpu", front=None, back=None):
    """Swap the module-level name ``torch`` of each product module for one
    GuardedTorch (undone by monkeypatch at the end of the test); returns it."""
    f, b = sizes_for(device)
    g = GuardedTorch(_torch, f if front is None else front, b if back is None else back)
    for m in modules:
        assert getattr(m, "torch") is _torch, f"{m.__name__}.torch is not torch"
        monkeypatch.setattr(m, "torch", g)
    return g


def same_bits(a, b):
    """a and b have the same shape and dtype, NaN at the same positions and the
    same bits everywhere else."""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if not a.dtype.is_floating_point:
        return _torch.equal(a, b)
    na, nb = _torch.isnan(a), _torch.isnan(b)
    if not _torch.equal(na, nb):
        return False
    bits = {2: _torch.int16, 4: _torch.int32, 8: _torch.int64}[a.element_size()]
    zero = _torch.zeros((), dtype=bits, device=a.device)
    return _torch.equal(_torch.where(na, zero, a.view(bits)), _torch.where(nb, zero, b.view(bits)))
