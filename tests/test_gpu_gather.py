"""GPU: ``mpv_gather_batch`` (csrc/gather.hip) against ``src[order[p : p + B]]``
(``.float()`` where cast), bit for bit: every element type into fp32 and into
itself, one to four sources per launch, the 16-byte path and the element path,
orders with repeats / reversed / NULL, the device cursor, out-of-range rows,
guard bands round everything the kernel may write, and the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import guarded_alloc
import mpvae_hip as H
from guarded_alloc import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64 << 10  # > the 3 rows past B a 4-row workgroup could reach, at 130 fp64 columns

ELEMS = {H.EL_F32: torch.float32, H.EL_F64: torch.float64, H.EL_I32: torch.int32,
         H.EL_I64: torch.int64, H.EL_U8: torch.uint8}
ALL_COLS = [1, 3, 4, 5, 25, 100, 130]


def _guarded():
    return guarded_alloc.GuardedTorch(torch, GUARD, GUARD)


def _values(n_rows, cols, elem, rng):
    """(n_rows, cols) CPU tensor of the element type: random values with the
    ones whose cast to fp32 rounds (or cannot be held) up front."""
    dt, n = ELEMS[elem], n_rows * cols
    if elem == H.EL_F64:
        special = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 - 2.0 ** -25, 1e-310, 1e-40, -1e-46,
                   float("inf"), float("-inf"), float("nan"), 1e300, -0.0, 16777217.0]
        v = torch.from_numpy(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n))
    elif elem == H.EL_F32:
        special = [float("inf"), float("-inf"), float("nan"), 1e-40, -0.0]
        v = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    elif elem == H.EL_I64:
        special = [2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24) - 1, 2 ** 53 + 1, 2 ** 63 - 1, -2 ** 63,
                   2 ** 62 + 2 ** 38]
        v = torch.from_numpy(rng.integers(-2 ** 40, 2 ** 40, n))
    elif elem == H.EL_I32:
        special = [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, -2 ** 31, -(2 ** 24) - 1]
        v = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32))
    else:
        special = [0, 1, 255, 128]
        v = torch.from_numpy(rng.integers(0, 256, n).astype(np.uint8))
    k = min(n, len(special))
    v[rng.permutation(n)[:k]] = torch.tensor(special[:k], dtype=dt)
    return v.reshape(n_rows, cols)


def _shifted(g, like, role):
    """A guarded tensor shaped like ``like`` whose base sits one element past a
    16-B boundary: the kernel has to take its element path."""
    flat = torch.zeros(like.numel() + 1, dtype=like.dtype)
    flat[1:] = like.reshape(-1)
    t = g.alloc_like(flat.to(DEV), role)[1:].view(like.shape)
    assert t.data_ptr() % 16 == like.element_size()
    return t


class Call:
    """One mpv_gather_batch call on guarded buffers and its torch reference."""

    def __init__(self, g, sources, n_rows, shift_src=False, shift_dst=False):
        """sources: [(cols, src_elem, cast to fp32?)]."""
        self.g, self.n_rows, self.sources = g, n_rows, sources
        self.shift_src, self.shift_dst = shift_src, shift_dst
        rng = np.random.default_rng(n_rows * 1000 + len(sources))
        self.host = [_values(n_rows, c, e, rng) for c, e, _ in sources]
        self.src = [_shifted(g, h, "input") if shift_src else g.alloc_like(h.to(DEV))
                    for h in self.host]
        self.bad = g.zeros(1, dtype=torch.uint8, device=DEV)

    def run(self, order, B, start=0, pos=None, advance=0, n_idx=None):
        g = self.g
        idx = None if order is None else g.alloc_like(
            torch.as_tensor(order, dtype=torch.int64).to(DEV))
        n_idx = (self.n_rows if order is None else len(order)) if n_idx is None else n_idx
        dts = [torch.float32 if cast else ELEMS[e] for _, e, cast in self.sources]
        if self.shift_dst:
            self.dst = [_shifted(g, torch.zeros((B, c), dtype=dt), "output")
                        for (c, _, _), dt in zip(self.sources, dts)]
        else:
            self.dst = [g.empty((B, c), dtype=dt, device=DEV)
                        for (c, _, _), dt in zip(self.sources, dts)]
        a = H.GatherArgs(n_sources=len(self.sources), n_rows=self.n_rows, idx=H.ptr(idx),
                         n_idx=n_idx, B=B, start=start, pos=H.ptr(pos), advance=advance,
                         bad=H.ptr(self.bad))
        for k, ((c, e, cast), s, d) in enumerate(zip(self.sources, self.src, self.dst)):
            a.src[k], a.src_elem[k], a.cols[k] = s.data_ptr(), e, c
            a.dst[k], a.dst_elem[k] = d.data_ptr(), H.EL_F32 if cast else e
        H.check(H.load_library().mpv_gather_batch(ctypes.byref(a), H.stream_of(DEV)),
                "mpv_gather_batch")
        return self.dst

    def want(self, rows):
        """The reference for good rows ``rows`` (source row indices)."""
        rows = torch.as_tensor(rows, dtype=torch.int64)
        return [h[rows].float() if cast else h[rows]
                for h, (_, _, cast) in zip(self.host, self.sources)]

    def assert_equal(self, rows, what=""):
        for k, (d, w) in enumerate(zip(self.dst, self.want(rows))):
            assert same_bits(d.cpu(), w), (what, k, self.sources[k])


def _orders(n_rows, B, rng):
    """name -> (order or None, start): with repeats, reversed, identity."""
    out = {"repeats": (rng.integers(0, n_rows, B + 5), 3),
           "reversed": (np.arange(max(n_rows, B))[::-1] % n_rows, 0)}
    if n_rows >= B:
        out["identity"] = (None, n_rows - B)
    return out


# ------------------------------------------------------------- 1. the grid
@pytest.mark.parametrize("B", [1, 3, 64, 65, 257])
@pytest.mark.parametrize("n_rows", [1, 7, 300])
def test_gather_equals_indexing_for_every_type_and_width(n_rows, B):
    """Every (cols, src_elem, dst_elem) of the grid, four sources per launch."""
    rng = np.random.default_rng(7 * n_rows + B)
    configs = [(c, e, cast) for e in ELEMS for cast in (True, False) for c in ALL_COLS]
    order_of = _orders(n_rows, B, rng)
    names = list(order_of)
    g = _guarded()
    for i in range(0, len(configs), H.GATHER_MAX_SOURCES):
        call = Call(g, configs[i:i + H.GATHER_MAX_SOURCES], n_rows)
        name = names[(i // H.GATHER_MAX_SOURCES) % len(names)]
        order, start = order_of[name]
        call.run(order, B, start=start)
        rows = np.arange(start, start + B) if order is None else order[start:start + B]
        call.assert_equal(rows, (name, i))
        assert int(call.bad) == 0
    g.assert_clean()


@pytest.mark.parametrize("n_sources", [1, 3, 4])
def test_mixed_sources_in_one_call(n_sources):
    mix = [(25, H.EL_U8, True), (100, H.EL_F32, False), (3, H.EL_I64, False),
           (130, H.EL_F64, True)][:n_sources]
    g = _guarded()
    rng = np.random.default_rng(n_sources)
    for n_rows, B in ((7, 65), (300, 257), (300, 3)):
        for name, (order, start) in _orders(n_rows, B, rng).items():
            call = Call(g, mix, n_rows)
            call.run(order, B, start=start)
            rows = np.arange(start, start + B) if order is None else order[start:start + B]
            call.assert_equal(rows, (n_rows, B, name))
            assert int(call.bad) == 0
    g.assert_clean()


@pytest.mark.parametrize("shift", ["src", "dst", "both", "none"])
def test_aligned_and_shifted_bases_give_the_same_bytes(shift):
    """fp32 -> fp32 with cols % 4 == 0 on aligned bases is the 16-byte path (and
    so are the raw copies of 8-B elements with even cols and of uint8 with cols %
    16 == 0); a base one element off a 16-B boundary forces the element path."""
    mix = [(4, H.EL_F32, False), (100, H.EL_F32, True), (16, H.EL_U8, False),
           (4, H.EL_I64, False)]
    g = _guarded()
    rng = np.random.default_rng(3)
    for n_rows, B in ((7, 3), (300, 65), (300, 257)):
        order = rng.integers(0, n_rows, B)
        call = Call(g, mix, n_rows, shift_src=shift in ("src", "both"),
                    shift_dst=shift in ("dst", "both"))
        if shift == "none":
            assert all(t.data_ptr() % 16 == 0 for t in call.src)
        call.run(order, B)
        call.assert_equal(order, (n_rows, B))
        assert int(call.bad) == 0
    g.assert_clean()


# --------------------------------------------------------------- 2. cursor
def test_device_cursor_and_advance():
    g = _guarded()
    n_rows, B = 300, 65
    mix = [(5, H.EL_F64, True), (100, H.EL_F32, False), (3, H.EL_I32, False)]
    order = np.random.default_rng(5).permutation(n_rows)[:3 * B + 10]
    call = Call(g, mix, n_rows)
    by_start = [d.clone() for d in call.run(order, B, start=B)]
    pos = g.zeros(1, dtype=torch.int64, device=DEV)
    pos.fill_(B)
    by_pos = call.run(order, B, start=12345, pos=pos)  # start is not read
    assert all(same_bits(a, b) for a, b in zip(by_start, by_pos))
    assert int(pos) == B  # no advance: unchanged
    pos.zero_()
    for i in range(3):  # three chained calls walk the order
        call.run(order, B, pos=pos, advance=1)
        call.assert_equal(order[i * B:(i + 1) * B], i)
        assert int(pos) == (i + 1) * B
    call.run(order, 10, pos=pos)  # the ragged tail at the cursor
    call.assert_equal(order[3 * B:], "tail")
    assert int(pos) == 3 * B and int(call.bad) == 0
    g.assert_clean()


# --------------------------------------------------------- 3. out of range
def _assert_poisoned(call, bad, good, good_rows, what):
    """Batch rows ``bad`` are NaN / 0, rows ``good`` hold source rows ``good_rows``."""
    want = call.want(good_rows)
    for k, d in enumerate(call.dst):
        d = d.cpu()
        assert same_bits(d[good], want[k]), (what, k)
        if d.dtype.is_floating_point:
            assert torch.isnan(d[bad]).all(), (what, k)
        else:
            assert (d[bad] == 0).all(), (what, k)


@pytest.mark.parametrize("B", [4, 65])
def test_out_of_range_rows_are_poisoned_and_flagged(B):
    g = _guarded()
    n_rows = 7
    mix = [(5, H.EL_F64, True), (4, H.EL_F32, False), (3, H.EL_I64, False), (16, H.EL_U8, False)]
    rng = np.random.default_rng(B)
    order = rng.integers(0, n_rows, B)
    order[1], order[2] = -1, n_rows
    call = Call(g, mix, n_rows)
    call.run(order, B, start=1)  # the batch's last row is position B = n_idx
    bad = [0, 1, B - 1]
    good = [r for r in range(B) if r not in bad]
    _assert_poisoned(call, bad, good, order[1:][[r for r in good]], "indices")
    assert int(call.bad) == 1
    call.run(np.zeros(B, np.int64), B)  # a clean call never clears the flag
    assert int(call.bad) == 1
    call.bad.zero_()
    call.run(np.zeros(B, np.int64), B)
    assert int(call.bad) == 0
    # positions before the order, and at the ends of the int64 range (no wrap-around)
    for start in (-1, -2 ** 63, 2 ** 63 - 1):
        call.run(None, B, start=start)
        good = [r for r in range(B) if 0 <= start + r < n_rows]
        bad = [r for r in range(B) if r not in good]
        _assert_poisoned(call, bad, good, [start + r for r in good], start)
        assert int(call.bad) == 1
        call.bad.zero_()
    g.assert_clean()


# ------------------------------------------------------- 4. argument checks
def test_bad_arguments_launch_nothing():
    lib = H.load_library()
    g = _guarded()
    src = g.alloc_like(torch.arange(12, dtype=torch.float32, device=DEV).reshape(3, 4))
    dst = g.alloc_like(torch.full((2, 4), -7.0, device=DEV), "output")
    bad = g.zeros(1, dtype=torch.uint8, device=DEV)
    pos = g.zeros(1, dtype=torch.int64, device=DEV)

    def call(n_sources=1, src_p=src, dst_p=dst, se=H.EL_F32, de=H.EL_F32, cols=4, B=2,
             pos_p=None, advance=0, bad_p=bad):
        a = H.GatherArgs(n_sources=n_sources, n_rows=3, idx=None, n_idx=3, B=B, start=0,
                         pos=H.ptr(pos_p), advance=advance, bad=H.ptr(bad_p))
        for k in range(min(max(n_sources, 0), H.GATHER_MAX_SOURCES)):
            a.src[k], a.dst[k] = H.ptr(src_p), H.ptr(dst_p)
            a.src_elem[k], a.dst_elem[k], a.cols[k] = se, de, cols
        return lib.mpv_gather_batch(ctypes.byref(a), H.stream_of(DEV))

    lib.mpv_timing_enable(1)
    lib.mpv_timing_reset()
    try:
        for kw, msg in ((dict(n_sources=0), b"sources"), (dict(n_sources=5), b"sources"),
                        (dict(B=0), b"B must be"), (dict(cols=0), b"cols"),
                        (dict(src_p=None), b"NULL"), (dict(dst_p=None), b"NULL"),
                        (dict(bad_p=None), b"NULL"), (dict(se=H.EL_F32, de=H.EL_I32), b"dst_elem"),
                        (dict(se=H.EL_I64, de=H.EL_F64), b"dst_elem"),
                        (dict(se=5, de=H.EL_F32), b"element type"),
                        (dict(advance=1), b"advance")):
            assert call(**kw) == H.EINVAL, kw
            assert msg in lib.mpv_last_error(), (kw, lib.mpv_last_error())
        assert not H.kernel_times()
        torch.cuda.synchronize()
        assert bool((dst == -7).all()) and int(bad) == 0 and int(pos) == 0
        assert call(pos_p=pos, advance=1) == 0  # the good call: the gather and the cursor launch
        torch.cuda.synchronize()
        assert H.kernel_times()["gather_batch"][0] == 2
    finally:
        lib.mpv_timing_enable(0)
    assert torch.equal(dst, src[:2]) and int(pos) == 2 and int(bad) == 0
    # mpv_group_rows still rejects the element type it does not know
    out = torch.empty(3, dtype=torch.int32, device=DEV)
    flag = torch.empty((), dtype=torch.bool, device=DEV)
    u8 = torch.zeros((3, 2), dtype=torch.uint8, device=DEV)
    assert lib.mpv_group_rows(H.ptr(u8), H.EL_U8, 3, 2, 3, H.ptr(out), H.ptr(out), H.ptr(out),
                              H.ptr(flag), H.stream_of(DEV)) == H.EINVAL
    g.assert_clean()
