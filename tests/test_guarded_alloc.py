"""The guarded allocator of tests/guarded_alloc.py on the CPU: that it sees what
it should, and the host library (libmpvae_host.so) under its guards.

  * a byte written through the raw arena just behind a buffer, just before it
    and at the far end of the back guard is reported with its offset; an
    untouched buffer reports nothing; a registered input that changed is
    reported; the call forms the product uses are guarded and every other one
    passes through;
  * compute_loss + backward on CPU tensors with mpvae_host's allocations
    guarded, on four golden fixtures: no guard byte changes, the inputs stay as
    they were, and the eight outputs and every gradient equal the plain call's
    bit for bit.
"""
import pytest
import torch

import mpvae
import mpvae_host
from golden_io import DIFF, INPUTS, fixtures
from guarded_alloc import (CPU_BACK, CPU_FRONT, GUARD_BYTE, GuardedTorch, Offender, guard,
                           same_bits)

FIX = {f.name: f for f in fixtures()}


def _g():
    return GuardedTorch(torch, CPU_FRONT, CPU_BACK)


# ------------------------------------------------------------------ the helper
def test_layout_fill_and_alignment():
    g = _g()
    e = g.empty((3, 5), dtype=torch.float32)
    z = g.zeros(7, dtype=torch.float64)
    assert e.shape == (3, 5) and e.dtype == torch.float32 and e.is_contiguous()
    assert torch.isnan(e).all()                       # 0xFF bytes: the NaN poison
    assert z.shape == (7,) and not z.any()
    for t, rec in zip((e, z), g.records):
        nbytes = t.numel() * t.element_size()
        assert rec.nbytes == nbytes
        assert rec.arena.numel() == CPU_FRONT + (nbytes + 511) // 512 * 512 + CPU_BACK
        assert t.data_ptr() == rec.arena.data_ptr() + CPU_FRONT
        assert bool((rec.arena[:CPU_FRONT] == GUARD_BYTE).all())
        assert bool((rec.arena[CPU_FRONT + nbytes:] == GUARD_BYTE).all())
    assert g.check() == (2, 0, None)
    with pytest.raises(ValueError):
        GuardedTorch(torch, 100, 512)


def test_call_forms():
    g = _g()
    src = torch.arange(12, dtype=torch.float64).view(3, 4)
    guarded = [
        g.empty(4, dtype=torch.uint8), g.empty((), dtype=torch.float32),
        g.empty((2, 3), dtype=torch.int16, device="cpu"), g.empty(src.shape, dtype=torch.float32),
        g.empty(src.shape[1:], dtype=torch.float64), g.empty(2, 3), g.zeros(0, dtype=torch.int32),
        g.zeros((), dtype=torch.bool), g.zeros(2, dtype=torch.int64), g.empty_like(src),
        g.zeros_like(src, memory_format=torch.preserve_format),
        g.empty_like(src, dtype=torch.float32),
    ]
    shapes = [(4,), (), (2, 3), (3, 4), (4,), (2, 3), (0,), (), (2,), (3, 4), (3, 4), (3, 4)]
    assert [tuple(t.shape) for t in guarded] == shapes
    assert guarded[5].dtype == torch.get_default_dtype()
    assert guarded[9].dtype == torch.float64 and guarded[11].dtype == torch.float32
    assert not guarded[10].any()
    assert len(g.records) == len(guarded)
    # every other form and every other function is torch's own, unguarded
    out = torch.empty(3)
    passed = [g.empty(3, out=out), g.empty(3, pin_memory=False), g.zeros(3, requires_grad=True),
              g.empty_like(src.t()), g.full((2,), 1.0), g.tensor([1.0]), g.ones(2),
              g.ones_like(src)]
    assert len(g.records) == len(guarded) and len(passed) == 8
    assert g.float32 is torch.float32 and g.Tensor is torch.Tensor and g.autograd is torch.autograd
    assert g.check().n_bad_bytes == 0


@pytest.mark.parametrize("nbytes_of", [1024, 12])   # a whole number of 512-B blocks, and not
def test_a_stray_byte_is_reported_with_its_offset(nbytes_of):
    def one(off_in_arena):
        g = _g()
        t = g.empty(nbytes_of // 4, dtype=torch.float32)
        other = g.empty(5, dtype=torch.float64)
        arena = g.records[0].arena
        arena[off_in_arena] = 0
        t.fill_(1.0), other.fill_(2.0)                 # writes inside the bodies are no offence
        return g.check(), g.records[0]

    body_start, body_end = CPU_FRONT, CPU_FRONT + nbytes_of
    arena_end = CPU_FRONT + (nbytes_of + 511) // 512 * 512 + CPU_BACK
    for off in (body_end, body_start - 1, arena_end - 1, 0):
        rep, rec = one(off)
        assert rep == (2, 1, Offender((nbytes_of // 4,), torch.float32, off - body_start, "guard"))
    if nbytes_of % 512 == 0:
        assert arena_end - 1 == body_end + CPU_BACK - 1
    # untouched
    g = _g()
    g.empty(nbytes_of // 4, dtype=torch.float32)
    assert g.check() == (1, 0, None)
    # several bytes, two buffers: all counted, the first buffer's first byte named
    g = _g()
    a, b = g.zeros(3, dtype=torch.int32), g.empty((2, 2), dtype=torch.float64)
    g.records[0].arena[CPU_FRONT - 8:CPU_FRONT] = 0
    g.records[1].arena[CPU_FRONT + 32 + 5] = 1
    rep = g.check()
    assert rep == (2, 9, Offender((3,), torch.int32, -8, "guard"))
    with pytest.raises(AssertionError):
        g.assert_clean()


def test_a_modified_input_is_reported():
    g = _g()
    src = torch.arange(10, dtype=torch.float32).view(2, 5)
    x = g.alloc_like(src)
    seed = g.alloc_like(torch.tensor([41]), role="output")
    assert torch.equal(x, src) and x.data_ptr() != src.data_ptr()
    assert g.check() == (2, 0, None)
    seed += 1                                  # an output of the test's: it may change
    assert g.check() == (2, 0, None)
    x[1, 2] = -7.0
    rep = g.check()
    assert rep.n_bad_bytes >= 1 and rep.first.where == "input"
    assert rep.first.shape == (2, 5) and 28 <= rep.first.offset < 32
    # the same bits written back: unchanged again
    x[1, 2] = 7.0
    assert g.check() == (2, 0, None)
    # alloc_like tensors do not count as the product's allocations
    g.assert_clean(min_buffers=0)
    with pytest.raises(AssertionError):
        g.assert_clean(min_buffers=1)


def test_same_bits():
    nan = float("nan")
    a = torch.tensor([1.0, nan, -0.0])
    assert same_bits(a, a.clone())
    assert not same_bits(a, torch.tensor([1.0, nan, 0.0]))       # -0.0 and 0.0 differ in bits
    assert not same_bits(a, torch.tensor([1.0, 2.0, -0.0]))      # NaN positions
    assert not same_bits(a, a.double()) and not same_bits(a, a[:2])
    assert same_bits(None, None) and not same_bits(a, None)
    assert same_bits(torch.tensor([3, 4]), torch.tensor([3, 4]))


# ------------------------------------------------------- the host library
def _run(f, tensors):
    t = {k: v for k, v in tensors.items()}
    if f.mode == "train":
        for k in DIFF + (["r_sqrt_sigma"] if f.trainable_r else []):
            t[k] = t[k].requires_grad_(True)
    out = mpvae.compute_loss(*[t[k] for k in INPUTS],
                             f.args(mpvae_noise=torch.from_numpy(f["noise"].copy())))
    grads = {}
    if f.mode == "train":
        (out[0] * 0.7 + sum(w * o for w, o in zip((1.3, 0.6, 1.7, 0.9, 1.4), out[1:6]))
         + (out[6] * torch.from_numpy(f["g_I"])).sum()
         + (out[7] * torch.from_numpy(f["g_IL"])).sum()).backward()
        grads = {k: t[k].grad for k in INPUTS if t[k].requires_grad}
        assert all(v is not None for v in grads.values())
    return [o.detach() for o in out], grads


@pytest.mark.parametrize("name", ["f1_l38", "f6_l81", "f7_l256", "f5_testmode"])
def test_host_library_under_guards(name, monkeypatch):
    f = FIX[name]
    plain_out, plain_grads = _run(f, {k: torch.from_numpy(f[k].copy()) for k in INPUTS})
    g = guard(monkeypatch, mpvae_host, device="cpu")
    assert mpvae_host.torch is g
    out, grads = _run(f, {k: g.alloc_like(torch.from_numpy(f[k])) for k in INPUTS})
    # forward: rowstat, bstat, colsum (+ T), out6, indiv, indiv_label; backward: d2, flat (+ dR64)
    # and the four KL gradients
    rep = g.assert_clean(min_buffers=13 if f.mode == "train" else 6, what=name)
    assert rep.n_buffers >= len(INPUTS) + (13 if f.mode == "train" else 6)
    assert len(out) == 8
    for i, (a, b) in enumerate(zip(out, plain_out)):
        assert same_bits(a, b), (name, i)
    assert set(grads) == set(plain_grads) and (f.mode != "train" or len(grads) >= 6)
    for k in grads:
        assert same_bits(grads[k], plain_grads[k]), (name, k)
