"""The operand kernels of csrc/util.hip, bit for bit: the 3xf16 split planes
against a torch emulation on every path of mpv_split_f16, and the slab sums
behind colsum and d fe_out / d fx_out in each of their layouts."""
import math

import pytest
import torch

from mpvae_ops import HipShardBackend

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------- split planes
def emulated_planes(R, rows_pad, cols_pad):
    """(the int16 words of Planes.data, the scale) as include/mpvae_hip.h
    defines them: s = 2^(14 - e) with max|x| = m 2^e (frexp), hi = fp16(x s),
    lo = fp16(x s - hi), every 32-column chunk of a row 32 hi then 32 lo words,
    +0 in the padding."""
    rows, cols = R.shape
    m = float(R.float().abs().max())
    s = 2.0 ** (14 - math.frexp(m)[1]) if m > 0.0 and math.isfinite(m) else 1.0
    xs = R.float() * s
    hi = xs.half()
    lo = (xs - hi.float()).half()
    want = torch.zeros((rows_pad, cols_pad), dtype=torch.float16, device=R.device)
    planes = torch.stack([want.clone(), want], 0)
    planes[0, :rows, :cols], planes[1, :rows, :cols] = hi, lo
    # (2, rows_pad, chunks, 32) -> (rows_pad, chunks, 2, 32)
    words = planes.view(2, rows_pad, cols_pad // 32, 32).permute(1, 2, 0, 3).contiguous()
    return words.view(torch.int16).view(rows_pad, 2 * cols_pad), s


# rows, cols, where the largest |x| goes, elements the view is offset by
SPLIT_CASES = [
    (3, 2, None, 0),         # the small path (one workgroup's share and less)
    (37, 53, None, 0),       # the small path, ragged
    (128, 128, None, 0),     # the small path at exactly its 16384 elements
    (129, 128, None, 0),     # vector max, 8-column split
    (127, 131, "last", 0),   # n % 4 == 1: vector max, the largest |x| in block 0's tail
    (127, 131, "first", 0),  # ... and in the first vector; cols % 8 != 0: scalar split
    (300, 136, None, 1),     # misaligned: scalar max, scalar split
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("rows,cols,peak,offset", SPLIT_CASES,
                         ids=[f"{r}x{c}" + (f"_{p}" if p else "") + ("_misaligned" if o else "")
                              for r, c, p, o in SPLIT_CASES])
def test_split_planes_bit_for_bit(rows, cols, peak, offset, dtype):
    """prepare_R's planes and scale equal the emulation word for word,
    padding rows and columns included (+0)."""
    be = HipShardBackend("f16x3")
    g = torch.Generator(device=DEV).manual_seed(rows * 1000 + cols)
    flat = torch.randn(rows * cols + offset, device=DEV, dtype=dtype, generator=g) * 0.3
    R = flat[offset:].view(rows, cols)
    assert R.data_ptr() % 16 == (offset * R.element_size()) % 16
    if peak is not None:
        R.view(-1)[-1 if peak == "last" else 0] = -7.5  # above every 0.3 N(0, 1) draw here
        assert float(R.abs().max()) == 7.5
    pl = be.prepare_R(R)
    want, s = emulated_planes(R, pl.rows_pad, pl.cols)
    assert float(pl.scale) == s
    assert torch.equal(pl.data, want)


@pytest.mark.parametrize("rows,cols", [(37, 53), (129, 128)], ids=["small", "large"])
def test_split_of_zeros(rows, cols):
    """An all-zero input: scale 1 and planes of +0."""
    pl = HipShardBackend("f16x3").prepare_R(torch.zeros((rows, cols), device=DEV))
    assert float(pl.scale) == 1.0
    assert not pl.data.any()


# ---------------------------------------------------------------- slab sums
def _inputs(B, L, z, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = (torch.rand((B, L), device=DEV, generator=g) < 0.3).float()
    y[:, 0], y[:, 1] = 1, 0
    fe = torch.randn((B, L), device=DEV, generator=g)
    fx = torch.randn((B, L), device=DEV, generator=g)
    R = (torch.rand((L, z), device=DEV, generator=g, dtype=torch.float64) * 2 - 1) * 0.3
    return y, fe, fx, R


def split_layout_sum(parts):
    """The split layout's order, formed by torch's fp32 adds: group g adds
    slabs g, g + 16, ... in order to 0, then the 16 groups are added in order."""
    groups = []
    for g in range(16):
        acc = torch.zeros_like(parts[0])
        for k in range(g, len(parts), 16):
            acc = acc + parts[k]
        groups.append(acc)
    total = groups[0]
    for acc in groups[1:]:
        total = total + acc
    return total


@pytest.mark.parametrize("gemm,L", [("f16x3", 49), ("f32", 3)])
def test_forward_colsum_is_the_slab_sum(gemm, L):
    """colsum of a forward whose s-chunk partials go through the slab-sum
    kernel, against torch's sum of the same partials in the kernel's order.

    plan_fwd (256 CUs): nSc = nSt chunks of one s-tile when cdiv(target, B nNt)
    >= nSt, target 256 (3xf16) or 2048 (fp32); fwd_combine folds up to 64
    chunks itself, so the slab sum runs from nSc = 65: B nNt <= 3 (3xf16) or
    <= 31 (fp32).  Then n = 2 B L <= 2 * 31 * 128 < 65536 with nslab >= 64: the
    forward reaches the split layout only.  Smallest: B = 1 and the 128-row
    s-tiles (3xf16: the 96-label tile, L = 49; fp32: any L <= 96), S = 64 * 128
    + 1 rows -- 65 chunks, the last of one row.  Chunk k alone is the forward
    of the shard [128 k, 128 k + 128) (one s-tile: the tile writes colsum
    itself), Philox noise being keyed on the global sample index."""
    B, z, BM = 1, 2, 128
    S = 64 * BM + 1
    y, fe, fx, R = _inputs(B, L, z, 5)
    be = HipShardBackend(gemm)
    Rop = be.prepare_R(R)

    def colsum(S_local, s_offset):
        shape = be.shape(S_local, S, s_offset, B, L, z)
        eps = be.make_noise(shape, DEV, 24680, 0)
        return be.forward_local(shape, y, fe, fx, Rop, eps, keep_T=False)["colsum"]

    parts = [colsum(min(BM, S - s0), s0) for s0 in range(0, S, BM)]
    assert len(parts) == 65
    assert torch.equal(colsum(S, 0), split_layout_sum(parts))


# B, L, z, S, gemm: the layouts of (d fe_out | d fx_out, dR)
BWD_SLAB_CASES = [
    (1, 3, 3, 4, "f16x3"),       # plain, plain
    (2, 4, 4, 4, "f16x3"),       # vec, vec
    (1, 512, 4, 2048, "f16x3"),  # split, vec
    (1, 2, 2, 16384, "f16x3"),   # vec, split
]


@pytest.mark.parametrize("B,L,z,S,gemm", BWD_SLAB_CASES,
                         ids=[f"B{B}_L{L}_z{z}_S{S}" for B, L, z, S, _ in BWD_SLAB_CASES])
def test_backward_pair_is_the_single_sum(B, L, z, S, gemm):
    """d fe_out | d fx_out summed beside the dR slabs (want_dR: the pair
    launch) equal the sum launched alone, and dR in fp64 is the fp32 dR.

    The layout rule: split when nslab >= 64 and n <= 65536, else vec when n % 4
    == 0 (the workspace is 256-B aligned), else plain.  d fe_out | d fx_out: n =
    2 B L over plan_bwd's nSc element-pass chunks; dR: n = L z over its nKc
    split-K chunks.  On 256 CUs:
    - plain, plain: B L and L z odd (1, 3, 3, 4).
    - vec, vec: both even, few chunks (2, 4, 4, 4).
    - split for d fe_out | d fx_out: nSc = min(8192 / B, S / (16 RPI)) >= 64
      with RPI = 1024 / L rows per pass of a block (L < 1024), so S = 2^20 / L
      at B = 1, the same B S L for every L; the shortest S short of the ring
      element pass (L >= 1024, 128 rows per chunk at least) is (1, 512, 4,
      2048): RPI 2, 64 chunks of 32 rows.  Its dR (256 tile, 2048 rows: 8
      chunks) is vec.
    - split for dR: nKc = min(512 / tiles, B S / 256) >= 64 on the 64 tile:
      B S = 16384 rows, (1, 2, 2, 16384); its d fe_out | d fx_out (4 chunks) is
      vec."""
    y, fe, fx, R = _inputs(B, L, z, 6)
    be = HipShardBackend(gemm)
    shape = be.shape(S, S, 0, B, L, z)
    eps = be.make_noise(shape, DEV, 13579, 0)
    loc = be.forward_local(shape, y, fe, fx, be.prepare_R(R), eps, keep_T=True)
    gscal = torch.tensor([1.0, 0.3, 0.2, 0.7, 0.4, 0.0], device=DEV)

    def bwd(want_dR, dR_dtype=torch.float32):
        # the element pass overwrites T in place: a fresh copy per call
        saved = dict(y=y, fe_out=fe, fx_out=fx, eps=eps, T=loc["T"].clone(),
                     rowstat=loc["rowstat"], bstat=loc["bstat"])
        _, dfe_dfx, dR = be.backward_local(shape, saved, gscal, 0b011111, None, None, 0.1, 200.0,
                                           want_dR, dR_dtype=dR_dtype)
        return dfe_dfx.clone(), dR

    single, _ = bwd(False)
    pair, dR32 = bwd(True)
    pair64, dR64 = bwd(True, torch.float64)
    assert torch.isfinite(single).all()
    assert torch.equal(pair, single) and torch.equal(pair64, single)
    assert torch.equal(dR64, dR32.double())


@pytest.mark.parametrize("B,L", [(1, 3), (2, 4)], ids=["plain", "vec"])
def test_backward_sum_is_the_slab_order_sum(B, L):
    """d fe_out | d fx_out over several element-pass chunks, alone and beside
    the dR slabs, against torch's sum of the chunks' partials slab by slab.

    plan_bwd at L <= 4 (RPI 256, 16 rows per thread at least): 4096 rows per
    chunk, so S = 3 * 4096 gives nSc = 3 slabs of n = 2 B L elements: 6 (plain
    in either launch) or 16 (vec in the pair, plain alone).  Chunk k alone is
    the backward of the shard [4096 k, 4096 k + 4096) under the whole batch's
    bstat (one chunk: its sum is 0 + the partial)."""
    z, S, rows = 3, 3 * 4096, 4096
    y, fe, fx, R = _inputs(B, L, z, 7)
    be = HipShardBackend("f16x3")
    Rop = be.prepare_R(R)
    gscal = torch.tensor([1.0, 0.3, 0.2, 0.7, 0.4, 0.0], device=DEV)

    def fwd(S_local, s_offset):
        shape = be.shape(S_local, S, s_offset, B, L, z)
        eps = be.make_noise(shape, DEV, 97531, 0)
        return shape, eps, be.forward_local(shape, y, fe, fx, Rop, eps, keep_T=True)

    def bwd(shape, eps, loc, bstat, want_dR):
        saved = dict(y=y, fe_out=fe, fx_out=fx, eps=eps, T=loc["T"].clone(),
                     rowstat=loc["rowstat"], bstat=bstat)
        return be.backward_local(shape, saved, gscal, 0b011111, None, None, 0.1, 200.0,
                                 want_dR)[1].clone()

    shape, eps, loc = fwd(S, 0)
    bstat = loc["bstat"]
    want = torch.zeros((2, B, L), device=DEV)
    for s0 in range(0, S, rows):
        want = want + bwd(*fwd(rows, s0), bstat, False)
    assert torch.isfinite(want).all() and bool(want.any())
    assert torch.equal(bwd(shape, eps, loc, bstat, False), want)
    assert torch.equal(bwd(shape, eps, loc, bstat, True), want)
