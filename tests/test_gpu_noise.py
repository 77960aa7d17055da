"""Device Philox noise (csrc/util.hip: noise_philox_kernel, the fp32 draw, and
noise_philox16_kernel, the 3xf16 planes) against oracle/philox.py on every
launch path: the narrow, one-row-per-block and column-stride geometries of the
planes kernel, counters beyond 32 bits, the call offset, the Box-Muller edges
of tests/golden/philox_edges.npz and the fp32 kernel's grid-stride loop.

Every draw goes through the C ABI into buffers pre-filled with 0xFF bytes (NaN
in fp32 and fp16, -1 as an integer), larger than what the kernel is to write:
an element it skips stays NaN, one it writes out of place shows in the fill.
Run with ``pytest -m gpu`` on an MI355X."""
import functools
import os

import numpy as np
import pytest
import torch

import mpvae_hip as H
from mpvae_ops import Planes
from oracle import philox
from tolerances import NOISE_ATOL, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY = 0x1234ABCD5678
S0, B0, L0 = 5, 7, 4        # 35 plane rows: three blocks of 16 on the wide paths, the last ragged
GUARD = 64                  # fp32 elements past the draw, plane rows past the last
R_MAX = 5.8875              # sqrt(-2 ln 2^-25) = 5.88710 (u's smallest value), and the fp32 error


def _shape(S, B, z, s_off=0, L=L0):
    return H.Shape(S, s_off + S, s_off, B, L, z)


def _dev_key(key):
    return torch.tensor([key - 2 ** 64 if key >= 2 ** 63 else key], dtype=torch.int64, device=DEV)


def draw_f32(shape, key=KEY, offset=0, dev_key=False):
    """mpv_noise_philox[_dev] into a 0xFF-filled buffer: the int32 view of the
    n drawn elements and of the guard behind them."""
    lib, st = H.load_library(), H.stream_of(DEV)
    n = shape.S_local * shape.B * shape.z
    buf = torch.full((n + GUARD,), -1, dtype=torch.int32, device=DEV)
    if dev_key:
        k = _dev_key(key)
        H.check(lib.mpv_noise_philox_dev(H.ptr(buf), shape, H.ptr(k), offset, st),
                "mpv_noise_philox_dev")
    else:
        H.check(lib.mpv_noise_philox(H.ptr(buf), shape, key, offset, st), "mpv_noise_philox")
    torch.cuda.synchronize()
    return buf


def draw_planes(shape, key=KEY, offset=0, dev_key=False):
    """mpv_noise_philox_f16[_dev] into 0xFF-filled planes of GUARD rows more
    than the draw has."""
    lib, st = H.load_library(), H.stream_of(DEV)
    cols = int(lib.mpv_noise_plane_cols(shape))
    assert cols > 0 and cols % 64 == 0 and cols >= shape.z
    pl = Planes(shape.S_local * shape.B + GUARD, cols, DEV)
    pl.data.fill_(-1)
    pl.scale.view(torch.int32).fill_(-1)
    if dev_key:
        k = _dev_key(key)
        H.check(lib.mpv_noise_philox_f16_dev(shape, H.ptr(k), offset, pl.c(), st),
                "mpv_noise_philox_f16_dev")
    else:
        H.check(lib.mpv_noise_philox_f16(shape, key, offset, pl.c(), st), "mpv_noise_philox_f16")
    torch.cuda.synchronize()
    return pl


def f32_values(buf, shape):
    """The (S, B, z) float64 values of a draw_f32 buffer; nothing skipped, the
    guard untouched."""
    S, B, z = shape.S_local, shape.B, shape.z
    raw = buf.cpu().numpy()
    assert (raw[S * B * z:] == -1).all(), "fp32 draw: wrote past its end"
    v = raw[:S * B * z].view(np.float32).astype(np.float64).reshape(S, B, z)
    assert np.isfinite(v).all(), "fp32 draw: skipped or non-finite elements"
    return v


def plane_values(pl, shape):
    """The (S, B, z) float64 values of the planes, after the layout checks every
    planes case makes: plane row b*S + s holds eps[s, b]; columns z ..
    round32(z)-1 are zeros; columns beyond and rows beyond S*B keep the fill;
    the scale is 4096."""
    S, B, z = shape.S_local, shape.B, shape.z
    rows, w = S * B, min(pl.cols, (z + 31) // 32 * 32)
    assert pl.rows_pad == rows + GUARD and pl.ld == 2 * pl.cols
    assert float(pl.scale.cpu()[0]) == 4096.0
    raw = pl.data.cpu().numpy()
    assert (raw[rows:] == -1).all(), "planes: wrote rows past S_local * B"
    assert (raw[:rows, 2 * w:] == -1).all(), "planes: wrote columns past round32(z)"
    v = pl.value()[:rows, :w].double().cpu().numpy()
    assert np.isfinite(v).all(), "planes: skipped or non-finite elements"
    assert not v[:, z:].any(), "planes: columns z .. round32(z)-1 are not zero"
    return v[:, :z].reshape(B, S, z).transpose(1, 0, 2)


@functools.lru_cache(maxsize=None)
def oracle_noise(S, B, z, s_off=0, offset=0):
    ref = philox.normal_noise(S, B, z, KEY, offset=offset, s_offset=s_off)
    ref.setflags(write=False)
    return ref


def check_both(test_id, shape, offset=0, dev_key_too=False):
    """The fp32 draw and the planes of `shape` against the oracle."""
    S, B, z, s_off = shape.S_local, shape.B, shape.z, shape.s_offset
    ref = oracle_noise(S, B, z, s_off, offset)
    buf, pl = draw_f32(shape, offset=offset), draw_planes(shape, offset=offset)
    errs = {"f32": np.abs(f32_values(buf, shape) - ref).max(),
            "planes": np.abs(plane_values(pl, shape) - ref).max()}
    print(test_id, errs)
    record(test_id, errs)
    assert errs["f32"] <= NOISE_ATOL and errs["planes"] <= NOISE_ATOL, errs
    if dev_key_too:  # the key read from device memory: the same bits, fill included
        assert torch.equal(draw_f32(shape, offset=offset, dev_key=True), buf)
        pd = draw_planes(shape, offset=offset, dev_key=True)
        assert torch.equal(pd.data, pl.data) and torch.equal(pd.scale, pl.scale)


def launch_geometry(shape):
    """(path, threads per plane row) of noise_philox_f16's dispatch, from the
    plane columns the library reports and z."""
    cols = int(H.load_library().mpv_noise_plane_cols(shape))
    tpr = min(cols, (shape.z + 31) // 32 * 32) // 8
    if tpr >= 256:
        return "stride", tpr       # 256-thread blocks, a column-stride loop per row
    if tpr % 64 == 0:
        return "row", tpr          # one row per block of tpr threads
    return "narrow", (shape.z + 7) // 8   # lanes holding normals; several rows per pass


# ------------------------------------------------------------------ a. geometries
@pytest.mark.parametrize("z,path,tpr", [
    (450, "narrow", 57),                        # a zero tail of three 8-column groups
    (509, "row", 64), (512, "row", 64),         # 509 % 4 = 1: the phase e_row & 3 varies by row
    (1001, "row", 128), (1024, "row", 128),     # 1024: the headline's own
    (1530, "row", 192), (1536, "row", 192),
    (2048, "stride", 256),                      # one column pass
    (2051, "stride", 260),                      # a second pass of four lanes, z % 4 = 3
    (4096, "stride", 512)])                     # two full passes
def test_launch_geometries(z, path, tpr):
    shape = _shape(S0, B0, z)
    assert launch_geometry(shape) == (path, tpr)
    check_both(f"noise_geometry_z{z}", shape, dev_key_too=True)


# ------------------------------------------------------------------ b. 64-bit counters
@pytest.mark.parametrize("where", ["wrap32", "high40"])
@pytest.mark.parametrize("B,z", [(3, 13), (2, 16), (3, 2051)],
                         ids=["three_counters", "aligned", "stride"])
def test_counters_beyond_32_bits(B, z, where):
    """Global element 2^34 (counter 2^32: the low word wraps, and with it
    ctr + 1 / ctr + 2 of the three-counter path) inside the shard, and a shard
    whose counters' high word is in the thousands."""
    S = 5
    s_off = 2 ** 34 // (B * z) - 2 if where == "wrap32" else 2 ** 40 + 1
    e0 = s_off * B * z
    if where == "wrap32":
        assert e0 < 2 ** 34 < e0 + S * B * z
    else:
        assert (e0 // 4) >> 32 > 1000
    check_both(f"noise_ctr64_{where}_B{B}_z{z}", _shape(S, B, z, s_off))


# ------------------------------------------------------------------ c. call offset
@pytest.mark.parametrize("offset", [1, 2 ** 32 - 3, 2 ** 32, 2 ** 63, 2 ** 64 - 2],
                         ids=["1", "2p32m3", "2p32", "2p63", "2p64m2"])
@pytest.mark.parametrize("z", [13, 1001, 2051], ids=["narrow", "row128", "stride"])
def test_call_offset(z, offset):
    """counter = element div 4 + offset, mod 2^64 (2^64 - 2 wraps inside the
    shard, 2^32 - 3 carries into the high word)."""
    shape = _shape(S0, B0, z)
    assert launch_geometry(shape)[0] == {13: "narrow", 1001: "row", 2051: "stride"}[z]
    check_both(f"noise_offset_{offset:#x}_z{z}", shape, offset=offset)


# ------------------------------------------------------------------ d. Box-Muller edges
EDGES = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "philox_edges.npz"))
EDGE_CLASSES = [str(c) for c in EDGES["classes"]]


@pytest.mark.parametrize("cls", EDGE_CLASSES)
def test_box_muller_edges(cls):
    """One counter per draw (S = B = 1, z = 4, offset = the counter): the four
    normals of the fixture's counters -- u at 2^-25 and at 1, v at the quarter
    turns -- finite, inside the bound behind the planes' scale, and the
    oracle's."""
    assert int(EDGES["key"][0]) == KEY
    sel = np.flatnonzero(EDGES["cls"] == EDGE_CLASSES.index(cls))
    shape = _shape(1, 1, 4)
    err = {"f32": [], "planes": []}
    for i in sel:
        c, pair = int(EDGES["counter"][i]), int(EDGES["pair"][i])
        ref = philox.normal_at(np.arange(4, dtype=np.uint64), KEY, offset=c)
        # the fixture's words are this counter's
        w = [int(x[0]) for x in philox.words_at(np.array([c], np.uint64), KEY)]
        assert w == [int(x) for x in EDGES["words"][i]]
        assert w[2 * pair] >> 8 == int(EDGES["m_even"][i])
        assert w[2 * pair + 1] >> 8 == int(EDGES["m_odd"][i])
        got = {"f32": f32_values(draw_f32(shape, offset=c), shape).ravel(),
               "planes": plane_values(draw_planes(shape, offset=c), shape).ravel()}
        for k, g in got.items():
            assert np.abs(g).max() <= R_MAX, (k, c, g)
            d = g - ref
            assert np.abs(d).max() <= NOISE_ATOL, (k, c, pair, int(EDGES["m_even"][i]),
                                                   int(EDGES["m_odd"][i]), g, ref)
            if int(EDGES["m_even"][i]) == 2 ** 24 - 1:   # u = 1: r = 0
                assert (ref[2 * pair:2 * pair + 2] == 0).all()
                assert np.abs(g[2 * pair:2 * pair + 2]).max() <= NOISE_ATOL, (k, c, g)
            err[k].append(d[2 * pair:2 * pair + 2])      # the pair at the edge
    errs = {}
    for k, d in err.items():
        d = np.concatenate(d)
        errs[k + "_min"], errs[k + "_max"] = d.min(), d.max()
    print(cls, len(sel), "counters", errs)
    record(f"noise_edges_{cls}", errs)


# ------------------------------------------------------------------ e. fp32 grid-stride loop
def _draw_and_sample(shape, n, idx):
    """Draw the n fp32 elements of `shape` into a 0xFF-filled buffer, check
    that every one was written and nothing past them, and return the elements
    idx (sorted int64) as float64.  The buffer is handled in views of 2^30
    elements, so that every torch index stays below 2^31."""
    lib, st = H.load_library(), H.stream_of(DEV)
    piece = 2 ** 30
    buf = torch.empty((n + GUARD,), dtype=torch.int32, device=DEV)
    views = [buf[a:min(a + piece, n + GUARD)] for a in range(0, n + GUARD, piece)]
    for v in views:
        v.fill_(-1)
    H.check(lib.mpv_noise_philox(H.ptr(buf), shape, KEY, 0, st), "mpv_noise_philox")
    torch.cuda.synchronize()
    assert (buf[n:].cpu().numpy() == -1).all(), "wrote past its end"
    got = np.empty(len(idx))
    for k, v in enumerate(views):
        m = min(piece, n - k * piece)
        # no element still holds the fill (a NaN): nothing skipped anywhere
        assert not bool((v[:m] == -1).any()), f"unwritten elements in piece {k}"
        sel = np.flatnonzero(idx // piece == k)
        if len(sel):
            j = torch.from_numpy(idx[sel] - k * piece).to(DEV)
            got[sel] = v[j].cpu().numpy().view(np.float32)
    return got


@pytest.mark.timeout(600)
def test_f32_grid_stride_loop_beyond_2p32_elements():
    """2^32 + 4096 elements (S_local = 2^20 + 1, B = 1, z = 4096; 17.2 GB): the
    grid is capped at 2^22 blocks of 256 counters, so elements 2^32 .. are the
    loop's second trip -- every fp32 draw of a C5 shard runs it."""
    S, B, z = 2 ** 20 + 1, 1, 4096
    n = S * B * z
    if torch.cuda.mem_get_info()[0] < 20 * 2 ** 30:
        pytest.skip("needs 20 GiB of free device memory")
    shape = _shape(S, B, z)
    blk = 256 * 4                     # elements per block
    stride = 2 ** 22 * blk            # elements per trip of the loop
    assert stride == 2 ** 32 < n
    idx = [np.arange(64), np.arange(n - 64, n), np.arange(stride - 64, stride + 64)]
    for b in (0, 1, 2 ** 22 - 1, 2 ** 22):
        idx.append(np.array([b * blk, b * blk + blk - 1]))
    rng = np.random.default_rng(4096)
    idx += [rng.integers(0, n, 2048), rng.integers(stride, n, 512)]
    idx = np.unique(np.concatenate(idx).astype(np.int64))
    assert idx.min() == 0 and idx.max() == n - 1
    got = _draw_and_sample(shape, n, idx)
    torch.cuda.empty_cache()
    ref = philox.normal_at(idx.astype(np.uint64), KEY)
    d = np.abs(got - ref)
    errs = {"f32": d.max(), "f32_second_trip": d[idx >= stride].max()}
    print("noise_grid_stride", len(idx), "samples", errs)
    record("noise_grid_stride", errs)
    assert np.isfinite(got).all() and d.max() <= NOISE_ATOL, (errs, idx[d.argmax()])
