"""numpy Philox4x32-10 + Box-Muller -- TEST INFRASTRUCTURE ONLY.

Restates the counter-based generator the build uses for its perf-mode probit
noise (the reference draws that noise from torch's CPU generator,
mpvae.py:162; the build's ``noise='philox'`` mode replaces it by design, see
DESIGN.md).  Philox4x32-10 follows Salmon et al., "Parallel random numbers: as
easy as 1, 2, 3" (SC'11) / Random123; pinned by its published known-answer
vectors in tests/test_oracle_golden.py.

Noise element e = ((s_global * B + b) * z + k) of the (S,B,z) tensor is output
word (e mod 4) of philox(counter = (e div 4 + offset) mod 2^64 as
(lo, hi, 0, 0), key = seed) with words (0,1) and (2,3) Box-Muller pairs.  With
m_even = w_even >> 8 and m_odd = w_odd >> 8 (24 bits each):
    u = fp32(fp32(m_even) + 0.5) * 2^-24,   v = m_odd * 2^-24
    n_even = sqrt(-2 ln u) cos(2 pi v),     n_odd = sqrt(-2 ln u) sin(2 pi v)
u is formed in fp32, as the device's ``box_muller`` forms it (csrc/
mpv_common.h): m_even + 0.5 is exact below 2^23 and rounds to even from there
on, so u is (m_even + 0.5) 2^-24 for m_even < 2^23 and that +- 2^-25 above
(m_even = 2^24 - 1 gives u = 1, r = 0).  Everything after u -- the logarithm,
the square root, sine and cosine -- is fp64 here; the kernels' fp32 hardware
transcendentals are what the tests' tolerance (tests/tolerances.py NOISE_ATOL)
measures.  The key is (seed_lo, seed_hi); the 64-bit ``offset`` is added to the
counter so successive calls draw disjoint streams.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 on uint32 arrays; returns 4 uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(a, np.uint32).copy() for a in (c0, c1, c2, c3))
    k0 = np.asarray(k0, np.uint32).copy()
    k1 = np.asarray(k1, np.uint32).copy()
    for _ in range(10):
        p0 = c0.astype(np.uint64) * M0
        p1 = c2.astype(np.uint64) * M1
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & MASK).astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & MASK).astype(np.uint32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = ((k0.astype(np.uint64) + np.uint64(W0)) & MASK).astype(np.uint32)
        k1 = ((k1.astype(np.uint64) + np.uint64(W1)) & MASK).astype(np.uint32)
    return c0, c1, c2, c3


def words_at(ctr, seed):
    """The 4 output words (uint32 arrays) of the 64-bit counters ``ctr`` (a
    uint64 array) under the 64-bit key ``seed``."""
    ctr = np.asarray(ctr, np.uint64)
    seed = int(seed) % 2 ** 64
    zero = np.zeros(ctr.shape, np.uint32)
    return philox4x32_10((ctr & MASK).astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32),
                         zero, zero, np.full(ctr.shape, seed & 0xFFFFFFFF, np.uint32),
                         np.full(ctr.shape, seed >> 32, np.uint32))


def uniform_u(m_even):
    """Box-Muller's u of the 24-bit m_even = w_even >> 8, formed in fp32 as the
    device forms it (module docstring), widened to float64."""
    m = np.asarray(m_even).astype(np.float32)
    return ((m + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64)


def box_muller(w_even, w_odd):
    """(n_even, n_odd) float64 of the word pair(s) (uint32 arrays)."""
    u = uniform_u(np.asarray(w_even, np.uint32) >> np.uint32(8))
    v = (np.asarray(w_odd, np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u))
    return r * np.cos(2 * np.pi * v), r * np.sin(2 * np.pi * v)


def normal_at(e, seed, offset=0):
    """float64 normals of the global element indices ``e`` (a uint64 array of
    any shape): element e is normal (e mod 4) of counter (e div 4 + offset)
    mod 2^64."""
    e = np.asarray(e, np.uint64)
    ctr = e // np.uint64(4) + np.full(e.shape, int(offset) % 2 ** 64, np.uint64)  # wraps mod 2^64
    lane = (e % np.uint64(4)).astype(np.int64)
    w = words_at(ctr, seed)
    second = lane >= 2                                     # the (2,3) pair
    n_even, n_odd = box_muller(np.where(second, w[2], w[0]), np.where(second, w[3], w[1]))
    return np.where(lane % 2 == 0, n_even, n_odd)


def normal_noise(S_local, B, z, seed, offset=0, s_offset=0):
    """(S_local,B,z) float64 noise of the shard starting at global sample s_offset."""
    e0 = int(s_offset) * int(B) * int(z)
    e = np.full(S_local * B * z, e0, np.uint64) + np.arange(S_local * B * z, dtype=np.uint64)
    return normal_at(e, seed, offset).reshape(S_local, B, z)
