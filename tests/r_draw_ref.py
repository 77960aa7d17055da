"""The draw rule of mpv_r_uniform_philox (include/mpvae_hip.h) restated in numpy
on oracle.philox.philox4x32_10 -- test infrastructure only.

Element e of the (L, z) array is double (e mod 2) of Philox4x32-10 counter
g = (e div 2 + offset) mod 2^64, counter words (lo32(g), hi32(g), 1, 0), key
``seed`` mod 2^64.  Double j comes from words (w_2j, w_2j+1) as numpy's
random_sample takes it from two MT19937 words, and the value from the double as
numpy's uniform does: low + (high - low) * u, each operation rounded.
"""
import numpy as np

from oracle.philox import MASK, philox4x32_10


def bound_of(L, z):
    """sqrt(6 / (L + z)), the reference's bound (fairsoft_train.py:63)."""
    return float(np.sqrt(6.0 / (L + z)))


def doubles_from_words(w_even, w_odd):
    """numpy's random_sample: ((a >> 5) * 2^26 + (b >> 6)) / 2^53 (exact)."""
    a = (np.asarray(w_even, np.uint32) >> np.uint32(5)).astype(np.float64)
    b = (np.asarray(w_odd, np.uint32) >> np.uint32(6)).astype(np.float64)
    return (a * 67108864.0 + b) / 9007199254740992.0


def affine(u, bound):
    """numpy's uniform(-bound, bound) of the doubles u: low + (high - low) * u,
    the product and the sum each rounded to fp64."""
    low = np.float64(-bound)
    scaled = (np.float64(bound) - low) * np.asarray(u, np.float64)
    return low + scaled


def r_uniform(L, z, bound, seed, offset=0):
    """The (L, z) float64 array mpv_r_uniform_philox writes."""
    n = int(L) * int(z)
    g = np.arange((n + 1) // 2, dtype=np.uint64)
    g = g + np.full(g.shape, int(offset) % 2 ** 64, np.uint64)  # wraps mod 2^64
    key = int(seed) % 2 ** 64
    ones, zeros = np.ones(g.shape, np.uint32), np.zeros(g.shape, np.uint32)
    w = philox4x32_10((g & MASK).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32), ones,
                      zeros, np.full(g.shape, key & 0xFFFFFFFF, np.uint32),
                      np.full(g.shape, key >> 32, np.uint32))
    u = np.stack([doubles_from_words(w[0], w[1]), doubles_from_words(w[2], w[3])], axis=1)
    return affine(u.reshape(-1)[:n], bound).reshape(int(L), int(z))
