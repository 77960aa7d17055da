"""Philox counters whose words sit at Box-Muller's edges (CPU only, the oracle
only: nothing here comes from the reference or from a kernel).

Box-Muller maps the 24-bit m_even = w_even >> 8 to the radius and
m_odd = w_odd >> 8 to the angle (oracle/philox.py).  A random draw reaches the
ends of either range with probability 2^-24 per word pair, so a noise test over
a few thousand elements never sees them.  This scans the counters 0 .. SCAN-1
under the tests' key and records, per class and in counter order, at most
PER_CLASS (counter, word pair) entries:

    even_lo   m_even < 256            u -> 2^-25: the largest |n| (5.89, the
                                      bound behind the planes' constant scale);
                                      holds every m_even == 0 of the scan
    even_hi   m_even >= 2^24 - 256    u -> 1, r -> 0; m_even >= 2^23 is where the
                                      fp32 m_even + 0.5 rounds; holds every
                                      m_even == 2^24 - 1 of the scan (u = 1, r = 0)
    odd_0, odd_q1, odd_q2, odd_q3
              m_odd within 256 of 0 (mod 2^24), 2^22, 2^23, 3 * 2^22: the
              quarter turns of sine and cosine, where one of them crosses zero

The exact hits (m_even == 0, m_even == 2^24 - 1) come first in their class; the
rest of the class is filled with its earliest entries.  main() asserts that the
scan found at least one of each exact hit.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_philox_edges.py
Writes: tests/golden/philox_edges.npz  (counters and words only, a few KB)
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import philox  # noqa: E402

KEY = 0x1234ABCD5678
SCAN = 1 << 23          # counters scanned (the exact hits: 353595, 1197692, 6551524)
CHUNK = 1 << 20
PER_CLASS = 32
NEAR = 256
M24 = 1 << 24
CLASSES = ["even_lo", "even_hi", "odd_0", "odd_q1", "odd_q2", "odd_q3"]
PATH = os.path.join(HERE, "philox_edges.npz")


def _class_masks(me, mo):
    """{class: (member mask, exact-hit mask)} of the 24-bit m_even, m_odd arrays."""
    me, mo = me.astype(np.int64), mo.astype(np.int64)
    none = np.zeros(me.shape, bool)
    out = {"even_lo": (me < NEAR, me == 0),
           "even_hi": (me >= M24 - NEAR, me == M24 - 1)}
    for name, q in (("odd_0", 0), ("odd_q1", M24 // 4), ("odd_q2", M24 // 2),
                    ("odd_q3", 3 * (M24 // 4))):
        d = (mo - q) % M24
        out[name] = (np.minimum(d, M24 - d) <= NEAR, none)
    return out


def scan():
    """{class: list of (exact, counter, pair, words[4])}, every hit of the scan
    for the exact classes' exact hits, the earliest PER_CLASS otherwise."""
    hits = {c: [] for c in CLASSES}
    for c0 in range(0, SCAN, CHUNK):
        ctr = np.arange(c0, c0 + CHUNK, dtype=np.uint64)
        w = np.stack(philox.words_at(ctr, KEY), -1)                # (n, 4)
        # a class already full of earlier entries takes only exact hits from here on
        full = {c: sum(1 for h in hits[c] if not h[0]) >= PER_CLASS for c in CLASSES}
        for pair in (0, 1):
            me, mo = w[:, 2 * pair] >> np.uint32(8), w[:, 2 * pair + 1] >> np.uint32(8)
            for name, (member, exact) in _class_masks(me, mo).items():
                take = exact if full[name] else member
                for i in np.flatnonzero(take):
                    hits[name].append((bool(exact[i]), int(ctr[i]), pair, w[i].copy()))
    return hits


def select(hits):
    """Per class: the exact hits, then the earliest others, PER_CLASS in all."""
    rows = []
    for k, name in enumerate(CLASSES):
        h = sorted(hits[name], key=lambda t: (not t[0], t[1], t[2]))[:PER_CLASS]
        rows += [(k,) + t for t in sorted(h, key=lambda t: (t[1], t[2]))]
    return rows


def tables():
    rows = select(scan())
    w = np.stack([r[4] for r in rows]).astype(np.uint32)
    pair = np.array([r[3] for r in rows], np.uint8)
    idx = np.arange(len(rows))
    return dict(key=np.array([KEY], np.uint64),
                classes=np.array(CLASSES),
                cls=np.array([r[0] for r in rows], np.uint8),
                counter=np.array([r[2] for r in rows], np.uint64),
                pair=pair, words=w,
                m_even=w[idx, 2 * pair] >> np.uint32(8),
                m_odd=w[idx, 2 * pair + 1] >> np.uint32(8))


def npz_bytes(arrays):
    """An uncompressed .npz with fixed member dates: the same bytes every run."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as zf:
        for name, a in arrays.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(a), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)),
                        member.getvalue())
    return buf.getvalue()


def main():
    t = tables()
    cls, me = t["cls"], t["m_even"]
    assert (me[cls == CLASSES.index("even_lo")] == 0).any(), "no m_even == 0 in the scan"
    assert (me[cls == CLASSES.index("even_hi")] == M24 - 1).any(), "no m_even == 2^24-1 in the scan"
    for k, name in enumerate(CLASSES):
        assert 0 < (cls == k).sum() <= PER_CLASS, name
    with open(PATH, "wb") as f:
        f.write(npz_bytes(t))
    for k, name in enumerate(CLASSES):
        print(name, int((cls == k).sum()), "entries, counters",
              int(t["counter"][cls == k].min()), "..", int(t["counter"][cls == k].max()))
    print(os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
