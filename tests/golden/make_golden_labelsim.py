"""Golden vectors for the closed-form label similarities (LabelSimilarity,
label_sim_kernel): the values the reference's builders store in
``label_distances[target][pattern]``.

Runs ONLY in the build container, where the reference is mounted at
/root/reference (it never travels to the GPU box).  label_distance_obs.py
cannot be imported (it imports mlxtend and pandas at module level, and its
builders load a dataset), so the generator reads the source text at run time
and executes, for every (target, pattern) pair of its own pattern set:

  * ``str_jac_similarity`` and ``str_ham_similarity``, the two function
    definitions as they stand;
  * the statements each builder runs per pair (everything after ``lab2 =
    ''.join(lab2)`` in its inner loop): indication_similarity,
    constant_similarity, _jaccard_similarity, _jaccard_nonlinear_similarity and
    _hamming_nonlinear_similarity, with the builder's own ``minimum_clip`` /
    ``maximum_clip`` defaults and ``args.dist_gamma``.

_hamming_similarity raises as written (``str_ham_similarity()(lab1, lab2)``):
the un-gamma'd Hamming value is ``str_ham_similarity(lab1, lab2)`` itself.
The reference has no gamma form of indication and constant; theirs is the
nonlinear builder's ``weight = ...`` / ``np.clip(...)`` statements applied to
the indication / constant value as ``sim``.

Recorded per file: ``patterns`` (P, L) and ``targets`` (T, L) uint8, ``kinds``
and ``gammas`` (NaN: no gamma), ``values`` (kind, gamma, target, pattern) fp64
and ``np64`` (kind, gamma): 1 where the stored values are numpy float64, 0
where they are Python floats (what decides the reference's loss dtype).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_labelsim.py
Writes: tests/golden/labelsim_s1_l25.npz, tests/golden/labelsim_s2_l130.npz
"""
import argparse
import os
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
KINDS = ["indication", "constant", "jaccard", "hamming"]
GAMMAS = [float("nan"), 0.01, 1.0, 10.0, -0.5]  # the negative one makes the clip act


def source_lines():
    return open(os.path.join(REF, "label_distance_obs.py")).read().split("\n")


def function_text(lines, name):
    """The text of top-level function ``name``."""
    start = next(i for i, l in enumerate(lines) if l.startswith(f"def {name}("))
    end = next((i for i in range(start + 1, len(lines))
                if lines[i] and not lines[i][0].isspace()), len(lines))
    return "\n".join(lines[start:end])


def pair_block(lines, name):
    """The statements builder ``name`` runs per (lab1, lab2) pair, dedented."""
    body = function_text(lines, name).split("\n")
    start = next(i for i, l in enumerate(body) if l.strip() == "lab2 = ''.join(lab2)") + 1
    end = next(i for i in range(start, len(body)) if body[i].strip().startswith("return"))
    return textwrap.dedent("\n".join(l for l in body[start:end] if l.strip()))


def clip_defaults(lines, name):
    ns = {}
    exec(function_text(lines, name).replace(f"def {name}(", "def f(").split("\n")[0] + "\n    "
         "return minimum_clip, maximum_clip", ns)
    return ns["f"](None)


def stored_value(block, lab1, lab2, ns, gamma=None):
    ns = dict(ns, lab1=lab1, lab2=lab2, dist_dict={lab1: {}},
              args=argparse.Namespace(dist_gamma=gamma))
    exec(block, ns)
    return ns["dist_dict"][lab1][lab2]


def record(name, patterns, targets):
    lines = source_lines()
    ns = {"np": np}
    exec(function_text(lines, "str_jac_similarity"), ns)
    exec(function_text(lines, "str_ham_similarity"), ns)
    plain = {"indication": pair_block(lines, "indication_similarity"),
             "constant": pair_block(lines, "constant_similarity"),
             "jaccard": pair_block(lines, "_jaccard_similarity")}
    nonlinear = {"jaccard": ("_jaccard_nonlinear_similarity",
                             pair_block(lines, "_jaccard_nonlinear_similarity")),
                 "hamming": ("_hamming_nonlinear_similarity",
                             pair_block(lines, "_hamming_nonlinear_similarity"))}
    # the nonlinear statements after `sim = ...`, for a given sim
    jn = nonlinear["jaccard"][1].split("\n")
    assert jn[0].startswith("sim = "), jn[0]
    from_sim = "\n".join(jn[1:])
    keys = ["".join(str(int(v)) for v in row) for row in patterns]
    tkeys = ["".join(str(int(v)) for v in row) for row in targets]
    values = np.zeros((len(KINDS), len(GAMMAS), len(tkeys), len(keys)), np.float64)
    np64 = np.zeros((len(KINDS), len(GAMMAS)), np.int8)
    for ki, kind in enumerate(KINDS):
        for gi, gamma in enumerate(GAMMAS):
            types = set()
            for ti, lab1 in enumerate(tkeys):
                for pi, lab2 in enumerate(keys):
                    if gamma != gamma:
                        if kind == "hamming":  # _hamming_similarity raises as written
                            v = ns["str_ham_similarity"](lab1, lab2)
                        else:
                            v = stored_value(plain[kind], lab1, lab2, ns)
                    elif kind in nonlinear:
                        fn, block = nonlinear[kind]
                        lo, hi = clip_defaults(lines, fn)
                        v = stored_value(block, lab1, lab2,
                                         dict(ns, minimum_clip=lo, maximum_clip=hi), gamma)
                    else:
                        lo, hi = clip_defaults(lines, nonlinear["jaccard"][0])
                        sim = stored_value(plain[kind], lab1, lab2, ns)
                        v = stored_value(from_sim, lab1, lab2,
                                         dict(ns, sim=sim, minimum_clip=lo, maximum_clip=hi), gamma)
                    types.add(type(v))
                    values[ki, gi, ti, pi] = v
            assert len(types) == 1, (kind, gamma, types)
            np64[ki, gi] = int(types.pop() is np.float64)
    path = os.path.join(HERE, f"labelsim_{name}.npz")
    np.savez_compressed(path, patterns=patterns.astype(np.uint8), targets=targets.astype(np.uint8),
                        kinds=np.array(KINDS), gammas=np.array(GAMMAS), values=values, np64=np64)
    print(name, "patterns", patterns.shape, "targets", targets.shape, os.path.getsize(path),
          "bytes; np64", np64.tolist())


def main():
    # s1: one word.  Targets: a random pattern, the all-zero pattern (Jaccard's
    # 0/0 against the all-zero row is settled by the identity rule), a dense one.
    rng = np.random.default_rng(2025)
    L = 25
    targets = np.stack([(rng.random(L) < 0.3), np.zeros(L, bool), (rng.random(L) < 0.7)])
    targets[0, :2] = (True, False)
    rows = [targets[0], targets[1], targets[2], np.ones(L, bool), ~targets[0], ~targets[2]]
    for j in (0, 1, L - 1):  # one bit away from target 0
        r = targets[0].copy()
        r[j] = ~r[j]
        rows.append(r)
    rows += [rng.random(L) < p for p in (0.1, 0.3, 0.5) for _ in range(10)]
    rows.append(targets[0] & (rng.random(L) < 0.5))  # a subset of target 0
    record("s1_l25", np.stack(rows).astype(np.uint8), targets.astype(np.uint8))

    # s2: three words; every pattern equals the base in words 0 and 1 and
    # differs from it in word 2 (labels 128, 129) only, beside the all-zero,
    # all-one and complement patterns.
    L = 130
    base = rng.random(L) < 0.4
    variants = []
    for a in (False, True):
        for b in (False, True):
            r = base.copy()
            r[128], r[129] = a, b
            variants.append(r)
    targets = np.stack([variants[1], np.zeros(L, bool), variants[2]])
    rows = variants + [np.zeros(L, bool), np.ones(L, bool), ~variants[1]]
    record("s2_l130", np.stack(rows).astype(np.uint8), targets.astype(np.uint8))


if __name__ == "__main__":
    main()
