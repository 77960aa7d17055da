"""CPU: the host side of mpvae_fair.py that needs no GPU (group_ids,
sensitive_groups, the pattern table's build) and the conditions that the case
builders of tests/fair_cases.py must meet for tests/test_gpu_fair_edges.py to
mean what it says (they are conditions on the inputs, checked with the oracle
and the host table only)."""
import numpy as np
import pytest
import torch

import fair_cases as fc
import mpvae_fair as mf
from oracle import fairness as of


# ------------------------------------------------------------------ groups
def test_group_ids_match_torch_unique():
    fc.check_groups(mf, "cpu")


def test_max_groups_zero_raises():
    with pytest.raises(ValueError):
        mf.sensitive_groups(torch.zeros(4, 2), max_groups=0)


@pytest.mark.parametrize("shape", [(0, 2), (0, 1), (0,), (0, 2, 3)])
def test_groups_of_an_empty_batch(shape):
    fc.check_empty_groups(mf, "cpu", shape)


# ----------------------------------------------------------- pattern table
@pytest.mark.parametrize("L", [3, 5])
def test_all_patterns_seed_displaces_a_key_and_wraps(L):
    """The seeded half-full table has a stored key off its home slot, and a
    lookup whose probe chain steps from the last slot to slot 0."""
    c = fc.all_patterns_case(L)
    tab = mf.LabelDistanceTable(c["dists"][0], L, "cpu")
    assert tab.nslots == 2 ** L and len(c["dists"][0]) == 2 ** L // 2
    displaced = wraps = False
    for row in c["labels"]:
        key = fc.key_of(row)
        seen = fc.probe_slots(tab, mf.pack_pattern(key, L))
        displaced |= key in c["dists"][0] and len(seen) > 1
        wraps |= any(a == tab.nslots - 1 and b == 0 for a, b in zip(seen, seen[1:]))
    assert displaced and wraps


def test_tables_without_a_usable_key_are_empty():
    assert mf.LabelDistanceTable({}, 5, "cpu").nslots == 0
    bad = {"0101": 1.0, "010101": 2.0, "01012": 3.0, "": 4.0}
    assert mf.LabelDistanceTable(bad, 5, "cpu").nslots == 0
    one = mf.LabelDistanceTable({"01010": np.float64(0.3)}, 5, "cpu")
    assert one.nslots == 2 and int(one.used.sum()) == 1


@pytest.mark.parametrize("L", fc.LW_L)
def test_pair_rows_differ_in_one_label_and_reach_every_index(L):
    reached = set()
    for B in fc.LW_B:
        lab = fc.weight_pair_case(L, B)["labels"]
        for b in range(1, B, 2):
            diff = np.flatnonzero(lab[b] != lab[b - 1])
            assert len(diff) == 1
            reached.add(int(diff[0]))
    assert reached == set(fc.flip_indices(L))


# -------------------------------------------------- fairness penalty cases
def test_penalty_lattice_covers_every_axis_with_both_norms():
    lat = fc.penalty_lattice()
    assert len(lat) == 40 and len({fc.lattice_id(c) for c in lat}) == 40
    for norm in fc.FP_NORMS:
        mine = [c for c in lat if c["norm"] == norm]
        for axis, values in (("L", fc.FP_L), ("B", fc.FP_B), ("T", fc.FP_T),
                             ("groups", fc.FP_GROUPS), ("maxg", fc.FP_MAXG)):
            assert {c[axis] for c in mine} == set(values), (norm, axis)


def _all_penalty_cases():
    out = [(fc.lattice_id(p), fc.penalty_case(**p)) for p in fc.penalty_lattice()]
    for norm in fc.FP_NORMS:
        out.append((f"dead-{norm}", fc.dead_target_group_case(norm)))
        out.append((f"wide-{norm}", fc.wide_weights_case(norm)))
        out.append((f"zero-{norm}", fc.exact_zero_case(norm)))
        out.append((f"pyfloat-{norm}", fc.penalty_case(257, 7, 3, 2, norm, pyfloat=True)))
    return out


def test_l1_cases_stay_away_from_the_sign_jump():
    """Every l1 case with more than one sensitive group has min |d| >= 1e-9
    over all (target, group, label) -- except on the columns that
    exact_zero_case builds to be exactly 0; the single-group ones are exactly
    0 in the oracle (loss and every gradient element)."""
    for name, c in _all_penalty_cases():
        loss, _, gl, gf, min_d = of.fair_penalty(c["label_z"], c["feat_z"], c["labels"],
                                                 c["sensitive"], c["dists"], c["norm"],
                                                 c["coeff"], return_min_d=True)
        assert loss is not None, name
        if fc.n_groups(c["sensitive"]) == 1:
            assert loss == 0.0 and not gl.any() and not gf.any(), name
        elif c["norm"] == "l1":
            assert fc.l1_condition(c, min_d), (name, min_d.min())
        if "zero_cols" in c:  # both norms: d = 0, so no gradient on those columns
            assert fc.n_groups(c["sensitive"]) == 2 and (min_d[c["zero_cols"]] == 0).all()
            assert not gl[:, c["zero_cols"]].any() and not gf[:, c["zero_cols"]].any()
            assert gl[:, ~c["zero_cols"]].any(1).all()


def test_constructed_penalty_cases_are_what_they_claim():
    c = fc.dead_target_group_case("l1")
    w = np.stack([of.row_weights(c["labels"], d) for d in c["dists"]])
    assert w[1].sum() == 0 and w[0].sum() > 0 and w[2].sum() > 0
    dead = (c["sensitive"] == 5).all(1)
    assert dead.sum() == 8 and w[:, dead].sum() == 0 and fc.n_groups(c["sensitive"]) == 3
    c = fc.wide_weights_case("l2")
    w = np.stack([of.row_weights(c["labels"], d) for d in c["dists"]])
    assert not w[:, [5, 6, 20]].any()
    live = w[w > 0]
    assert live.max() / live.min() >= 1e6
    *_, gl, gf = of.fair_penalty(c["label_z"], c["feat_z"], c["labels"], c["sensitive"],
                                 c["dists"], "l2", c["coeff"])
    assert not gl[[5, 6, 20]].any() and not gf[[5, 6, 20]].any()


def test_oracle_order_sensitivity_is_at_rounding_level():
    """s, the term of the per-row gradient tolerance that comes from the
    oracle itself: the oracle on permuted rows against the oracle."""
    for norm in fc.FP_NORMS:
        c = fc.wide_weights_case(norm)
        p, perm = fc.permuted_rows(c)
        a = of.fair_penalty(c["label_z"], c["feat_z"], c["labels"], c["sensitive"], c["dists"],
                            norm, c["coeff"])
        b = of.fair_penalty(p["label_z"], p["feat_z"], p["labels"], p["sensitive"], p["dists"],
                            norm, c["coeff"])
        for g, gp in ((a[2], b[2]), (a[3], b[3])):
            back = np.empty_like(gp)
            back[perm] = gp
            assert fc.row_rel_err(back, g) <= 1e-12


# ----------------------------------------------------------- metric cases
def test_metric_lattice_cases_have_a_true_label():
    for L in fc.MET_L:
        for B in fc.MET_B:
            p, t = fc.metrics_case(L, B)
            assert p.shape == t.shape == (B, L) and t.sum() >= 1


@pytest.mark.parametrize("build, pk", [
    (fc.tie_all_equal, (1, 2 / 3, 3 / 5)),
    (fc.tie_pairs, (1, 1 / 3, 1 / 5)),
    (fc.five_on_one_thread, (1, 2 / 3, 3 / 5)),
    (fc.inf_scores, (1, 2 / 3, 3 / 5)),
    (fc.all_neg_inf_l3, (1, 2 / 3, 2 / 5)),
], ids=["all_equal", "pairs", "one_thread", "inf", "neg_inf_l3"])
def test_oracle_tie_rule_on_constructed_rows(build, pk):
    """The oracle's stated rule (larger score, then larger index) gives the
    p@k that the constructions were made for; any other pick moves them."""
    p, t = build()
    v = of.train_metrics(p, t, 0.5)
    assert np.allclose(v[5:], pk, rtol=1e-15), v[5:]
    if build is fc.tie_pairs:  # the smaller index of each pair holds a false target
        for b, (i, j) in enumerate(fc.TIE_PAIRS):
            assert p[b, i] == p[b, j] == p[b].max() and t[b, j] == 1 and t[b, i] == 0


def test_threshold_and_dead_rows_constructions():
    for thr in fc.MET_THR:
        p, t = fc.at_threshold(thr)
        assert (p == np.float32(thr)).sum() == 80 and t[p == np.float32(thr)].sum() == 40
        below = np.nextafter(np.float32(thr), np.float32(0))
        assert (p == below).sum() == 80 and t[p == below].sum() == 40
    p, t = fc.one_live_row()
    assert not t[:-1].any() and not (p[:-1] >= 0.5).any() and t[-1].any()
    p, t = fc.dead_label()
    assert not t[:, 2].any() and not (p[:, 2] >= 0.5).any()
    v = of.train_metrics(p, t, 0.5)
    f = []  # per-label F1 by hand: tp, fp, fn over the two rows
    for l in range(6):
        pr, tr = p[:, l] >= 0.5, t[:, l] == 1
        tp, fp, fn = (pr & tr).sum(), (pr & ~tr).sum(), (~pr & tr).sum()
        f.append(2 * tp / (2 * tp + fp + fn + 1e-6))
    assert f[2] == 0 and abs(v[4] - np.mean(f)) <= 1e-6
