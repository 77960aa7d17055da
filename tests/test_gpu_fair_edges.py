"""GPU: csrc/fairness.hip through mpvae_fair.py at the edges of its kernels,
against oracle/fairness.py (numpy, fp64; pinned to the reference's own code by
the goldens of tests/test_oracle_fair.py).  The cases come from
tests/fair_cases.py, the bounds from tests/tolerances.py; with
MPVAE_RECORD_ERRS set every penalty and metric case records its measured
error (and the oracle's own order sensitivity s) -- profiles/fair_edges_errs.jsonl.

1. label_weights_kernel: word boundaries, the W = 64 limit, partial workgroups
   of rows, probe chains that wrap, empty and one-entry tables, stored zeros,
   non-fp32 values, non-binary label values, several tables per call.
2. fair_fwd_kernel / fair_bwd_kernel: L past one workgroup with and without a
   tail, one group (exact zeros), d = 0 with two live groups (sgn(0) = 0),
   dead targets and groups, a per-row gradient
   bound, the other ways into the backward, determinism.
3. metric_rows_kernel and the metrics after it: L < 5, ties, five winners on
   one thread, infinite scores, scores at the threshold, other thresholds.
4. group_ids / sensitive_groups on the device.
5. The empty batch and the empty table list."""
import functools

import numpy as np
import pytest
import torch

import fair_cases as fc
import mpvae_fair as mf
import mpvae_hip as H
import tolerances as T
from oracle import fairness as of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------- 1. label weights
def _lookup(labels, dists):
    """label_weights against row_weights, bit for bit, and the count."""
    L = labels.shape[1]
    tables = [mf.LabelDistanceTable(d, L, DEV) for d in dists]
    w, count = mf.label_weights(torch.from_numpy(labels).to(DEV), tables)
    ref = np.stack([of.row_weights(labels, d) for d in dists])
    assert w.dtype == torch.float64 and tuple(w.shape) == ref.shape
    assert np.array_equal(w.cpu().numpy(), ref), (w.cpu().numpy(), ref)
    assert int(count) == int((ref > 0).sum())
    return ref


@pytest.mark.parametrize("B", fc.LW_B)
@pytest.mark.parametrize("L", fc.LW_L)
def test_label_weights_one_label_apart(L, B):
    c = fc.weight_pair_case(L, B)
    ref = _lookup(c["labels"], c["dists"])
    assert (ref[0, ::2] > 0).all()     # the dict members hit


@pytest.mark.parametrize("L", [3, 5])
def test_label_weights_every_pattern_half_full_table(L):
    c = fc.all_patterns_case(L)
    ref = _lookup(c["labels"], c["dists"])
    assert int((ref > 0).sum()) == 2 ** L // 2


def test_label_weights_degenerate_tables():
    rng = np.random.default_rng(41)
    labels = rng.integers(0, 2, (6, 70))
    keys = [fc.key_of(r) for r in labels]
    assert not _lookup(labels, [{}]).any()                                   # nslots 0
    assert not _lookup(labels, [{keys[0][:-1]: 1.0, "2" + keys[1][1:]: 1.0}]).any()
    assert _lookup(labels, [{keys[3]: np.float64(0.25)}])[0, 3] == 0.25       # one entry
    # stored zeros: present, weight 0, not counted
    ref = _lookup(labels, [{keys[0]: 0.0, keys[1]: np.float64(0.0), keys[2]: 0.5}])
    assert list(ref[0]) == [0, 0, 0.5, 0, 0, 0]
    # float64 values that fp32 cannot hold come back bit for bit
    vals = [np.float64(0.1), np.float64(1) / 3, np.float64(1 + 2.0 ** -40), np.float64(1e-300),
            np.float64(1e300), np.float64(np.pi)]
    ref = _lookup(labels, [dict(zip(keys, vals))])
    with np.errstate(all="ignore"):
        assert all(np.float32(v) != v for v in vals)
    assert list(ref[0]) == vals


def test_label_weights_non_binary_values():
    """Float label values: the reference's astype(int) decides (0.5 and -0.5
    are 0, 1.9 is 1, 2.0 and -1.0 have no binary key)."""
    rng = np.random.default_rng(42)
    base = rng.integers(0, 2, 65)
    rows, dist = [base.astype(np.float32)], {fc.key_of(base): np.float64(0.5)}
    for pos in (0, 63, 64):
        other = base.copy()
        other[pos] ^= 1
        dist[fc.key_of(other)] = np.float64(0.1 + pos / 100)
        for v in (2.0, 0.5, 1.9, -0.5, -1.0):
            rows.append(base.astype(np.float32))
            rows[-1][pos] = v
    ref = _lookup(np.stack(rows), [dist])
    assert (ref[0].reshape(-1)[1:].reshape(3, 5)[:, [0, 4]] == 0).all()       # 2.0 and -1.0 miss
    assert (ref[0].reshape(-1)[1:].reshape(3, 5)[:, [1, 2, 3]] > 0).all()     # the others hit


def test_label_weights_int64_and_float32_rows_agree():
    c = fc.weight_pair_case(129, 9)
    a = _lookup(c["labels"], c["dists"])
    b = _lookup(c["labels"].astype(np.float32), c["dists"])
    assert np.array_equal(a, b)


def test_label_weights_three_tables_one_call():
    rng = np.random.default_rng(43)
    labels = rng.integers(0, 2, (9, 130))
    keys = [fc.key_of(r) for r in labels]
    dists = [{k: np.float64(rng.uniform(0.1, 1)) for k in keys[i::2]} for i in range(2)]
    dists.append({keys[4]: 0.75})
    for _ in range(2):      # the count starts from zero in every call
        ref = _lookup(labels, dists)
    assert [int((r > 0).sum()) for r in ref] == [5, 4, 1]


# ---------------------------------------------------- 2. fairness penalty
def _penalty_cases():
    cases = {fc.lattice_id(p): fc.penalty_case(**p) for p in fc.penalty_lattice()}
    for norm in fc.FP_NORMS:
        cases[f"one-group-{norm}"] = fc.penalty_case(257, 8, 2, 1, norm, seed=50)
        cases[f"dead-{norm}"] = fc.dead_target_group_case(norm)
        cases[f"wide-{norm}"] = fc.wide_weights_case(norm)
        cases[f"zero-{norm}"] = fc.exact_zero_case(norm)
        cases[f"pyfloat-{norm}"] = fc.penalty_case(257, 7, 3, 2, norm, pyfloat=True)
    return cases


CASES = _penalty_cases()
LATTICE = [fc.lattice_id(p) for p in fc.penalty_lattice()]


def _of(c):
    return of.fair_penalty(c["label_z"], c["feat_z"], c["labels"], c["sensitive"], c["dists"],
                           c["norm"], c["coeff"], return_min_d=True)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's answer for a case, computed once and shared, and s: the
    oracle on the rows in a fixed permutation against itself, per row."""
    c = CASES[name]
    loss, count, gl, gf, min_d = _of(c)
    p, perm = fc.permuted_rows(c)
    _, _, pl, pf, _ = _of(p)
    s = 0.0
    for g, gp in ((gl, pl), (gf, pf)):
        back = np.empty_like(gp)
        back[perm] = gp
        s = max(s, fc.row_rel_err(back, g))
    for a in (gl, gf):
        a.setflags(write=False)
    return dict(loss=loss, count=count, gl=gl, gf=gf, min_d=min_d, s=s)


def _leaf(a, dtype=torch.float32, transposed=False):
    t = torch.from_numpy(a).to(DEV, dtype)
    if transposed:  # the same values behind a (B, L) view of an (L, B) buffer
        t = t.t().contiguous().t()
    return t.requires_grad_(True)


def _run(c, objective=lambda loss: loss, dtype=torch.float32, transposed=False):
    L = c["labels"].shape[1]
    tables = [mf.LabelDistanceTable(d, L, DEV) for d in c["dists"]]
    lz, fz = _leaf(c["label_z"], dtype, transposed), _leaf(c["feat_z"], dtype, transposed)
    loss, count = mf.fairness_penalty(lz, fz, torch.from_numpy(c["labels"]).to(DEV),
                                      torch.from_numpy(c["sensitive"]).to(DEV), tables,
                                      c["norm"], c["coeff"], max_groups=c["max_groups"])
    objective(loss).backward()
    return loss.detach(), count, lz, fz


def _check(name, loss, count, gl, gf, gscale=1.0, loss_rtol=T.FAIR_LOSS_RTOL, tag=""):
    c, r = CASES[name], _oracle(name)
    single = fc.n_groups(c["sensitive"]) == 1
    if c["norm"] == "l1" and not single:  # a bad seed fails here, loudly
        assert fc.l1_condition(c, r["min_d"]), r["min_d"].min()
    assert int(count) == r["count"]
    tol = T.fair_row_grad_tol(r["s"])
    errs = dict(s=r["s"], tol=tol,
                loss=abs(float(loss) - r["loss"]) / abs(r["loss"]) if r["loss"] else
                abs(float(loss)),
                g_label_z=fc.row_rel_err(gl.cpu().numpy(), gscale * r["gl"]),
                g_feat_z=fc.row_rel_err(gf.cpu().numpy(), gscale * r["gf"]))
    T.record(f"fair_edges/{name}{tag}", errs)
    print(name + tag, errs)
    assert abs(float(loss) - r["loss"]) <= loss_rtol * abs(r["loss"]), errs
    assert errs["g_label_z"] <= tol and errs["g_feat_z"] <= tol, errs
    if single:  # one group: every difference of means is exactly 0, sgn(0) = 0
        assert float(loss) == 0.0 and not gl.any() and not gf.any()


@pytest.mark.parametrize("name", LATTICE)
def test_fair_penalty_lattice(name):
    loss, count, lz, fz = _run(CASES[name])
    assert loss.dtype == torch.float64 and lz.grad.dtype == torch.float32
    _check(name, loss, count, lz.grad, fz.grad)


@pytest.mark.parametrize("norm", fc.FP_NORMS)
@pytest.mark.parametrize("kind", ["one-group", "dead", "wide", "zero"])
def test_fair_penalty_constructed(kind, norm):
    name = f"{kind}-{norm}"
    loss, count, lz, fz = _run(CASES[name])
    _check(name, loss, count, lz.grad, fz.grad)
    if kind == "wide":  # rows in no dict: exactly zero, whatever the tolerance
        assert not lz.grad[[5, 6, 20]].any() and not fz.grad[[5, 6, 20]].any()
    if kind == "zero":  # d = 0 with two live groups: sgn(0) = 0, no gradient there
        cols = torch.from_numpy(CASES[name]["zero_cols"]).to(DEV)
        assert not lz.grad[:, cols].any() and not fz.grad[:, cols].any()
        assert lz.grad[:, ~cols].any() and fz.grad[:, ~cols].any()


@pytest.mark.parametrize("norm", fc.FP_NORMS)
def test_fair_penalty_other_gradient_paths(norm):
    name = f"wide-{norm}"
    c, r = CASES[name], _oracle(name)
    loss0, count, lz0, fz0 = _run(c)
    # a scaled objective
    loss, count, lz, fz = _run(c, lambda x: 2.5 * x)
    _check(name, loss, count, lz.grad, fz.grad, gscale=2.5, tag="/scaled")
    # the loss used twice: d (loss^2 + loss) = (2 loss + 1) d loss
    loss, count, lz, fz = _run(c, lambda x: x * x + x)
    _check(name, loss, count, lz.grad, fz.grad, gscale=2 * r["loss"] + 1, tag="/twice")
    # fp64 inputs: the same values, gradients in fp64
    loss, count, lz, fz = _run(c, dtype=torch.float64)
    assert lz.grad.dtype == fz.grad.dtype == torch.float64 and torch.equal(loss, loss0)
    assert torch.equal(lz.grad, lz0.grad.double()) and torch.equal(fz.grad, fz0.grad.double())
    _check(name, loss, count, lz.grad, fz.grad, tag="/fp64")
    # transposed views: the gradient in the input's dtype and layout
    loss, count, lz, fz = _run(c, transposed=True)
    assert lz.stride() == (1, lz.shape[0]) and lz.grad.stride() == lz.stride()
    assert lz.grad.dtype == torch.float32 and fz.grad.stride() == fz.stride()
    assert torch.equal(loss, loss0)
    assert torch.equal(lz.grad, lz0.grad) and torch.equal(fz.grad, fz0.grad)
    _check(name, loss, count, lz.grad, fz.grad, tag="/transposed")


@pytest.mark.parametrize("norm", fc.FP_NORMS)
def test_fair_penalty_fp32_loss_path_l257(norm):
    """Tables of Python floats: the loss comes back in fp32, the fp64 value
    rounded once; the gradients as ever."""
    name = f"pyfloat-{norm}"
    loss, count, lz, fz = _run(CASES[name])
    assert loss.dtype == torch.float32
    _check(name, loss, count, lz.grad, fz.grad, loss_rtol=T.FAIR_LOSS_F32_RTOL)


@pytest.mark.parametrize("name", ["l1-L513-B33-T1-g2-mgNone", "wide-l2"])
def test_fair_penalty_is_deterministic(name):
    assert name in CASES
    a, b = _run(CASES[name]), _run(CASES[name])
    assert torch.equal(a[0], b[0]) and int(a[1]) == int(b[1])
    assert torch.equal(a[2].grad, b[2].grad) and torch.equal(a[3].grad, b[3].grad)


# --------------------------------------------------------- 3. train metrics
COUNTS, F1S = [0, 1, 5, 6, 7], [2, 3, 4]   # ACC, HA, p@1/3/5 | ebF1, miF1, maF1


def _metrics(p, t, thr):
    res = mf.compute_metrics(torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV), thr)
    return np.array([float(res[k]) for k in mf.METRIC_KEYS])


def _check_metrics(name, p, t, thr):
    v, r = _metrics(p, t, thr), of.train_metrics(p, t, thr)
    B = p.shape[0]
    assert np.isfinite(r).all(), r
    err = np.abs(v - r)
    T.record(f"fair_edges/metrics/{name}", dict(zip(mf.METRIC_KEYS, err)))
    assert (err[COUNTS] <= B * T.METRIC_COUNT_ULP * np.abs(r[COUNTS])).all(), (v, r)
    assert np.allclose(v[F1S], r[F1S], rtol=T.METRIC_F1_RTOL, atol=T.METRIC_F1_ATOL), (v, r)
    return v


@pytest.mark.parametrize("thr", fc.MET_THR)
@pytest.mark.parametrize("B", fc.MET_B)
@pytest.mark.parametrize("L", fc.MET_L)
def test_train_metrics_lattice(L, B, thr):
    p, t = fc.metrics_case(L, B)
    _check_metrics(f"L{L}-B{B}-thr{thr}", p, t, thr)


@pytest.mark.parametrize("build, pk", [
    (fc.tie_all_equal, (1, 2 / 3, 3 / 5)),
    (fc.tie_pairs, (1, 1 / 3, 1 / 5)),
    (fc.five_on_one_thread, (1, 2 / 3, 3 / 5)),
    (fc.inf_scores, (1, 2 / 3, 3 / 5)),
    (fc.all_neg_inf_l3, (1, 2 / 3, 2 / 5)),
], ids=["all_equal", "pairs", "one_thread", "inf", "neg_inf_l3"])
def test_train_metrics_top5_rule(build, pk):
    """Larger score first, then the larger index (the oracle's stated rule;
    the reference's own tie order is implementation-defined).  The p@k values
    are the ones the rows were built for (tests/test_fair_host.py)."""
    p, t = build()
    v = _check_metrics(build.__name__, p, t, 0.5)
    assert np.allclose(v[5:], pk, rtol=p.shape[0] * T.METRIC_COUNT_ULP, atol=0), v[5:]
    if build is fc.tie_pairs:  # each pair on its own: the rows do not average out
        for b, pair in enumerate(fc.TIE_PAIRS):
            vb = _check_metrics(f"tie_pair_{pair[0]}_{pair[1]}", p[b:b + 1], t[b:b + 1], 0.5)
            assert vb[5] == 1.0, (pair, vb)


@pytest.mark.parametrize("thr", fc.MET_THR)
def test_train_metrics_score_at_threshold_predicts_one(thr):
    p, t = fc.at_threshold(thr)
    _check_metrics(f"at_threshold_{thr}", p, t, thr)
    # by hand: the 20 true labels per row that sit at thr are true positives
    at = p == np.float32(thr)
    assert at.sum() == 80 and t[at].sum() == 40
    flipped = p.copy()
    flipped[at] = np.nextafter(np.float32(thr), np.float32(0))
    assert _metrics(p, t, thr)[3] > _metrics(flipped, t, thr)[3]   # miF1 loses them


def test_train_metrics_dead_rows_and_dead_label():
    p, t = fc.one_live_row()
    v = _check_metrics("one_live_row", p, t, 0.5)
    live = _metrics(p[-1:], t[-1:], 0.5)
    assert abs(v[2] - live[2]) <= 1e-7       # ebF1 is the live row's alone
    p, t = fc.dead_label()
    _check_metrics("dead_label", p, t, 0.5)


# ------------------------------------------------------------- 4. groups
def test_group_ids_on_the_device():
    fc.check_groups(mf, DEV)


# -------------------------------------------------------- 5. empty edges
@pytest.mark.parametrize("shape", [(0, 2), (0,)])
def test_groups_of_an_empty_batch_on_the_device(shape):
    fc.check_empty_groups(mf, DEV, shape)


@pytest.mark.parametrize("kind", ["empty_batch", "no_tables"])
@pytest.mark.parametrize("pyfloat", [False, True])
def test_fair_penalty_empty_edges(kind, pyfloat):
    """B = 0 with tables, and tables = [] at B = 7: the reference leaves
    fairloss = 0. -- a finite 0-d fp64 zero on the device, count 0, zero
    gradient through it, and no launch of a fairness kernel."""
    L, B = 257, 0 if kind == "empty_batch" else 7
    rng = np.random.default_rng(51)
    v = 0.5 if pyfloat else np.float64(0.5)
    tables = [] if kind == "no_tables" else [
        mf.LabelDistanceTable({fc.key_of(rng.integers(0, 2, L)): v}, L, DEV) for _ in range(2)]
    lz = _leaf(rng.uniform(0.01, 0.99, (B, L)).astype(np.float32))
    fz = _leaf(rng.uniform(0.01, 0.99, (B, L)).astype(np.float32))
    labels = torch.from_numpy(rng.integers(0, 2, (B, L))).to(DEV)
    sens = torch.from_numpy(rng.integers(0, 2, (B, 2))).to(DEV)
    lib = H.load_library()
    lib.mpv_timing_reset()
    lib.mpv_timing_enable(1)
    try:
        loss, count = mf.fairness_penalty(lz, fz, labels, sens, tables, "l1", 0.75)
        other = (2.0 * lz).sum() + fz.sum()
        (other + loss).backward()
        torch.cuda.synchronize()
        launched = H.kernel_times()
    finally:
        lib.mpv_timing_enable(0)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.is_cuda
    assert float(loss.detach()) == 0.0 and int(count) == 0 and count.is_cuda
    assert not {"label_weights", "fair_fwd", "fair_bwd"} & set(launched), launched
    assert torch.equal(lz.grad, torch.full_like(lz, 2.0))
    assert torch.equal(fz.grad, torch.ones_like(fz))
    # on its own the zero is still differentiable, with exactly zero gradients
    lz.grad = fz.grad = None
    loss, _ = mf.fairness_penalty(lz, fz, labels, sens, tables, "l2", 0.75, max_groups=1)
    loss.backward()
    assert lz.grad.shape == lz.shape and not lz.grad.any() and not fz.grad.any()
