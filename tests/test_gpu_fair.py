"""GPU: the device fairness regulariser, label-pattern weights and train
metrics (csrc/fairness.hip through mpvae_fair.py) against the golden vectors
recorded from the reference and against the oracle at training sizes."""
import numpy as np
import pytest
import torch

import mpvae_fair as mf
from fair_io import fair_fixtures, metric_fixtures
from oracle import fairness as of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAIR = fair_fixtures()
MET = metric_fixtures()


def _run(f, dists=None, norm=None, coeff=None):
    dists = f["dists"] if dists is None else dists
    L = f["labels"].shape[1]
    tables = [mf.LabelDistanceTable(d, L, DEV) for d in dists]
    lz = torch.from_numpy(f["label_z"]).to(DEV).requires_grad_(True)
    fz = torch.from_numpy(f["feat_z"]).to(DEV).requires_grad_(True)
    loss, count = mf.fairness_penalty(lz, fz, torch.from_numpy(f["labels"]).to(DEV),
                                      torch.from_numpy(f["sensitive"]).to(DEV), tables,
                                      f["norm"] if norm is None else norm,
                                      f["coeff"] if coeff is None else coeff)
    loss.backward()
    return loss, count, lz.grad, fz.grad


@pytest.mark.parametrize("f", FAIR, ids=[f["name"] for f in FAIR])
def test_fair_penalty_matches_reference(f):
    loss, count, gl, gf = _run(f)
    assert int(count) == int(f["contributed"])
    if not int(f["active"]):
        assert float(loss.detach()) == 0.0 and float(gl.abs().max()) == 0.0
        return
    ref = float(f["fairloss"])
    assert str(loss.dtype) == "torch." + str(f["ref_dtype"])
    if f["pyfloat"]:
        # the reference ran in fp32 (Python-float distances), the kernels in fp64
        ltol, gtol = 1e-7, 1e-6
    else:
        # fp64 on both sides, fp32 at the leaf: a few fp32 ulps
        ltol, gtol = 1e-12, 1e-6
    # a fp32 loss carries the fp64 value rounded once
    if loss.dtype == torch.float32:
        ltol = max(ltol, 1.2e-7)
    assert abs(float(loss.detach()) - ref) <= ltol * abs(ref)
    for g, r in ((gl, f["g_label_z"]), (gf, f["g_feat_z"])):
        assert np.abs(g.cpu().numpy() - r).max() <= gtol * np.abs(r).max()


@pytest.mark.parametrize("norm", ["l1", "l2"])
def test_fair_penalty_training_size_against_oracle(norm):
    rng = np.random.default_rng(7)
    B, L = 512, 1024
    labels = (rng.random((B, L)) < 0.02).astype(np.int64)
    labels[256:] = labels[:256]
    sens = rng.integers(0, 3, (B, 2)).astype(np.int64)
    # numpy float64 distances (label_distance*.py's np.clip): the reference's
    # weights tensor is then float64, and so is the returned loss
    dists = [{"".join(r.astype(str)): np.float64(rng.uniform(0.1, 1)) for r in labels[i::7]}
             for i in range(3)]
    f = dict(labels=labels, sensitive=sens, dists=dists, norm=norm, coeff=0.5,
             label_z=rng.uniform(0.01, 0.99, (B, L)).astype(np.float32),
             feat_z=rng.uniform(0.01, 0.99, (B, L)).astype(np.float32))
    loss, count, gl, gf = _run(f)
    rl, rc, rgl, rgf = of.fair_penalty(f["label_z"], f["feat_z"], labels, sens, dists, norm, 0.5)
    assert int(count) == rc
    assert loss.dtype == torch.float64
    assert abs(float(loss.detach()) - rl) <= 1e-10 * abs(rl)
    for g, r in ((gl, rgl), (gf, rgf)):
        assert np.abs(g.cpu().numpy() - r).max() <= 1e-6 * np.abs(r).max()


def test_label_weights_multiword_and_misses():
    rng = np.random.default_rng(3)
    B, L = 64, 200
    labels = (rng.random((B, L)) < 0.1).astype(np.float32)
    labels[5, 7] = 2.0                         # int() not 0/1: a miss, as in the reference
    d = {"".join(r.astype(int).astype(str)): float(i + 1) for i, r in enumerate(labels[::2])}
    tab = mf.LabelDistanceTable(d, L, DEV)
    w, count = mf.label_weights(torch.from_numpy(labels).to(DEV), [tab])
    ref = of.row_weights(labels, d)
    assert np.array_equal(w.cpu().numpy()[0], ref)
    assert int(count) == int((ref > 0).sum())


@pytest.mark.parametrize("m", MET, ids=[m["name"] for m in MET])
def test_train_metrics_match_reference(m):
    res = mf.compute_metrics(torch.from_numpy(m["pred"]).to(DEV),
                             torch.from_numpy(m["target"]).to(DEV), m["threshold"])
    v = np.array([float(res[k]) for k in mf.METRIC_KEYS])
    assert np.allclose(v, m["values"], rtol=1e-6, atol=1e-7), (v, m["values"])


def test_train_metrics_training_size_against_oracle():
    rng = np.random.default_rng(11)
    B, L = 512, 1024
    t = (rng.random((B, L)) < 0.05).astype(np.float32)
    p = rng.random((B, L)).astype(np.float32)
    res = mf.compute_metrics(torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV), 0.5)
    v = np.array([float(res[k]) for k in mf.METRIC_KEYS])
    assert np.allclose(v, of.train_metrics(p, t, 0.5), rtol=2e-6, atol=1e-7)


def test_fair_penalty_is_graph_capturable():
    """fairness_penalty forward + backward with no host sync: captured in a HIP
    graph, replays on new batch contents equal eager calls (SURVEY 8(f) rank
    3); a max_groups bound gives the same value as the default bound.  The
    warm-up's autograd graph is dropped before the capture, so the leaves'
    AccumulateGrad nodes are rebuilt on the capture stream: no stream-mismatch
    warning (which would mean a cross-stream sync inside the graph)."""
    import warnings
    rng = np.random.default_rng(5)
    B, L = 256, 300
    lab = torch.from_numpy((rng.random((B, L)) < 0.05).astype(np.float32)).to(DEV)
    dists = [{"".join(r.astype(int).astype(str)): float(rng.uniform(0.1, 1))
              for r in lab.cpu().numpy()[i::3]} for i in range(2)]
    tables = [mf.LabelDistanceTable(d, L, DEV) for d in dists]
    sens = torch.from_numpy(rng.integers(0, 3, (B, 2))).to(DEV)
    lz = torch.from_numpy(rng.uniform(0.01, 0.99, (B, L)).astype(np.float32)).to(DEV)
    fz = torch.from_numpy(rng.uniform(0.01, 0.99, (B, L)).astype(np.float32)).to(DEV)

    def eager(lz_v, fz_v, sens_v, mg=None):
        a, b = lz_v.clone().requires_grad_(True), fz_v.clone().requires_grad_(True)
        loss, cnt = mf.fairness_penalty(a, b, lab, sens_v, tables, "l2", 0.7, max_groups=mg)
        loss.backward()
        return loss.detach(), cnt, a.grad, b.grad

    a = lz.clone().requires_grad_(True)
    b = fz.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            a.grad = b.grad = None
            loss, cnt = mf.fairness_penalty(a, b, lab, sens, tables, "l2", 0.7)
            loss.backward()
    torch.cuda.current_stream().wait_stream(side)
    a.grad = b.grad = None
    del loss, cnt  # the warm-up's graph holds AccumulateGrad nodes made on `side`
    graph = torch.cuda.CUDAGraph()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.cuda.graph(graph):
            loss, cnt = mf.fairness_penalty(a, b, lab, sens, tables, "l2", 0.7)
            loss.backward()
    bad = [str(w.message)[:80] for w in caught if "AccumulateGrad" in str(w.message)]
    assert not bad, bad
    for it in range(3):
        new_l = torch.from_numpy(rng.uniform(0.01, 0.99, (B, L)).astype(np.float32)).to(DEV)
        new_s = torch.from_numpy(rng.integers(0, 2 + it, (B, 2))).to(DEV)
        with torch.no_grad():
            a.copy_(new_l)
            sens.copy_(new_s)
        graph.replay()
        torch.cuda.synchronize()
        ref = eager(new_l, fz, new_s)
        assert torch.equal(loss, ref[0]) and int(cnt) == int(ref[1])
        assert torch.equal(a.grad, ref[2]) and torch.equal(b.grad, ref[3])
        bounded = eager(new_l, fz, new_s, mg=16)
        assert abs(float(bounded[0]) - float(ref[0])) <= 1e-12 * abs(float(ref[0]))
    # more distinct patterns than the bound: NaN, not an out-of-bounds read
    assert torch.isnan(eager(lz, fz, sens, mg=2)[0])
