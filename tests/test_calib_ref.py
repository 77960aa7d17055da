"""CPU: the calibration restatement (tests/calib_ref.py) against the golden
records of the reference (tests/golden/make_golden_calib.py), ``centroid_ids``
on CPU tensors, and the host-side argument checks of mpv_calib_*."""
import ctypes

import numpy as np
import pytest
import torch

import calib_ref as cr
import mpvae_fair as mf
import mpvae_hip as H
from calib_io import calib_fixtures, gap
from tolerances import rel_err

CAL = calib_fixtures()
F32_ROUND = 2.0 ** -23  # one rounding of a value to the fp32 the record holds


def _runs(f):
    """The restatement's total-loss run (active cases) and its BCE-only run."""
    a = (f["p"], f["threshold"], f["labels"], f["sensitive"], f["centroids"], f["dists"],
         f["learn_logit"])
    return cr.run64(*a, g_bce=1.0, g_fair=f["fair_coeff"]), cr.run64(*a, g_bce=1.0, g_fair=0.0)


def _pairs(f):
    """(name of the record, the restatement's value) for everything recorded."""
    tot, bce = _runs(f)
    out = [("bce", tot["bce"]), ("fair", tot["fair"]), ("cal_prob", tot["cal_prob"]),
           ("g_bce_threshold", bce["g_threshold"]), ("g_bce_p", bce["g_p"])]
    if f["active"]:
        out += [("total", tot["fair"] * f["fair_coeff"] + tot["bce"]),
                ("g_threshold", tot["g_threshold"]), ("g_p", tot["g_p"])]
    return tot, out


def test_the_cases_the_issue_lists_are_recorded():
    names = {f["name"] for f in CAL}
    assert {"c1_logit", "c2_prob_pyfloat", "c3_zero_weight_group", "c4_dead_target", "c5_inactive",
            "c6_one_group", "c7_l257", "c8_edge"} <= names
    by = {f["name"]: f for f in CAL}
    assert by["c1_logit"]["learn_logit"] and not by["c2_prob_pyfloat"]["learn_logit"]
    assert by["c2_prob_pyfloat"]["pyfloat"] and not by["c1_logit"]["pyfloat"]
    assert not by["c5_inactive"]["active"] and np.isnan(by["c5_inactive"]["eval_mean_diff"])
    assert len(by["c6_one_group"]["centroids"]) == 1 and by["c7_l257"]["p"].shape[1] == 257
    p = by["c8_edge"]["p"].astype(np.float64)
    assert (np.minimum(np.abs(p - 5e-7), np.abs(p - (1 - 5e-7))) <= 1e-4 + 1e-7).all()
    # a group with rows but no weight; a target whose dict misses the batch
    f = by["c3_zero_weight_group"]
    w, gid = cr.weights(f["labels"], f["dists"]), cr.group_of(f["sensitive"], f["centroids"])
    assert (gid == 0).any() and (w[:, gid == 0] == 0).all() and (w.sum(1) > 0).all()
    assert (cr.weights(by["c4_dead_target"]["labels"], by["c4_dead_target"]["dists"]).sum(1)
            == 0).tolist() == [False, True, False]


@pytest.mark.parametrize("f", CAL, ids=[f["name"] for f in CAL])
def test_restatement_matches_the_fp64_records(f):
    tot, pairs = _pairs(f)
    assert (tot["nterms"] > 0) == f["active"]
    for k, v in pairs:
        assert rel_err(v, f[k + "_64"]) <= 1e-12, k


@pytest.mark.parametrize("f", CAL, ids=[f["name"] for f in CAL])
def test_restatement_within_the_references_fp32_error(f):
    """Against the fp32 records -- the reference as it is -- the restatement
    sits within the reference's own recorded fp32-vs-fp64 gap plus the
    rounding of the recorded fp32 value."""
    _, pairs = _pairs(f)
    for k, v in pairs:
        ref = np.asarray(f[k], np.float64)
        tol = gap(f, k) + F32_ROUND * np.abs(ref).max()
        assert np.abs(np.asarray(v) - ref).max() <= tol, k


@pytest.mark.parametrize("f", CAL, ids=[f["name"] for f in CAL])
def test_mean_diff_restatement_matches_the_evaluation_block(f):
    got = cr.mean_diff(f["eval_cal_prob"], f["labels"], f["sensitive"], f["centroids"], f["dists"])
    ref = float(f["eval_mean_diff"])
    if np.isnan(ref):
        assert np.isnan(got)
    else:
        assert abs(got - ref) <= 1e-12 * abs(ref)


def test_centroid_ids_match_sen_belong_on_cpu():
    rng = np.random.default_rng(0)
    cents = torch.from_numpy(np.unique(rng.integers(0, 3, (40, 2)), axis=0))
    sens = cents[torch.from_numpy(rng.integers(0, len(cents), 57))]
    # fairsoft_train_postprocess.py:114-115
    sen_belong = torch.all(torch.eq(sens.unsqueeze(1), cents), dim=2)
    gid, unmatched = mf.centroid_ids(sens, cents)
    assert gid.dtype == torch.int32 and gid.shape == (57,) and not bool(unmatched)
    onehot = torch.zeros_like(sen_belong)
    onehot[torch.arange(57), gid.long()] = True
    assert torch.equal(onehot, sen_belong)
    # a row that is no centroid: flagged, id clamped to 0
    sens[5] = torch.tensor([7, 7])
    gid2, unmatched2 = mf.centroid_ids(sens, cents)
    assert bool(unmatched2) and int(gid2[5]) == 0
    assert torch.equal(gid2[torch.arange(57) != 5], gid[torch.arange(57) != 5])
    with pytest.raises(ValueError):
        mf.centroid_ids(sens, cents[:0])


def test_calib_host_checks():
    """mpv_calib_*'s workspace sizing and argument checks run on the host and
    reject bad calls before any launch (csrc/calib.hip)."""
    lib = H.load_library()
    assert lib.mpv_calib_workspace_bytes(0, 1, 2, 1) == 0
    assert lib.mpv_calib_workspace_bytes(38, -1, 2, 1) == 0
    assert lib.mpv_calib_workspace_bytes(38, 1, 0, 1) == 0
    assert lib.mpv_calib_workspace_bytes(38, 1, 2, 0) == 0
    need = lib.mpv_calib_workspace_bytes(38, 1, 4, 8)
    assert need > lib.mpv_calib_workspace_bytes(38, 0, 4, 8) > 0  # T = 0 is valid
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its checks

    def args(**kw):
        base = dict(p=fake, threshold=fake, y=fake, w=fake, order=fake, goff=fake, B=8, L=38, T=1,
                    G=4, R=8, learn_logit=1, cal_prob=fake, out=fake)
        base.update(kw)
        return H.CalibArgs(**base)

    def fwd(a, ws=fake, n=need):
        return lib.mpv_calib_fwd(ctypes.byref(a), ws, n, None)

    assert fwd(args(p=None)) == 1 and b"NULL p" in lib.mpv_last_error()
    for k in ("B", "L", "G"):
        assert fwd(args(**{k: 0})) == 1 and b"shape" in lib.mpv_last_error(), k
    assert fwd(args(T=-1)) == 1
    assert fwd(args(R=0)) == 1 and b"R must be" in lib.mpv_last_error()
    assert fwd(args(order=None)) == 1 and fwd(args(goff=None)) == 1
    assert fwd(args(w=None)) == 1 and b"NULL w" in lib.mpv_last_error()
    assert fwd(args(out=None)) == 1
    assert fwd(args(), n=need - 1) == 1 and b"workspace" in lib.mpv_last_error()
    assert fwd(args(), ws=None) == 1
    assert lib.mpv_calib_fwd(None, fake, need, None) == 1

    def bwd(a, gout=fake, gx=fake, n=need):
        return lib.mpv_calib_bwd(ctypes.byref(a), gout, gx, None, fake, n, None)

    assert bwd(args(p=None)) == 1
    assert bwd(args(threshold=None)) == 1 and b"threshold" in lib.mpv_last_error()
    assert bwd(args(), gout=None) == 1 and bwd(args(), gx=None) == 1
    assert bwd(args(), n=need - 1) == 1 and b"workspace" in lib.mpv_last_error()
    assert bwd(args(R=0)) == 1
