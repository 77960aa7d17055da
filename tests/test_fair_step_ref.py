"""CPU: the references of the fused fairness path (tests/fair_step_ref.py)
against numpy's own unique and against the vectors recorded from the
reference, and the host-side argument checks of the two ABI 15 entry points."""
import ctypes

import numpy as np
import pytest
import torch

import mpvae_hip as H
from fair_io import fair_fixtures
from fair_step_ref import groups_ref, penalty_ref

FAIR = fair_fixtures()


def _rows(kind, B, n, rng):
    """Rows with repeats; the float kind mixes -0.0 and +0.0 in equal rows."""
    if kind == "int64":
        return rng.integers(-2, 2, (B, n)).astype(np.int64)
    x = rng.integers(-1, 2, (B, n)).astype(np.float64) * 0.5
    x[rng.random((B, n)) < 0.5] *= -1.0  # 0.0 -> -0.0 at random places
    return x


@pytest.mark.parametrize("kind", ["int64", "float64"])
@pytest.mark.parametrize("B,n", [(1, 1), (7, 1), (40, 2), (65, 3)])
def test_groups_ref_matches_numpy_unique(kind, B, n):
    rng = np.random.default_rng(B * 10 + n)
    x = _rows(kind, B, n, rng)
    if kind == "float64" and B > 1:
        assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    uniq, inv = np.unique(x, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(B)
    gid, order, goff, G, overflow = groups_ref(x)
    assert G == B and not overflow
    assert np.array_equal(gid, inv)
    assert np.array_equal(order, np.argsort(inv, kind="stable"))
    assert np.array_equal(goff, np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=B))]))
    # a bound equal to the number of groups changes nothing; one below clamps
    k = len(uniq)
    g2 = groups_ref(x, k)
    assert np.array_equal(g2[0], inv) and not g2[4] and len(g2[2]) == k + 1
    if k > 1:
        g3 = groups_ref(x, k - 1)
        assert g3[4] and np.array_equal(g3[0], np.minimum(inv, k - 2))
        assert g3[2][-1] == B and np.array_equal(np.sort(g3[1]), np.arange(B))


@pytest.mark.parametrize("f", FAIR, ids=[f["name"] for f in FAIR])
def test_penalty_ref_matches_reference(f):
    """The tolerances of tests/test_oracle_fair.py."""
    lz = torch.from_numpy(f["label_z"]).requires_grad_(True)
    fz = torch.from_numpy(f["feat_z"]).requires_grad_(True)
    loss, contributed = penalty_ref(lz, fz, f["labels"], torch.from_numpy(f["sensitive"]),
                                    f["dists"], f["norm"], f["coeff"])
    assert contributed == int(f["contributed"])
    if not int(f["active"]):
        assert isinstance(loss, float) and loss == 0.0
        return
    ltol, gtol = (1e-7, 1e-6) if f["pyfloat"] else (1e-12, 1e-6)
    assert str(loss.dtype) == "torch." + str(f["ref_dtype"])
    loss.backward()
    assert abs(float(loss.detach()) - float(f["fairloss"])) <= ltol * abs(float(f["fairloss"]))
    for g, ref in ((lz.grad.numpy(), f["g_label_z"]), (fz.grad.numpy(), f["g_feat_z"])):
        assert np.abs(g - ref).max() <= gtol * np.abs(ref).max()


def test_group_rows_host_checks():
    """mpv_group_rows states its range (include/mpvae_hip.h) and rejects
    anything outside it on the host, before any launch."""
    lib = H.load_library()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails its checks
    call = lambda B, n, G, elem=H.EL_I64, x=fake: lib.mpv_group_rows(x, elem, B, n, G, fake, fake,
                                                                     fake, fake, None)
    assert call(4, 2, 4, x=None) == H.EINVAL and b"NULL" in lib.mpv_last_error()
    for B, n, G in ((0, 2, 1), (H.GROUP_MAX_B + 1, 2, 4), (8, 0, 4), (8, H.GROUP_MAX_N + 1, 4),
                    (8, 2, 0), (8, 2, H.GROUP_MAX_B + 1)):
        assert call(B, n, G) == H.EINVAL, (B, n, G)
        assert b"supports" in lib.mpv_last_error()
    assert call(8, 2, 4, elem=7) == H.EINVAL and b"element type" in lib.mpv_last_error()
    assert (H.GROUP_MAX_B, H.GROUP_MAX_N) == (4096, 64)


def test_label_weights_batch_host_checks():
    lib = H.load_library()
    fake = ctypes.c_void_p(0x1000)
    L = 70
    good = H.LabelTable(fake, fake, fake, 8, 2)
    tabs = (H.LabelTable * 3)(good, H.LabelTable(None, None, None, 0, 2),
                              H.LabelTable(fake, fake, fake, 8, 1))  # W != ceil(L / 64)
    assert lib.mpv_label_weights_batch(fake, 4, L, tabs, 3, fake, fake, None) == H.EINVAL
    assert b"ceil(L/64)" in lib.mpv_last_error()
    assert lib.mpv_label_weights_batch(fake, 4, L, tabs, 0, fake, fake, None) == H.EINVAL
    assert lib.mpv_label_weights_batch(fake, 0, L, tabs, 2, fake, fake, None) == H.EINVAL
    tabs[2] = H.LabelTable(fake, fake, fake, 6, 2)  # not a power of two
    assert lib.mpv_label_weights_batch(fake, 4, L, tabs, 3, fake, fake, None) == H.EINVAL
    assert b"power of two" in lib.mpv_last_error()
    assert H.LABEL_TABLES_PER_LAUNCH >= 8
