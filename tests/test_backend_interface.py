"""The interface ProbitELBO and probit_predict drive, as declared in
mpvae_ops.ShardBackend and mpvae_ops.LocalExchange: every backend and both
exchanges keep to it, and a backend that lacks a method fails loudly.  CPU
only; no library is loaded (the classes are imported, the oracle computes)."""
import inspect

import pytest
import torch

from mpvae_dist import SampleShardExchange
from mpvae_host import HostShardBackend
from mpvae_ops import (ElboConfig, HipShardBackend, LocalExchange, ProbitELBO, ShardBackend,
                       probit_predict)
from oracle_backend import OracleShardBackend

# what ShardBackend itself implements; a backend must define every other method
DEFAULTED = {"shape", "make_noise_and_R", "from_f32", "finalize_slots"}
# the oracle backend is never asked to predict (test_predict_host.py drives the
# host backend): it leaves the two prediction calls undefined
UNDEFINED = {OracleShardBackend: {"predict_local", "indiv_from_colsum"}}
BACKENDS = [HipShardBackend, HostShardBackend, OracleShardBackend]


def _public(cls):
    return {n for n, v in vars(cls).items()
            if not n.startswith("_") and isinstance(v, (staticmethod, type(_public)))}


def _params(cls, name):
    return [p for p in inspect.signature(getattr(cls, name)).parameters.values()
            if p.name != "self"]


@pytest.mark.parametrize("cls", BACKENDS, ids=lambda c: c.__name__)
def test_backend_signatures_match_the_base(cls):
    assert issubclass(cls, ShardBackend)
    declared = _public(ShardBackend)
    assert DEFAULTED < declared
    for name in sorted(declared):
        defined = any(name in vars(c) for c in cls.__mro__ if c not in (ShardBackend, object))
        if name not in DEFAULTED and name not in UNDEFINED.get(cls, ()):
            assert defined, f"{cls.__name__} does not define {name}"
        base, sub = _params(ShardBackend, name), _params(cls, name)
        assert [(p.name, p.default, p.kind) for p in sub[:len(base)]] == \
            [(p.name, p.default, p.kind) for p in base], (cls.__name__, name)
        for p in sub[len(base):]:  # extras: callable exactly as the base is
            assert p.default is not p.empty or p.kind is p.KEYWORD_ONLY, (cls.__name__, name, p)


def _inputs(B=3, L=5, z=4, d=2, S=2):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    y = (r(B, L) > 0).float()
    return (y, r(B, L), r(B, d), r(B, d), r(B, L), r(B, d), r(B, d), r(L, z).double()), r(S, B, z)


@pytest.mark.parametrize("noise", ["explicit", "philox"])
def test_backend_without_methods_fails_loudly(noise):
    """Nothing defined: NotImplementedError from the driver's first call into
    the backend's own arithmetic, not an AttributeError further on."""
    class Bare(ShardBackend):
        pass

    t, eps = _inputs()
    cfg = ElboConfig(2, 2, 0, 1.0, 1.0, noise=noise, backend=Bare())
    with pytest.raises(NotImplementedError):
        ProbitELBO.apply(*t, eps, cfg)
    with pytest.raises(NotImplementedError):
        probit_predict(t[4], t[7], eps, cfg)


def test_exchanges_expose_the_same_methods():
    assert _public(LocalExchange) == _public(SampleShardExchange)
    for name in sorted(_public(LocalExchange)):
        assert [p.name for p in _params(LocalExchange, name)] == \
            [p.name for p in _params(SampleShardExchange, name)], name
    assert LocalExchange.local is True and SampleShardExchange.local is False


class _Recording(OracleShardBackend):
    def backward_local(self, *a, **kw):
        self.call = (a, kw)
        return super().backward_local(*a, **kw)


def test_one_element_gscal_equals_the_six_slot_stack():
    """total.backward() alone: the driver hands the backend the upstream
    gradient as a one-element gscal (live == 1).  The oracle backend expands
    it; the gradients are, bit for bit, those of the six-slot stack [g, 0, 0,
    0, 0, 0] passed through backward_local by hand."""
    from golden_io import fixtures
    f = next(f for f in fixtures() if f.name == "f1_l38")
    keys = ["y", "fe_out", "fe_mu", "fe_logvar", "fx_out", "fx_mu", "fx_logvar", "r_sqrt_sigma"]
    t = {k: torch.from_numpy(f[k].copy()).requires_grad_(k != "y") for k in keys}
    be = _Recording()
    cfg = ElboConfig(f.S, f.S, 0, f.nll_coeff, f.c_coeff, backend=be, exchange=LocalExchange())
    out = ProbitELBO.apply(*(t[k] for k in keys), torch.from_numpy(f["noise"].copy()), cfg)
    out[0].backward()
    (shape, saved, gscal, live, *rest), kw = be.call
    assert gscal.numel() == 1 and live == 1 and kw["kl"]
    six = torch.cat([gscal, torch.zeros(5)])
    _, dfe_dfx, dR, gk = OracleShardBackend().backward_local(shape, saved, six, live, *rest, **kw)
    want = dict(fe_out=dfe_dfx[0], fx_out=dfe_dfx[1], r_sqrt_sigma=dR, fe_mu=gk[0],
                fe_logvar=gk[1], fx_mu=gk[2], fx_logvar=gk[3])
    for k, w in want.items():
        got = t[k].grad
        assert got.dtype == w.dtype and got.shape == w.shape, k
        assert torch.equal(got.contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)), k
        assert bool(got.ne(0).any()), k
