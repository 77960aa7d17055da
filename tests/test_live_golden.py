"""Which outputs of compute_loss send a gradient where (tests/golden/live_l20.npz,
recorded from the reference by tests/golden/make_golden_live.py): the oracle
and the host C++ backend against the record, one output at a time and in
branch-crossed subsets.  The HIP kernels meet the same record in
tests/test_gpu_bwd_lattice.py."""
from golden_io import OUTS
from live_io import KEYS, LiveFixture, check_live, compute_loss_runner
from oracle import probit_elbo as pe
from tolerances import FWD_RTOL, rel_err

FIX = LiveFixture()


def test_oracle_live_subsets_match_reference():
    """oracle.probit_elbo.elbo_backward; measured <= 9.3e-7."""
    f = FIX
    inp = [f[k] for k in KEYS]
    fwd = pe.elbo_forward(*inp, f["r_sqrt_sigma"], f["noise"], f.nll_coeff, f.c_coeff, shards=2)
    for k in OUTS:
        assert rel_err(fwd[k], f["out_" + k]) <= FWD_RTOL, k

    def run(obj):
        up = f.weights(obj)
        if "indiv_prob" in obj:
            up["g_I"] = f["g_I"]
        if "indiv_prob_label" in obj:
            up["g_IL"] = f["g_IL"]
        return pe.elbo_backward(fwd, *inp, f["noise"], f.nll_coeff, f.c_coeff, **up)

    check_live(f, run)


def test_host_backend_live_subsets_match_reference():
    """libmpvae_host.so through compute_loss on CPU tensors."""
    check_live(FIX, compute_loss_runner(FIX, "cpu"))
