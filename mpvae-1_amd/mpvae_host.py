"""The probit-ELBO hot path for CPU tensors: libmpvae_host.so (include/mpvae_host.h).

The reference runs its small configuration on the CPU (BASELINE configs[0],
script/run_train_mirflickr.sh; fairsoft_trial.py:157-158 picks the CPU when
CUDA is absent).  ``compute_loss`` dispatches on the tensors' device: CPU
tensors run here, in host C++ with OpenMP (the same algorithm as the HIP
kernels: factorised ranking loss, exact log-sum-exp, analytic backward; E in
fp32 in the reference's op order, fp64 after).  This is a backend for CPU
tensors, not a fallback: CUDA tensors always run the HIP library and raise
when it is missing.

``HostShardBackend`` is a ``mpvae_ops.ShardBackend`` (the per-shard interface,
declared there), so ``ProbitELBO``, ``probit_predict`` and the sample-sharded
exchange (mpvae_dist.py, gloo on CPU) drive it as they drive the GPU's.
"""
import ctypes
import os

import torch

import mpvae_hip as H
from mpvae_ops import ShardBackend, stat_buffers

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPVAE_HOST_LIB", os.path.join(HERE, "libmpvae_host.so"))
F32, F64 = torch.float32, torch.float64

_header = H.read_header("mpvae_host.h", {"mpv_shape": H.Shape})
STRUCTS, _SIGS = _header.structs, _header.prototypes
EXPORTS = sorted(_SIGS)
ABI_VERSION = _header.constants["MPVH_ABI_VERSION"]
FwdArgs = STRUCTS["mpvh_fwd_args"]
FinalArgs = STRUCTS["mpvh_final_args"]
BwdArgs = STRUCTS["mpvh_bwd_args"]

_lib = None


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise H.MPVError(f"libmpvae_host.so not found at {LIB_PATH}: run `make -C mpvae-1_amd`")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
        if lib.mpvh_abi_version() != ABI_VERSION:
            raise H.MPVError(f"host ABI mismatch: library {lib.mpvh_abi_version()} != {ABI_VERSION}")
        _lib = lib
    return _lib


def _check(rc, what):
    if rc != 0:
        raise H.MPVError(f"{what} failed ({rc}): {load_library().mpvh_last_error().decode()}")


def _c(t, dtype):
    if t.dtype != dtype:
        raise TypeError(f"expected {dtype}, got {t.dtype}")
    return t.detach().contiguous()


class HostShardBackend(ShardBackend):
    """Per-shard arithmetic on the CPU through libmpvae_host.so (statistics in
    fp64)."""

    def make_noise(self, shape, device, seed, offset):
        raise ValueError("args.mpvae_noise = 'philox' draws on the GPU; CPU tensors take the "
                         "reference's torch_cpu draw or an explicit noise tensor")

    def prepare_noise(self, eps, shape):
        return _c(eps, F32)

    def prepare_R(self, R):
        if R.dtype not in (F32, F64):
            raise TypeError(f"r_sqrt_sigma must be float32 or float64 (got {R.dtype})")
        return R.detach().contiguous()

    def forward_local(self, shape, y, fe_out, fx_out, Rop, eps, keep_T, stat_slots=None):
        S, B, L = shape.S_local, shape.B, shape.L
        T = torch.empty((S, B, L), dtype=F32) if keep_T else None
        rowstat = torch.empty((6, B, S), dtype=F64)
        packed, colsum, bstat = stat_buffers(B, L, stat_slots,
                                             lambda n: torch.empty(n, dtype=F64))
        y, fe_out, fx_out = (_c(t, F32) for t in (y, fe_out, fx_out))
        a = FwdArgs(H.ptr(y), H.ptr(fe_out), H.ptr(fx_out), H.ptr(Rop), H.F64 if Rop.dtype == F64 else H.F32,
                    H.ptr(eps), H.ptr(T), H.ptr(rowstat), H.ptr(bstat), H.ptr(colsum))
        _check(load_library().mpvh_probit_fwd(shape, a), "mpvh_probit_fwd")
        return dict(rowstat=rowstat, bstat=bstat, colsum=colsum, T=T, packed=packed)

    def predict_local(self, shape, fx_out, Rop, eps, want_indiv=True, seed_advance=None):
        """mpvh_probit_predict: (this shard's (B, L) fp64 sum over s of E_x,
        indiv_prob or None), the feature-branch half of forward_local."""
        if seed_advance is not None:
            raise ValueError("args.mpvae_seed_advance is a device-key option (philox on the GPU)")
        colsum = torch.empty((shape.B, shape.L), dtype=F64)
        fx_out = _c(fx_out, F32)
        _check(load_library().mpvh_probit_predict(shape, H.ptr(fx_out), H.ptr(Rop),
                                                  H.F64 if Rop.dtype == F64 else H.F32, H.ptr(eps),
                                                  H.ptr(colsum)), "mpvh_probit_predict")
        return colsum, (self.indiv_from_colsum(colsum, shape.S_total) if want_indiv else None)

    @staticmethod
    def indiv_from_colsum(colsum, S_total):
        """mpvh_probit_finalize's indiv_prob: the fp64 quotient rounded to fp32."""
        return (colsum / float(S_total)).to(F32)

    def combine_bstats(self, gathered):
        g = gathered.to(F64).contiguous()
        out = torch.empty(g.shape[1:], dtype=F64)
        _check(load_library().mpvh_bstat_combine(H.ptr(g), g.shape[0], g.shape[2], H.ptr(out)),
               "mpvh_bstat_combine")
        return out

    def finalize(self, shape, bstat, colsum, fe_mu, fe_logvar, fx_mu, fx_logvar, nll_coeff,
                 c_coeff, seed_advance=None):
        if seed_advance is not None:
            raise ValueError("args.mpvae_seed_advance is a device-key option (philox on the GPU)")
        B, L = shape.B, shape.L
        out6 = torch.empty((6,), dtype=F32)
        indiv = torch.empty((B, L), dtype=F32)
        indiv_label = torch.empty((B, L), dtype=F32)
        mus = [_c(t, F32) for t in (fe_mu, fe_logvar, fx_mu, fx_logvar)]
        bstat, colsum = bstat.to(F64).contiguous(), colsum.to(F64).contiguous()
        a = FinalArgs(H.ptr(bstat), H.ptr(colsum), *[H.ptr(t) for t in mus], fe_mu.shape[1], nll_coeff,
                      c_coeff, H.ptr(out6), H.ptr(indiv), H.ptr(indiv_label))
        _check(load_library().mpvh_probit_finalize(shape, a), "mpvh_probit_finalize")
        return (*[out6[i] for i in range(6)], indiv, indiv_label)

    def backward_local(self, shape, saved, gscal, live, g_I, g_IL, nll_coeff, c_coeff, want_dR,
                       dR_dtype=F32, kl=False):
        B, L, z = shape.B, shape.L, shape.z
        d2 = torch.empty((2, B, L), dtype=F64)
        dR64 = torch.empty((L, z), dtype=F64) if want_dR else None
        # every tensor the call reads is bound to a name here (alive through the call)
        gscal = _c(gscal.reshape(-1).to(F32), F32)
        rowstat = saved["rowstat"].to(F64).contiguous()
        bstat = saved["bstat"].to(F64).contiguous()
        g_I = None if g_I is None else _c(g_I, F32)
        g_IL = None if g_IL is None else _c(g_IL, F32)
        a = BwdArgs(H.ptr(saved["y"]), H.ptr(saved["fe_out"]), H.ptr(saved["fx_out"]), H.ptr(saved["eps"]),
                    H.ptr(saved["T"]), H.ptr(rowstat), H.ptr(bstat), H.ptr(gscal), int(live), H.ptr(g_I),
                    H.ptr(g_IL), nll_coeff, c_coeff, H.ptr(d2), H.ptr(dR64))
        _check(load_library().mpvh_probit_bwd(shape, a), "mpvh_probit_bwd")
        n = 2 * B * L
        local64 = dR_dtype == F64 and want_dR
        flat = torch.empty((n + (L * z if want_dR and not local64 else 0),), dtype=F32)
        flat[:n] = d2.reshape(-1)
        dR = None
        if want_dR:
            if local64:
                dR = dR64
            else:
                flat[n:] = dR64.reshape(-1)
                dR = flat[n:].view(L, z)
        out = (flat, flat[:n].view(2, B, L), dR)
        if kl:
            out = (*out, self.kl_backward(saved["fe_mu"], saved["fe_logvar"], saved["fx_mu"],
                                          saved["fx_logvar"], gscal, live))
        return out

    def kl_backward(self, fe_mu, fe_logvar, fx_mu, fx_logvar, gscal, live=0x3F):
        mus = [_c(t, F32) for t in (fe_mu, fe_logvar, fx_mu, fx_logvar)]
        B, d = fe_mu.shape
        outs = [torch.empty((B, d), dtype=F32) for _ in range(4)]  # g_fe_mu, g_fe_logvar, ...
        g = _c(gscal.reshape(-1).to(F32), F32)
        _check(load_library().mpvh_kl_bwd(*[H.ptr(t) for t in mus], B, d, H.ptr(g), int(live),
                                          H.ptr(outs[0]), H.ptr(outs[1]), H.ptr(outs[2]), H.ptr(outs[3])),
               "mpvh_kl_bwd")
        return outs
