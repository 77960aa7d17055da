"""ctypes binding of libmpvae_hip.so (C ABI: include/mpvae_hip.h).

The struct layouts, the signatures and the constants are read from the header
at import (cabi.py), so there is no second copy of the ABI to keep in step.

The library is loaded from this directory, after ``import torch`` so that the
HIP runtime torch already loaded is the one the kernels register with (both
share the SONAME libamdhip64.so.7).  There is deliberately no fallback: if the
library is missing or the device is not a GPU, every entry point raises.
"""
import ctypes
import os

import torch  # noqa: F401  (must precede the .so load: one HIP runtime per process)

import cabi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPVAE_HIP_LIB", os.path.join(HERE, "libmpvae_hip.so"))
INCLUDE = os.path.join(HERE, os.pardir, "include")


class MPVError(RuntimeError):
    """An MPV_E* status returned by libmpvae_hip.so."""


def read_header(name, known=None):
    """cabi.parse of include/<name>, the directory beside the package."""
    path = os.path.join(INCLUDE, name)
    if not os.path.exists(path):
        raise MPVError(f"{name} not found at {path}: the binding takes its struct layouts, "
                       "signatures and constants from include/ beside the package")
    return cabi.parse(path, known)


_header = read_header("mpvae_hip.h")
STRUCTS = _header.structs  # C name -> ctypes.Structure, fields as the header declares them
SIGNATURES = _header.prototypes  # name -> (restype, argtypes); exactly the header's symbols
# MPV_X of the header is X here: ABI_VERSION, EINVAL, F32, G_TOTAL, GEMM_F16X3, EL_U8, ...
globals().update({k[4:]: v for k, v in _header.constants.items() if k.startswith("MPV_")})

Shape = STRUCTS["mpv_shape"]
Split16 = STRUCTS["mpv_split16"]
FwdArgs = STRUCTS["mpv_fwd_args"]
PredictArgs = STRUCTS["mpv_predict_args"]
FinalArgs = STRUCTS["mpv_final_args"]
BwdArgs = STRUCTS["mpv_bwd_args"]
KlBwdArgs = STRUCTS["mpv_kl_bwd_args"]
ReparamArgs = STRUCTS["mpv_reparam_args"]
ReparamBwdArgs = STRUCTS["mpv_reparam_bwd_args"]
LabelTable = STRUCTS["mpv_label_table"]
LabelSim = STRUCTS["mpv_label_sim"]
LinearArgs = STRUCTS["mpv_linear_args"]
AdamTensor = STRUCTS["mpv_adam_tensor"]
AdamArgs = STRUCTS["mpv_adam_args"]
AdamFinishArgs = STRUCTS["mpv_adam_finish_args"]
FairArgs = STRUCTS["mpv_fair_args"]
CurveArgs = STRUCTS["mpv_curve_args"]
SweepArgs = STRUCTS["mpv_sweep_args"]
CalibArgs = STRUCTS["mpv_calib_args"]
SplitEvalArgs = STRUCTS["mpv_split_eval_args"]
GatherArgs = STRUCTS["mpv_gather_args"]

_lib = None


def load_library(path=None):
    """Load (once) and type the C ABI.  Raises if the library is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise MPVError(f"libmpvae_hip.so not found at {p}: run `make -C mpvae-1_amd` "
                       "(or __graft_entry__.build()); there is no CPU fallback")
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if lib.mpv_abi_version() != ABI_VERSION:
        raise MPVError(f"ABI mismatch: library {lib.mpv_abi_version()} != {ABI_VERSION}")
    if path is None:
        _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load_library().mpv_last_error().decode(errors="replace")
        raise MPVError(f"{what} failed (status {rc}): {msg}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_of(device):
    """The current HIP stream of `device` (the capturing stream inside
    torch.cuda.graph).  The raw-handle query costs ~0.3 us where building a
    torch.cuda.Stream object costs ~6 (several per compute_loss call)."""
    d = device if isinstance(device, torch.device) else torch.device(device)
    idx = d.index if d.index is not None else torch.cuda.current_device()
    if _raw_stream is None:  # a torch without the private query: the public object
        return ctypes.c_void_p(torch.cuda.current_stream(idx).cuda_stream)
    return ctypes.c_void_p(_raw_stream(idx))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def require_gpu(*tensors):
    """The product path runs only on the GPU; CPU tensors are an error, not a fallback."""
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("mpvae-1_amd runs the probit-ELBO hot path on the GPU only "
                               f"(got a {t.device} tensor); move inputs to a ROCm device")
    load_library()


KERNELS = ["noise_philox", "split", "probit_fwd", "fwd_combine", "finalize", "bwd_coef", "bwd_elem",
           "dR_gemm", "sum_slabs", "convert", "bstat_combine", "reparam_fwd", "reparam_bwd",
           "kl_bwd", "label_weights", "label_sim", "group_rows", "fair_fwd", "fair_bwd", "metrics", "linear", "adam",
           "adam_finish", "curve_keys", "curve_sort", "curve_merge", "curve_pass", "curve_agg",
           "metric_sweep", "calib_fwd", "calib_tables", "calib_bwd", "probit_predict",
           "predict_final", "split_eval", "split_final", "gather_batch", "philox_raw",
           "r_uniform"]


def kernel_times():
    """{kernel: (launches, total_ms)} recorded since the last mpv_timing_reset()."""
    lib = load_library()
    out = {}
    for k in KERNELS:
        n, ms = ctypes.c_int64(), ctypes.c_double()
        check(lib.mpv_timing_query(k.encode(), ctypes.byref(n), ctypes.byref(ms)), "timing_query")
        if n.value:
            out[k] = (n.value, ms.value)
    return out
