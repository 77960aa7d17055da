"""Autograd Functions over the HIP kernels of libmpvae_hip.so.

``ProbitELBO`` is the whole of reference ``compute_loss`` (mpvae.py:145-210) as
one custom Function: its forward launches noise (optional) -> fused GEMM +
probit decode + row statistics -> combine -> finalize, and its backward the
analytic gradient kernels.  Sharding of the
Monte-Carlo axis across ranks plugs in through ``exchange`` (``LocalExchange``
here, ``mpvae_dist.SampleShardExchange``: the same methods on both); the
per-shard arithmetic through ``backend``, a ``ShardBackend`` (the interface,
declared once below): ``HipShardBackend`` here for CUDA tensors,
``mpvae_host.HostShardBackend`` for CPU tensors, an oracle one in the tests.

``FusedReparam`` is the reparameterisation of both encoders in one launch
(mpvae.py:66-74).
"""
import ctypes

import torch

import mpvae_hip as H


def _f32(t, name):
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    return t.contiguous()


def _pad(n, m):
    return (n + m - 1) // m * m


class Planes:
    """3xf16 split operand (include/mpvae_hip.h mpv_split16) of `cols` padded
    columns: value = (hi + lo) / scale, stored chunked -- every 32-column chunk
    of a row is 32 hi halves then 32 lo halves (row length ld = 2 * cols)."""

    def __init__(self, rows_pad, cols, device):
        if cols % 32:
            raise ValueError(f"split planes need a multiple of 32 columns (got {cols})")
        self.rows_pad, self.cols, self.ld = int(rows_pad), int(cols), 2 * int(cols)
        self.data = torch.empty((self.rows_pad, self.ld), dtype=torch.int16, device=device)
        self.scale = torch.empty((1,), dtype=torch.float32, device=device)

    def c(self):
        return H.Split16(self.data.data_ptr(), self.scale.data_ptr(), self.rows_pad, self.ld)

    def halves(self):
        """(hi, lo) as (rows_pad, cols) fp16 views' fp32 values."""
        v = self.data.view(torch.float16).float().view(self.rows_pad, self.cols // 32, 2, 32)
        return v[:, :, 0, :].reshape(self.rows_pad, self.cols), \
            v[:, :, 1, :].reshape(self.rows_pad, self.cols)

    def value(self):
        """fp32 value of the planes (tests / diagnostics)."""
        hi, lo = self.halves()
        return (hi + lo) / self.scale


GEMMS = {"f16x3": H.GEMM_F16X3, "f32": H.GEMM_F32}
DTYPE_TAGS = {torch.float32: H.F32, torch.float64: H.F64}


def eps_cols(shape):
    """Noise plane columns: z padded to whole dR tiles (mpv_noise_plane_cols)."""
    n = H.load_library().mpv_noise_plane_cols(shape)
    if n <= 0:
        raise H.MPVError("mpv_noise_plane_cols: bad shape")
    return int(n)


def stat_buffers(B, L, stat_slots, alloc):
    """(packed, colsum (2, B, L), bstat (6, B)): forward_local's statistics
    buffers from ``alloc(shape)`` (uninitialised storage of the backend's
    dtype).  stat_slots None: two buffers, packed None.  stat_slots = (world,
    slot): views of one packed buffer [colsum (2 B L) | world slots of bstat
    (6 B)], bstat being this shard's slot and the slots zeroed, so that ONE
    all_reduce(SUM) of it both sums colsum and gathers bstat (x + 0 is exact;
    SampleShardExchange.finalize)."""
    if stat_slots is None:
        return None, alloc((2, B, L)), alloc((6, B))
    world, slot = stat_slots
    n, m = 2 * B * L, 6 * B
    packed = alloc((n + world * m,))
    packed[n:].zero_()
    return packed, packed[:n].view(2, B, L), packed[n + slot * m:n + (slot + 1) * m].view(6, B)


class ShardBackend:
    """The per-shard arithmetic ProbitELBO and probit_predict drive: what a
    backend defines, and the defaults of what it may leave out.  A method a
    backend does not define raises NotImplementedError.  Subclasses keep every
    name, parameter order and default (tests/test_backend_interface.py)."""

    def shape(self, S_local, S_total, s_offset, B, L, z):
        """The problem's sizes as the backend's calls take them: samples
        [s_offset, s_offset + S_local) of S_total, batch B, labels L, latent z."""
        return H.Shape(S_local, S_total, s_offset, B, L, z)

    def make_noise(self, shape, device, seed, offset):
        """Philox noise of this shard, as the GEMM operand.  seed: an int, or a
        one-element int64 tensor on `device` read at run time."""
        raise NotImplementedError

    def prepare_noise(self, eps, shape):
        """Explicit contiguous (S_local, B, z) fp32 noise -> the GEMM operand."""
        raise NotImplementedError

    def prepare_R(self, R):
        """r_sqrt_sigma (L, z) fp64 / fp32 -> the GEMM operand (R.T.float(),
        mpvae.py:165); TypeError for another dtype."""
        raise NotImplementedError

    def make_noise_and_R(self, shape, device, seed, offset, R):
        """(make_noise(...), prepare_R(R)); a backend may fuse the two."""
        return self.make_noise(shape, device, seed, offset), self.prepare_R(R)

    def from_f32(self, x32, dtype):
        """A summed fp32 gradient in r_sqrt_sigma's dtype."""
        return x32 if dtype == torch.float32 else x32.to(dtype)

    def forward_local(self, shape, y, fe_out, fx_out, Rop, eps, keep_T, stat_slots=None):
        """This shard's statistics: dict(rowstat (6, B, S_local), bstat (6, B),
        colsum (2, B, L), T (what backward_local needs of the forward, None
        unless keep_T), packed).  stat_slots = exchange.stat_slots(): see
        stat_buffers for bstat, colsum and packed."""
        raise NotImplementedError

    def predict_local(self, shape, fx_out, Rop, eps, want_indiv=True, seed_advance=None):
        """(this shard's (B, L) sum over s of E_x, indiv_prob = that / S_total
        or None).  want_indiv=False for a sharded caller, which divides after
        its all-reduce (indiv_from_colsum).  seed_advance: as finalize's."""
        raise NotImplementedError

    @staticmethod
    def indiv_from_colsum(colsum, S_total):
        """indiv_prob from the all-reduced (B, L) column sums, rounded as
        predict_local rounds its own."""
        raise NotImplementedError

    def combine_bstats(self, gathered):
        """The exact combine of the shards' (world, 6, B) bstat: M = max m_r,
        Z = sum Z_r exp(m_r - M), the ranking sums added."""
        raise NotImplementedError

    def finalize(self, shape, bstat, colsum, fe_mu, fe_logvar, fx_mu, fx_logvar, nll_coeff,
                 c_coeff, seed_advance=None):
        """The 8 outputs from the global statistics.  seed_advance: a device
        Philox key (int64 tensor) this step's noise has read, advanced by 1 in
        the same launch; a backend without device keys raises on one."""
        raise NotImplementedError

    def finalize_slots(self, shape, slots, colsum, fe_mu, fe_logvar, fx_mu, fx_logvar, nll_coeff,
                       c_coeff, seed_advance=None):
        """(the combined (6, B) bstat, the 8 outputs) from the all-reduced
        (world, 6, B) slots of the shards' bstat and the summed colsum."""
        bstat = self.combine_bstats(slots)
        return bstat, self.finalize(shape, bstat, colsum, fe_mu, fe_logvar, fx_mu, fx_logvar,
                                    nll_coeff, c_coeff, seed_advance=seed_advance)

    def backward_local(self, shape, saved, gscal, live, g_I, g_IL, nll_coeff, c_coeff, want_dR,
                       dR_dtype=torch.float32, kl=False):
        """(flat, its (2, B, L) view [d fe_out, d fx_out], dR or None[, the 4
        KL gradients when kl]) of this shard.  flat is the fp32 buffer
        [d fe_out | d fx_out | d r_sqrt_sigma] the exchange sums over the
        ranks, dR its tail -- unless dR_dtype is float64: dR is then a tensor
        of its own, outside flat (no cross-shard sum may follow).  gscal: the
        upstream gradients of the 6 scalars, or one element when live == 1
        (the total's alone); live: bit i set when slot i is.  kl: kl_backward
        on saved's fe_mu ... fx_logvar rides along."""
        raise NotImplementedError

    def kl_backward(self, fe_mu, fe_logvar, fx_mu, fx_logvar, gscal, live=0x3F):
        """[g_fe_mu, g_fe_logvar, g_fx_mu, g_fx_logvar]; gscal, live as
        backward_local's."""
        raise NotImplementedError


class HipShardBackend(ShardBackend):
    """Per-shard arithmetic on the GPU through the C ABI.

    gemm="f16x3" (default): the two noise GEMMs run on the f16 matrix cores
    with 3xf16 split operands (~fp32 accuracy); gemm="f32": exact fp32 MFMA.

    poison=True (tests and tools/repeat_probe.py only): every output and
    workspace buffer of forward_local / backward_local is filled with NaN bytes
    (0xFF) before the launch, so a write the kernels skip or lose shows up as a
    NaN instead of hiding behind the identical bytes the caching allocator
    hands back from an earlier launch."""

    def __init__(self, gemm="f16x3", poison=False):
        if gemm not in GEMMS:
            raise ValueError(f"gemm must be one of {sorted(GEMMS)} (got {gemm!r})")
        self.gemm = GEMMS[gemm]
        self.poison = bool(poison)

    def _buf(self, shape, device, dtype):
        t = torch.empty(shape, device=device, dtype=dtype)
        if self.poison:
            t.view(torch.uint8).fill_(0xFF)  # all-ones words: NaN in fp32 and fp64
        return t

    @staticmethod
    def _check_seed(seed, device):
        if isinstance(seed, torch.Tensor) and (seed.dtype != torch.int64 or seed.numel() != 1 or
                                               seed.device != torch.device(device)):
            raise ValueError("a device Philox seed must be a one-element int64 tensor on "
                             f"{device} (got {seed.dtype}, {seed.numel()} elements, {seed.device})")

    def make_noise(self, shape, device, seed, offset):
        """Philox noise for this shard.  seed: an int (the key, passed by value)
        or a one-element int64 device tensor holding it (read by the kernel at
        run time: graph-capturable, no host sync)."""
        lib, st = H.load_library(), H.stream_of(device)
        dev_key = isinstance(seed, torch.Tensor)
        self._check_seed(seed, device)
        if self.gemm == H.GEMM_F16X3:
            eps = Planes(shape.S_local * shape.B, eps_cols(shape), device)
            if dev_key:
                H.check(lib.mpv_noise_philox_f16_dev(shape, H.ptr(seed), offset, eps.c(), st),
                        "mpv_noise_philox_f16_dev")
            else:
                H.check(lib.mpv_noise_philox_f16(shape, seed, offset, eps.c(), st),
                        "mpv_noise_philox_f16")
            return eps
        eps = torch.empty((shape.S_local, shape.B, shape.z), device=device, dtype=torch.float32)
        if dev_key:
            H.check(lib.mpv_noise_philox_dev(H.ptr(eps), shape, H.ptr(seed), offset, st),
                    "mpv_noise_philox_dev")
        else:
            H.check(lib.mpv_noise_philox(H.ptr(eps), shape, seed, offset, st), "mpv_noise_philox")
        return eps

    # r_sqrt_sigma of at most this many elements is split inside the noise
    # launch (mpv_noise_philox_f16_split; the split_small path)
    SPLIT_WITH_NOISE = 16384

    def make_noise_and_R(self, shape, device, seed, offset, R):
        """(make_noise(...), prepare_R(R)) -- in ONE launch when the noise is
        3xf16 Philox and R is small (L, z <= 128: C2, C3), else two."""
        L, z = R.shape
        if (self.gemm != H.GEMM_F16X3 or L * z > self.SPLIT_WITH_NOISE
                or R.dtype not in (torch.float32, torch.float64)):
            return self.make_noise(shape, device, seed, offset), self.prepare_R(R)
        lib, st = H.load_library(), H.stream_of(device)
        dev_key = isinstance(seed, torch.Tensor)
        self._check_seed(seed, device)
        eps = Planes(shape.S_local * shape.B, eps_cols(shape), device)
        Rc = R.detach().contiguous()
        Rop = Planes(_pad(L, 256), _pad(z, 128), R.device)
        H.check(lib.mpv_noise_philox_f16_split(
            shape, 0 if dev_key else int(seed) & (2 ** 64 - 1), H.ptr(seed) if dev_key else None,
            offset, eps.c(), H.ptr(Rc), DTYPE_TAGS[Rc.dtype], L, z, Rop.c(), st),
            "mpv_noise_philox_f16_split")
        return eps, Rop

    def _split(self, x, rows, cols, planes):
        lib = H.load_library()
        ws = torch.empty((lib.mpv_split_workspace_bytes(),), device=x.device, dtype=torch.uint8)
        H.check(lib.mpv_split_f16(H.ptr(x), DTYPE_TAGS[x.dtype], rows, cols, planes.c(),
                                  H.ptr(ws), H.stream_of(x.device)), "mpv_split_f16")
        return planes

    def prepare_noise(self, eps, shape):
        """Explicit (S_local,B,z) fp32 noise -> the GEMM operand."""
        if self.gemm == H.GEMM_F32:
            return eps
        rows = shape.S_local * shape.B
        # plane rows are b-major (row b*S + s): split the (B, S, z) transpose
        eps_bs = eps.transpose(0, 1).contiguous()
        return self._split(eps_bs, rows, shape.z, Planes(rows, eps_cols(shape), eps.device))

    def prepare_R(self, R):
        """r_sqrt_sigma (L,z) fp64/fp32 -> the GEMM operand (R.T.float(), mpvae.py:165)."""
        if R.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"r_sqrt_sigma must be float32 or float64 (got {R.dtype})")
        if self.gemm == H.GEMM_F32:
            return self.to_f32(R)
        L, z = R.shape
        return self._split(R.detach().contiguous(), L, z,
                           Planes(_pad(L, 256), _pad(z, 128), R.device))

    def to_f32(self, R):
        if R.dtype == torch.float32:
            return R.contiguous()
        if R.dtype != torch.float64:
            raise TypeError(f"r_sqrt_sigma must be float32 or float64 (got {R.dtype})")
        return self._convert(R.contiguous(), torch.float32)

    def from_f32(self, x32, dtype):
        return x32 if dtype == torch.float32 else self._convert(x32, dtype)

    @staticmethod
    def _convert(x, dtype):
        """Contiguous fp32 / fp64 x as a new tensor of dtype (mpv_convert)."""
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
        H.check(H.load_library().mpv_convert(H.ptr(x), DTYPE_TAGS[x.dtype], H.ptr(out),
                                             DTYPE_TAGS[dtype], x.numel(),
                                             H.stream_of(x.device)), "mpv_convert")
        return out

    def _eps_operands(self, eps):
        """The (eps, eps16) slots of the kernels' argument structs: the 3xf16
        noise planes or the fp32 pointer, the other mode's slot empty."""
        if self.gemm == H.GEMM_F16X3:
            return None, eps.c()
        return H.ptr(eps), H.Split16()

    def _gemm_operands(self, Rop, eps):
        """The (R32, eps, R16, eps16) slots: r_sqrt_sigma beside _eps_operands."""
        eps32, eps16 = self._eps_operands(eps)
        if self.gemm == H.GEMM_F16X3:
            return None, eps32, Rop.c(), eps16
        return H.ptr(Rop), eps32, H.Split16(), eps16

    def forward_local(self, shape, y, fe_out, fx_out, Rop, eps, keep_T, stat_slots=None):
        lib = H.load_library()
        dev = y.device
        S, B, L = shape.S_local, shape.B, shape.L
        # rows padded to 4 floats (ABI v5: 16-B aligned rows for the element pass)
        f32 = torch.float32
        T = self._buf((B, S, (L + 3) // 4 * 4), dev, f32) if keep_T else None
        rowstat = self._buf((6, B, S), dev, f32)
        packed, colsum, bstat = stat_buffers(B, L, stat_slots, lambda n: self._buf(n, dev, f32))
        nbytes = lib.mpv_fwd_workspace_bytes(shape)
        ws = self._buf((max(nbytes, 1),), dev, torch.uint8)
        args = H.FwdArgs(H.ptr(y), H.ptr(fe_out), H.ptr(fx_out), self.gemm,
                         *self._gemm_operands(Rop, eps), H.ptr(T),
                         H.ptr(rowstat), H.ptr(bstat), H.ptr(colsum), H.ptr(ws), nbytes)
        H.check(lib.mpv_probit_fwd(shape, args, H.stream_of(dev)), "mpv_probit_fwd")
        return dict(rowstat=rowstat, bstat=bstat, colsum=colsum, T=T, packed=packed)

    def predict_local(self, shape, fx_out, Rop, eps, want_indiv=True, seed_advance=None):
        """mpv_probit_predict.  No host sync; the workspace comes from the
        caching allocator (the graph pool inside a capture)."""
        lib = H.load_library()
        dev = fx_out.device
        B, L = shape.B, shape.L
        colsum = self._buf((B, L), dev, torch.float32)
        indiv = self._buf((B, L), dev, torch.float32) if want_indiv else None
        nbytes = lib.mpv_predict_workspace_bytes(shape)
        ws = self._buf((max(nbytes, 1),), dev, torch.uint8)
        args = H.PredictArgs(H.ptr(fx_out), self.gemm, *self._gemm_operands(Rop, eps),
                             H.ptr(colsum), H.ptr(indiv),
                             H.ptr(seed_advance), H.ptr(ws), nbytes)
        H.check(lib.mpv_probit_predict(shape, args, H.stream_of(dev)), "mpv_probit_predict")
        return colsum, indiv

    @staticmethod
    def indiv_from_colsum(colsum, S_total):
        """The all-reduced (B, L) column sums / S_total: a plain fp32 division
        (by a device scalar; torch multiplies by the reciprocal of a host one)."""
        return colsum / torch.full((), float(S_total), dtype=torch.float32, device=colsum.device)

    def _final_args(self, shape, bstat, colsum, fe_mu, fe_logvar, fx_mu, fx_logvar, nll_coeff,
                    c_coeff, seed_advance=None):
        dev = fe_mu.device
        B, L = shape.B, shape.L
        scal = [torch.empty((), device=dev, dtype=torch.float32) for _ in range(6)]
        indiv = torch.empty((B, L), device=dev, dtype=torch.float32)
        indiv_label = torch.empty((B, L), device=dev, dtype=torch.float32)
        args = H.FinalArgs(H.ptr(bstat), H.ptr(colsum), H.ptr(fe_mu), H.ptr(fe_logvar),
                           H.ptr(fx_mu), H.ptr(fx_logvar), fe_mu.shape[1], nll_coeff, c_coeff,
                           *[H.ptr(s) for s in scal], H.ptr(indiv), H.ptr(indiv_label),
                           H.ptr(seed_advance))
        return args, (*scal, indiv, indiv_label)

    def finalize_slots(self, shape, slots, colsum, fe_mu, fe_logvar, fx_mu, fx_logvar, nll_coeff,
                       c_coeff, seed_advance=None):
        """combine_bstats + finalize in one launch (mpv_probit_finalize_shards)."""
        B = shape.B
        bstat = torch.empty((6, B), device=colsum.device, dtype=torch.float32)
        fin, outs = self._final_args(shape, None, colsum, fe_mu, fe_logvar, fx_mu, fx_logvar,
                                     nll_coeff, c_coeff, seed_advance)
        slots = slots.contiguous()
        H.check(H.load_library().mpv_probit_finalize_shards(shape, H.ptr(slots), slots.shape[0],
                                                             H.ptr(bstat), fin,
                                                             H.stream_of(colsum.device)),
                "mpv_probit_finalize_shards")
        return bstat, outs

    def combine_bstats(self, gathered):
        R, _, B = gathered.shape
        out = torch.empty((6, B), device=gathered.device, dtype=torch.float32)
        H.check(H.load_library().mpv_bstat_combine(H.ptr(gathered.contiguous()), R, B, H.ptr(out),
                                                   H.stream_of(gathered.device)),
                "mpv_bstat_combine")
        return out

    def finalize(self, shape, bstat, colsum, fe_mu, fe_logvar, fx_mu, fx_logvar, nll_coeff,
                 c_coeff, seed_advance=None):
        args, outs = self._final_args(shape, bstat, colsum, fe_mu, fe_logvar, fx_mu, fx_logvar,
                                      nll_coeff, c_coeff, seed_advance)
        H.check(H.load_library().mpv_probit_finalize(shape, args, H.stream_of(bstat.device)),
                "mpv_probit_finalize")
        return outs

    def backward_local(self, shape, saved, gscal, live, g_I, g_IL, nll_coeff, c_coeff, want_dR,
                       dR_dtype=torch.float32, kl=False):
        """One mpv_probit_bwd call: dR_dtype float64 is written in fp64
        directly, and the KL backward runs in the same call."""
        lib = H.load_library()
        dev = gscal.device
        B, L, z = shape.B, shape.L, shape.z
        n_fe = 2 * B * L
        dR64 = None
        if want_dR and dR_dtype == torch.float64:
            dR64 = self._buf((L, z), dev, torch.float64)
        with_32 = want_dR and dR64 is None
        flat = self._buf((n_fe + (L * z if with_32 else 0),), dev, torch.float32)
        dfe_dfx = flat[:n_fe].view(2, B, L)
        dR = flat[n_fe:].view(L, z) if with_32 else dR64
        nbytes = lib.mpv_bwd_workspace_bytes(shape, self.gemm)
        ws = self._buf((max(nbytes, 1),), dev, torch.uint8)
        kl_outs, kl_ref = None, None
        if kl:
            kl_args, kl_outs = self._kl_args(saved["fe_mu"], saved["fe_logvar"], saved["fx_mu"],
                                             saved["fx_logvar"], gscal, live)
            kl_ref = ctypes.byref(kl_args)
        args = H.BwdArgs(H.ptr(saved["y"]), H.ptr(saved["fe_out"]), H.ptr(saved["fx_out"]),
                         self.gemm, *self._eps_operands(saved["eps"]), H.ptr(saved["T"]),
                         H.ptr(saved["rowstat"]),
                         H.ptr(saved["bstat"]), H.ptr(gscal), H.ptr(g_I), H.ptr(g_IL),
                         nll_coeff, c_coeff, live, H.ptr(dfe_dfx),
                         H.ptr(dR if with_32 else None), H.ptr(ws), nbytes, H.ptr(dR64),
                         ctypes.cast(kl_ref, ctypes.c_void_p) if kl_ref is not None else None)
        H.check(lib.mpv_probit_bwd(shape, args, H.stream_of(dev)), "mpv_probit_bwd")
        if kl:
            return flat, dfe_dfx, dR, kl_outs
        return flat, dfe_dfx, dR

    @staticmethod
    def _kl_args(fe_mu, fe_logvar, fx_mu, fx_logvar, gscal, live=0x3F):
        B, d = fe_mu.shape
        outs = [torch.empty_like(fe_mu) for _ in range(4)]
        args = H.KlBwdArgs(H.ptr(fe_mu), H.ptr(fe_logvar), H.ptr(fx_mu), H.ptr(fx_logvar), B, d,
                           H.ptr(gscal), *[H.ptr(o) for o in outs], live)
        return args, outs  # outs: g_fe_mu, g_fe_logvar, g_fx_mu, g_fx_logvar

    def kl_backward(self, fe_mu, fe_logvar, fx_mu, fx_logvar, gscal, live=0x3F):
        args, outs = self._kl_args(fe_mu, fe_logvar, fx_mu, fx_logvar, gscal, live)
        H.check(H.load_library().mpv_kl_bwd(args, H.stream_of(fe_mu.device)), "mpv_kl_bwd")
        return outs


class LocalExchange:
    """Single shard: global statistics are the local ones.

    The exchange interface, which mpvae_dist.SampleShardExchange implements
    with collectives.  ``local``: no other shard exists, so the backward may
    write dR in r_sqrt_sigma's own dtype and fuse the KL backward, and predict
    divides in its own launch; a SampleShardExchange is never local, a world
    of one included."""
    world, local = 1, True

    def agree_seed(self, seed, device):
        """The Philox seed every shard draws from."""
        return seed

    def verify_replicas(self, tensors, names=None):
        """Raise unless every shard holds the same tensors."""

    def stat_slots(self):
        """backend.forward_local's stat_slots: None, or (world, this shard's slot)."""
        return None

    def finalize(self, backend, shape, loc, *fin, seed_advance=None):
        """(the global (6, B) bstat, the 8 outputs) from this shard's
        forward_local output `loc`; fin = (fe_mu, fe_logvar, fx_mu, fx_logvar,
        nll_coeff, c_coeff)."""
        return loc["bstat"], backend.finalize(shape, loc["bstat"], loc["colsum"], *fin,
                                              seed_advance=seed_advance)

    def reduce_colsum(self, colsum):
        """predict_local's (B, L) sums, summed over the shards in place."""
        return colsum

    def reduce_grads(self, flat):
        """backward_local's flat buffer, summed over the shards in place."""
        return flat


class ElboConfig:
    """Non-tensor arguments of ProbitELBO."""

    def __init__(self, S_total, S_local, s_offset, nll_coeff, c_coeff, noise="explicit",
                 seed=0, offset=0, backend=None, exchange=None, gemm="f16x3", seed_advance=None):
        self.S_total, self.S_local, self.s_offset = int(S_total), int(S_local), int(s_offset)
        self.nll_coeff, self.c_coeff = float(nll_coeff), float(c_coeff)
        # seed: an int, or a one-element int64 device tensor (HipShardBackend.make_noise)
        self.noise, self.offset = noise, int(offset)
        self.seed = seed if isinstance(seed, torch.Tensor) else int(seed)
        self.backend = backend if backend is not None else HipShardBackend(gemm)
        # a device int64 key tensor the finalize launch advances by 1 once the
        # noise has read it (args.mpvae_seed_advance), or None
        self.seed_advance = seed_advance
        self.exchange = exchange if exchange is not None else LocalExchange()


def _operands(be, cfg, shape, device, R, eps):
    """(eps, Rop): the noise and r_sqrt_sigma as the backend's GEMM operands.
    Philox noise (cfg.noise) is drawn on the device -- a small r_sqrt_sigma's
    split rides on that launch (make_noise_and_R) -- explicit noise is eps."""
    if cfg.noise == "philox":
        return be.make_noise_and_R(shape, device, cfg.seed, cfg.offset, R)
    eps = _f32(eps, "noise")
    want = (cfg.S_local, shape.B, shape.z)
    if tuple(eps.shape) != want:
        raise ValueError(f"noise must be {want}, got {tuple(eps.shape)}")
    return be.prepare_noise(eps, shape), be.prepare_R(R)


def probit_predict(fx_out, R, eps, cfg):
    """indiv_prob = mean_s E_x (mpvae.py:180, 203) alone, with no labels, no
    label branch and no loss terms: ProbitELBO.forward's noise and operand
    preparation, then the backend's predict_local (mpv_probit_predict on the
    GPU, mpvh_probit_predict for CPU tensors).  Sharded (cfg.exchange): one
    all_reduce(SUM) of the (B, L) column sums, then a plain division by
    S_total.  No autograd: the result never has a grad_fn."""
    with torch.no_grad():
        be, ex = cfg.backend, cfg.exchange
        fx_out = _f32(fx_out.detach(), "fx_out")
        B, L = fx_out.shape
        if R.dim() != 2 or R.shape[0] != L:
            raise ValueError(f"r_sqrt_sigma must be (label_dim={L}, z_dim), got {tuple(R.shape)}")
        R = R.detach()
        z = R.shape[1]
        ex.verify_replicas((fx_out, R), names=("fx_out", "r_sqrt_sigma"))
        shape = be.shape(cfg.S_local, cfg.S_total, cfg.s_offset, B, L, z)
        eps, Rop = _operands(be, cfg, shape, fx_out.device, R, eps)
        colsum, indiv = be.predict_local(shape, fx_out, Rop, eps, want_indiv=ex.local,
                                         seed_advance=cfg.seed_advance)
        if not ex.local:
            indiv = be.indiv_from_colsum(ex.reduce_colsum(colsum), cfg.S_total)
        return indiv


class ProbitELBO(torch.autograd.Function):
    """(total, nll, nll_x, c, c_x, kl, indiv_prob, indiv_prob_label) of mpvae.py:145-210."""

    @staticmethod
    def forward(ctx, y, fe_out, fe_mu, fe_logvar, fx_out, fx_mu, fx_logvar, R, eps, cfg):
        be = cfg.backend
        y, fe_out, fx_out = _f32(y, "input_label"), _f32(fe_out, "fe_out"), _f32(fx_out, "fx_out")
        fe_mu, fe_logvar = _f32(fe_mu, "fe_mu"), _f32(fe_logvar, "fe_logvar")
        fx_mu, fx_logvar = _f32(fx_mu, "fx_mu"), _f32(fx_logvar, "fx_logvar")
        B, L = y.shape
        if fe_out.shape != (B, L) or fx_out.shape != (B, L):
            raise ValueError(f"fe_out/fx_out must be {(B, L)}, got {tuple(fe_out.shape)}, "
                             f"{tuple(fx_out.shape)}")
        if R.dim() != 2 or R.shape[0] != L:
            raise ValueError(f"r_sqrt_sigma must be (label_dim={L}, z_dim), got {tuple(R.shape)}")
        z = R.shape[1]
        cfg.exchange.verify_replicas((y, fe_out, fx_out, R))
        shape = be.shape(cfg.S_local, cfg.S_total, cfg.s_offset, B, L, z)
        eps, Rop = _operands(be, cfg, shape, y.device, R, eps)
        need = ctx.needs_input_grad
        keep_T = need[1] or need[4] or need[7]
        fin = (fe_mu, fe_logvar, fx_mu, fx_logvar, cfg.nll_coeff, cfg.c_coeff)
        loc = be.forward_local(shape, y, fe_out, fx_out, Rop, eps, keep_T,
                               stat_slots=cfg.exchange.stat_slots())
        bstat, outs = cfg.exchange.finalize(be, shape, loc, *fin, seed_advance=cfg.seed_advance)
        ctx.set_materialize_grads(False)
        ctx.cfg, ctx.shape, ctx.r_dtype, ctx.keep_T = cfg, shape, R.dtype, keep_T
        ctx.consumed = False
        if any(need[:8]):
            ctx.saved = dict(y=y, fe_out=fe_out, fx_out=fx_out, eps=eps, T=loc["T"],
                             rowstat=loc["rowstat"], bstat=bstat, fe_mu=fe_mu,
                             fe_logvar=fe_logvar, fx_mu=fx_mu, fx_logvar=fx_logvar)
        return outs

    @staticmethod
    def backward(ctx, g_total, g_nll, g_nll_x, g_c, g_c_x, g_kl, g_I, g_IL):
        if ctx.consumed:
            raise RuntimeError("ProbitELBO backward reuses its forward buffers in place; "
                               "backward through the same compute_loss twice is not supported")
        ctx.consumed = True
        cfg, shape, be, sv = ctx.cfg, ctx.shape, ctx.cfg.backend, ctx.saved
        need = ctx.needs_input_grad
        gs = [g_total, g_nll, g_nll_x, g_c, g_c_x, g_kl]
        live = sum(1 << i for i, g in enumerate(gs) if g is not None)
        dev = sv["y"].device
        if live == 1:
            # total_loss.backward() alone: a backend reads only the live slot,
            # so the upstream gradient's own storage is gscal (no zeros + stack:
            # two launches fewer per step)
            gscal = gs[0].reshape((1,)).to(torch.float32).contiguous()
        else:
            zero = torch.zeros((), device=dev, dtype=torch.float32)
            gscal = torch.stack([zero if g is None else g.reshape(()).to(torch.float32)
                                 for g in gs])
        g_I = None if g_I is None else g_I.to(torch.float32).contiguous()
        g_IL = None if g_IL is None else g_IL.to(torch.float32).contiguous()
        grads = [None] * 10
        want_kl = need[2] or need[3] or need[5] or need[6]
        gk = None
        if ctx.keep_T and (need[1] or need[4] or need[7]):
            # one shard: dR straight in R's dtype and the KL backward in the
            # same call (two launches fewer); sharded: the packed fp32 buffer
            # is summed over the ranks first
            dR_dtype = ctx.r_dtype if cfg.exchange.local else torch.float32
            res = be.backward_local(shape, sv, gscal, live, g_I, g_IL, cfg.nll_coeff,
                                    cfg.c_coeff, need[7], dR_dtype=dR_dtype, kl=want_kl)
            flat, dfe_dfx, dR = res[:3]
            if want_kl:
                gk = res[3]
            cfg.exchange.reduce_grads(flat)
            if need[1]:
                grads[1] = dfe_dfx[0]
            if need[4]:
                grads[4] = dfe_dfx[1]
            if need[7]:
                grads[7] = dR if dR.dtype == ctx.r_dtype else be.from_f32(dR, ctx.r_dtype)
        if want_kl:
            if gk is None:
                gk = be.kl_backward(sv["fe_mu"], sv["fe_logvar"], sv["fx_mu"], sv["fx_logvar"],
                                    gscal, live)
            grads[2], grads[3], grads[5], grads[6] = gk
        ctx.saved = None
        return tuple(grads)


class FusedReparam(torch.autograd.Function):
    """z = mu + eps*exp(0.5*logvar) for the label and the feature encoder in one
    launch (mpvae.py:66-74).  eps is an input (drawn by the caller with
    torch.randn_like, so the RNG stream matches the reference's draw order).

    mu and logvar are also returned, as fresh copies the kernel writes in the
    same pass (ordinary tensors: a caller may modify them in place, as it may
    the reference's): the VAE returns those to the caller, so the gradient
    compute_loss's KL sends them arrives here and is added inside
    mpv_reparam_bwd -- the one add autograd would otherwise launch per tensor
    when two consumers of an encoder head meet."""

    @staticmethod
    def forward(ctx, mu_e, lv_e, eps_e, mu_x, lv_x, eps_x):
        H.require_gpu(mu_e, mu_x)
        mu_e, lv_e, eps_e = (_f32(t, "reparam input") for t in (mu_e, lv_e, eps_e))
        mu_x, lv_x, eps_x = (_f32(t, "reparam input") for t in (mu_x, lv_x, eps_x))
        z_e, z_x = torch.empty_like(mu_e), torch.empty_like(mu_x)
        outs = [torch.empty_like(t) for t in (mu_e, lv_e, mu_x, lv_x)]
        a = H.ReparamArgs(H.ptr(mu_e), H.ptr(lv_e), H.ptr(eps_e), H.ptr(z_e), mu_e.numel(),
                          H.ptr(mu_x), H.ptr(lv_x), H.ptr(eps_x), H.ptr(z_x), mu_x.numel(),
                          *[H.ptr(o) for o in outs])
        H.check(H.load_library().mpv_reparam_fwd(a, H.stream_of(mu_e.device)), "mpv_reparam_fwd")
        ctx.save_for_backward(lv_e, eps_e, lv_x, eps_x)
        ctx.set_materialize_grads(False)
        return (z_e, z_x, *outs)

    @staticmethod
    def backward(ctx, gz_e, gz_x, gmu_e_in, glv_e_in, gmu_x_in, glv_x_in):
        lv_e, eps_e, lv_x, eps_x = ctx.saved_tensors
        gmu_e, glv_e = torch.empty_like(lv_e), torch.empty_like(lv_e)
        gmu_x, glv_x = torch.empty_like(lv_x), torch.empty_like(lv_x)
        c = lambda g: None if g is None else _f32(g, "reparam gradient")
        gz_e, gz_x = c(gz_e), c(gz_x)
        gmu_e_in, glv_e_in, gmu_x_in, glv_x_in = (c(g) for g in (gmu_e_in, glv_e_in, gmu_x_in,
                                                                  glv_x_in))
        a = H.ReparamBwdArgs(H.ptr(gz_e), H.ptr(lv_e), H.ptr(eps_e), H.ptr(gmu_e), H.ptr(glv_e),
                             lv_e.numel(), H.ptr(gz_x), H.ptr(lv_x), H.ptr(eps_x), H.ptr(gmu_x),
                             H.ptr(glv_x), lv_x.numel(), H.ptr(gmu_e_in), H.ptr(glv_e_in),
                             H.ptr(gmu_x_in), H.ptr(glv_x_in))
        H.check(H.load_library().mpv_reparam_bwd(a, H.stream_of(lv_e.device)), "mpv_reparam_bwd")
        return gmu_e, glv_e, None, gmu_x, glv_x, None


class SingleReparam(torch.autograd.Function):
    """One encoder's reparameterisation (label_reparameterize / feat_reparameterize)."""

    @staticmethod
    def forward(ctx, mu, lv, eps):
        H.require_gpu(mu)
        mu, lv, eps = (_f32(t, "reparam input") for t in (mu, lv, eps))
        z = torch.empty_like(mu)
        a = H.ReparamArgs(H.ptr(mu), H.ptr(lv), H.ptr(eps), H.ptr(z), mu.numel(),
                          None, None, None, None, 0, None, None, None, None)
        H.check(H.load_library().mpv_reparam_fwd(a, H.stream_of(mu.device)), "mpv_reparam_fwd")
        ctx.save_for_backward(lv, eps)
        return z

    @staticmethod
    def backward(ctx, gz):
        lv, eps = ctx.saved_tensors
        gmu, glv = torch.empty_like(lv), torch.empty_like(lv)
        a = H.ReparamBwdArgs(H.ptr(gz.contiguous()), H.ptr(lv), H.ptr(eps), H.ptr(gmu),
                             H.ptr(glv), lv.numel(), None, None, None, None, None, 0)
        H.check(H.load_library().mpv_reparam_bwd(a, H.stream_of(lv.device)), "mpv_reparam_bwd")
        return gmu, glv, None
