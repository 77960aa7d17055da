"""The per-step host syncs of the reference training loop, batched (SURVEY.md
section 8(f) rank 3).

After ``total_loss.backward()`` the reference loop (fairsoft_train.py:140-162)
synchronises with the device once per parameter in ``has_finite_grad``
(fairsoft_utils.py:28-41: ``torch.isnan(g).any() or torch.isinf(g).any()`` is a
host bool per tensor) and once per logged scalar (eight ``.item()`` calls,
fairsoft_train.py:154-162).  Each sync drains the stream.  Here:

* ``has_finite_grad(model)`` -- the same answer from one fused multi-tensor
  reduction and one sync: max |g| of every gradient (``torch._foreach_norm``
  with ord = inf, which propagates NaN and cannot overflow), all finite;
* ``step_scalars(**tensors)`` -- every 0-d tensor the loop logs, fetched by ONE
  device-to-host copy, as Python floats (what ``.item()`` returns).

Both are torch glue around the loop, not kernels of the hot path: they run on
whatever device the tensors live on.

The loop bodies themselves are one call each (``TrainStep``, ``FairTrainStep``,
``CalibrationStep``, ``EvalPass``), and so is the feeding of their batches:
``DeviceSplit`` keeps a split on the device and ``run_epoch`` /
``capture_epoch`` / ``validate_epoch`` / ``run_split`` gather every batch there
(mpv_gather_batch, csrc/gather.hip) instead of the reference's per-batch
``torch.from_numpy(data[idx]).float().to(device)``.
"""
import collections
import contextlib
import copy
import ctypes
import functools

import torch

import mpvae_hip as H


def has_finite_grad(model):
    """fairsoft_utils.py:28-41 with one host sync: True iff every existing
    gradient of ``model`` (a module, or a tensor with .grad) is finite."""
    if isinstance(model, torch.Tensor):
        grads = [model.grad]
    else:
        grads = [p.grad for p in model.parameters() if p.grad is not None]
    grads = [g for g in grads if g is not None]
    if not grads:
        return True
    peaks = torch._foreach_norm(grads, float("inf"))
    by_dtype = {}
    for pk in peaks:  # one stack per dtype (fp32 MLP grads, fp64 r_sqrt_sigma grad)
        by_dtype.setdefault(pk.dtype, []).append(pk)
    ok = [torch.isfinite(torch.stack(v)).all() for v in by_dtype.values()]
    return bool((torch.stack(ok).all() if len(ok) > 1 else ok[0]).item())


def step_scalars(**tensors):
    """{name: float} for 0-d tensors (loss components, device metrics) with one
    device-to-host copy instead of one ``.item()`` each (fairsoft_train.py:
    154-162).  Non-tensor values pass through unchanged."""
    names = [k for k, v in tensors.items() if isinstance(v, torch.Tensor)]
    out = {k: v for k, v in tensors.items() if not isinstance(v, torch.Tensor)}
    if names:
        vals = torch.stack([tensors[k].detach().reshape(()).to(torch.float64) for k in names])
        for k, v in zip(names, vals.cpu().tolist()):
            out[k] = v
    return out


def _native_adam(opt):
    """True when ``opt`` is a plain fused torch.optim.Adam that mpv_adam_step
    reproduces (L2 weight decay, float lr, no amsgrad / maximize /
    decoupled weight decay, CUDA parameters)."""
    if type(opt) is not torch.optim.Adam:
        return False
    for g in opt.param_groups:
        if (not g.get("fused") or g.get("amsgrad") or g.get("maximize")
                or g.get("differentiable") or g.get("decoupled_weight_decay", False)
                or isinstance(g["lr"], torch.Tensor) or isinstance(g["betas"][0], torch.Tensor)):
            return False
        if any(p.device.type != "cuda" or p.dtype not in (torch.float32, torch.float64)
               for p in g["params"]):
            return False
    return True


def adam_step(opt, found_inf, updates=None, sched=None):
    """optimizer.step() of a fused torch.optim.Adam in one mpv_adam_step launch
    per parameter group (csrc/adam.hip) instead of torch's multi-tensor kernel,
    which runs the VAE's 1.5 M parameters on ~25 workgroups (DESIGN.md
    section 11), then one mpv_adam_finish launch.  Same state (``step``,
    ``exp_avg``, ``exp_avg_sq`` in ``opt.state``), same step-count protocol as
    torch's capturable fused path (+1 for the update, -found_inf after), same
    per-element arithmetic; nothing is written when ``found_inf`` is 1.
    ``updates`` (an int64 device scalar, or None) counts the applied updates
    and ``sched`` (a DeviceStepLR, or None) takes the scheduler step the
    reference takes after an applied update (fairsoft_train.py:142-146), both
    in the finish launch."""
    lib = H.load_library()
    all_steps = []
    for gi, g in enumerate(opt.param_groups):
        params = [p for p in g["params"] if p.grad is not None]
        if not params:
            continue
        for p in params:
            st = opt.state[p]
            if len(st) == 0:  # torch's _init_group for fused Adam
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        all_steps += [opt.state[p]["step"] for p in params]
        beta1, beta2 = g["betas"]
        lr_dev = None if sched is None else sched.lr[gi:gi + 1]
        for c in range(0, len(params), H.ADAM_MAX_TENSORS):
            a = H.AdamArgs(n=0, lr=float(g["lr"]), beta1=float(beta1), beta2=float(beta2),
                           weight_decay=float(g["weight_decay"]), eps=float(g["eps"]),
                           found_inf=H.ptr(found_inf), lr_dev=H.ptr(lr_dev))
            for p in params[c:c + H.ADAM_MAX_TENSORS]:
                st = opt.state[p]
                ts = (p, p.grad, st["exp_avg"], st["exp_avg_sq"])
                if not all(t.is_contiguous() and t.dtype == p.dtype for t in ts):
                    raise ValueError("mpv_adam_step needs contiguous parameters, gradients "
                                     "and state of the parameter's dtype")
                a.t[a.n] = H.AdamTensor(param=p.data_ptr(), grad=p.grad.data_ptr(),
                                        exp_avg=st["exp_avg"].data_ptr(),
                                        exp_avg_sq=st["exp_avg_sq"].data_ptr(),
                                        step=st["step"].data_ptr(), numel=p.numel(),
                                        is_f64=int(p.dtype == torch.float64))
                a.n += 1
            H.check(lib.mpv_adam_step(ctypes.byref(a), H.stream_of(params[0].device)),
                    "mpv_adam_step")
    if not all_steps and updates is None and sched is None:
        return
    dev = (all_steps[0] if all_steps else updates if updates is not None else sched.lr).device
    for c in range(0, max(1, len(all_steps)), H.ADAM_FINISH_MAX):
        chunk = all_steps[c:c + H.ADAM_FINISH_MAX]
        f = H.AdamFinishArgs(n_steps=len(chunk), found_inf=H.ptr(found_inf))
        for i, st in enumerate(chunk):
            f.steps[i] = st.data_ptr()
        if c == 0:  # the counter and the scheduler step once per optimizer step
            f.updates = H.ptr(updates)
            if sched is not None:
                f.n_lr, f.lr, f.last_epoch = sched.lr.numel(), H.ptr(sched.lr), \
                    H.ptr(sched.last_epoch)
                f.step_size, f.gamma = sched.step_size, sched.gamma
        H.check(lib.mpv_adam_finish(ctypes.byref(f), H.stream_of(dev)), "mpv_adam_finish")


class DeviceStepLR:
    """The state of a torch.optim.lr_scheduler.StepLR (fairsoft_jaccard.py:67-68)
    held on the device, so TrainStep can take the reference's scheduler step
    (after an applied update only, fairsoft_train.py:142-145) with no host
    sync and inside a captured graph.  ``lr`` holds one float64 learning rate
    per param group, ``last_epoch`` the scheduler's epoch counter; both follow
    torch's StepLR bit for bit (the chainable ``lr * gamma`` in double when
    last_epoch is a non-zero multiple of step_size).  The optimizer's
    ``param_groups[i]["lr"]`` and the scheduler's ``last_epoch`` /
    ``get_last_lr()`` would go stale while TrainStep owns them; so (ADVICE
    r04):
      * ``opt.state_dict()`` and ``sched.state_dict()`` sync first (an
        optimizer state-dict pre-hook; the scheduler's method wrapped), so a
        checkpoint holds the current lr and epoch;
      * the scheduler's own ``step()`` raises while TrainStep owns it (the
        reference loop's host ``scheduler.step()`` would step it twice) until
        ``release()`` hands it back, synced;
      * a host edit of ``param_groups[i]["lr"]`` is adopted by the device
        state before the next step (``adopt_host_lr``, called by TrainStep: a
        host-side comparison, no device sync), with a warning.
    ``sync()`` (one host sync) writes the device state back on demand, e.g.
    before logging."""

    def __init__(self, sched, opt):
        if type(sched) is not torch.optim.lr_scheduler.StepLR:
            raise ValueError("TrainStep runs torch.optim.lr_scheduler.StepLR (the reference's "
                             f"scheduler) on the device; got {type(sched).__name__}")
        if sched.optimizer is not opt:
            raise ValueError("the scheduler must wrap TrainStep's optimizer")
        dev = next(p.device for g in opt.param_groups for p in g["params"])
        self.sched, self.opt = sched, opt
        self.lr = torch.tensor([float(g["lr"]) for g in opt.param_groups], dtype=torch.float64,
                               device=dev)
        self.last_epoch = torch.tensor(int(sched.last_epoch), dtype=torch.int64, device=dev)
        self.step_size, self.gamma = float(sched.step_size), float(sched.gamma)
        self._epoch0 = int(sched.last_epoch)
        self._host_lr = [float(g["lr"]) for g in opt.param_groups]  # as last synced / adopted
        self._hook = opt.register_state_dict_pre_hook(lambda _opt: self.sync())
        self._sched_state_dict, self._sched_step = sched.state_dict, sched.step
        self._sched_load = sched.load_state_dict

        def state_dict():
            self.sync()
            return self._sched_state_dict()

        def load_state_dict(state):
            # a resumed scheduler checkpoint: the device epoch and
            # lr follow it, so the decay boundaries are the checkpoint's and
            # the next sync() does not write a stale epoch back
            self._sched_load(state)
            self._adopt(int(sched.last_epoch), [float(g["lr"]) for g in opt.param_groups])

        def step(*a, **k):
            raise RuntimeError("this StepLR is stepped on the device by TrainStep after every "
                               "applied update (fairsoft_train.py:142-145); do not call "
                               "scheduler.step() as well -- TrainStep.release_scheduler() hands "
                               "it back")
        sched.state_dict, sched.step, sched.load_state_dict = state_dict, step, load_state_dict

    def _adopt(self, epoch, lrs):
        """Host values -> the device state, stream-ordered, without a host wait:
        the lrs go through a pinned staging tensor (the caching host allocator
        keeps it alive until the copy has run)."""
        src = torch.tensor(lrs, dtype=torch.float64)
        if self.lr.is_cuda:
            src = src.pin_memory()
        self.lr.copy_(src, non_blocking=True)
        if epoch is not None:
            self.last_epoch.fill_(epoch)
            self._epoch0 = epoch
        self._host_lr = list(lrs)

    def sync(self):
        """Copy the device lr / last_epoch into the optimizer and the scheduler."""
        lrs = self.lr.tolist()
        epoch = int(self.last_epoch)
        for g, v in zip(self.opt.param_groups, lrs):
            g["lr"] = v
        self.sched.last_epoch = epoch
        self.sched._last_lr = list(lrs)
        self.sched._step_count += epoch - self._epoch0
        self._epoch0 = epoch
        self._host_lr = list(lrs)
        return lrs

    def adopt_host_lr(self):
        """A param group's lr changed on the host since the last sync: the
        device lr takes it (a host-side compare; the copy is stream-ordered from
        a pinned staging tensor, so the host does not wait for the device)."""
        now = [float(g["lr"]) for g in self.opt.param_groups]
        if now != self._host_lr:
            import warnings
            warnings.warn("optimizer param_groups lr edited on the host while TrainStep owns "
                          "the StepLR: the device lr adopts the new value", stacklevel=3)
            self._adopt(None, now)

    def release(self):
        """Sync, then hand the scheduler and optimizer back to host control."""
        lrs = self.sync()
        self._hook.remove()
        self.sched.state_dict, self.sched.step = self._sched_state_dict, self._sched_step
        self.sched.load_state_dict = self._sched_load
        return lrs


def _warm_capture(body, warmup, prepare=None):
    """``warmup`` eager runs of ``body()`` (at least one) on a side stream, then
    ``prepare()`` and the capture of one more run: ``(the HIP graph, what the
    captured run returned)``."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(max(1, warmup)):
            body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    if prepare is not None:
        prepare()
    with torch.cuda.graph(graph):
        out = body()
    return graph, out


class _Captured:
    """One captured HIP graph: ``graph``, the static input buffers ``bufs`` it
    reads and ``out``, what the captured run of ``body(*bufs)`` returned (see
    ``_warm_capture``).  An epoch's record also names its ``split`` and ``B``."""

    def __init__(self, body, bufs, warmup, prepare=None, split=None, B=None):
        self.bufs, self.split, self.B = list(bufs), split, B
        self.graph, self.out = _warm_capture(lambda: body(*self.bufs), warmup, prepare)

    def replay(self, *batch):
        """Copy ``batch`` into the static buffers (an epoch's gather fills them
        inside the graph: no batch), replay, and return the static outputs."""
        for buf, x in zip(self.bufs, batch):
            buf.copy_(x)
        self.graph.replay()
        return self.out


class _Capturing:
    """``graph`` and ``out`` of the object's captured record ``_captured`` (None
    until ``capture()``)."""

    _captured = None
    graph = property(lambda self: self._captured and self._captured.graph)
    out = property(lambda self: self._captured and self._captured.out)


@contextlib.contextmanager
def _eval_mode(model):
    """``model.eval()`` under ``no_grad``; the previous mode is restored."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        model.train(was_training)


_SPLIT_ELEMS = {torch.float32: H.EL_F32, torch.float64: H.EL_F64, torch.int32: H.EL_I32,
                torch.int64: H.EL_I64, torch.uint8: H.EL_U8}  # dtype -> mpv_elem


class DeviceSplit:
    """A dataset split resident on one device, and the batches gathered from
    it there: what the reference builds per batch on the host as
    ``torch.from_numpy(data.input_feat[idx]).float().to(device)`` for the
    features, the labels and the sensitive columns (fairsoft_train.py:48-56,
    :235-243, :266-267).

    ``labels`` (N, L), ``feats`` (N, F) and ``sensitive_feat`` (N, n, optional)
    are numpy arrays or tensors; each is held contiguous in its own dtype
    (fp32, fp64, int32, int64 or uint8, so a large 0/1 label matrix can stay
    uint8) on ``device`` (default: where ``feats`` already lives, the CPU for a
    numpy array).

    ``gather(order, start, B)`` returns rows ``order[start : start + B]`` as
    ``(label fp32, feat fp32, sens in its own dtype)`` -- the values ``.float()``
    gives.  On a GPU this is one ``mpv_gather_batch`` launch (csrc/gather.hip);
    on the CPU, torch indexing with the same semantics.  The dispatch is by the
    split's device; there is no fallback from one to the other.  A position
    outside the order or an index outside the split reads nothing: the row is
    NaN (fp32 outputs; a floating-point ``sens``) or 0 (an integer ``sens``) and
    the device flag ``bad`` is set.  ``check()`` (one host sync) raises if it
    is.  A numpy ``order`` is range-checked on the host before it is uploaded;
    the flag is the backstop for an order that is already a tensor.

    The split also owns the state an epoch loop walks (TrainStep.run_epoch):
    ``order`` (int64, capacity N; the rows past the current order hold -1),
    ``n_order`` and the device ``cursor``.  Their addresses never change, so a
    captured epoch graph reads them on every replay."""

    def __init__(self, labels, feats, sensitive_feat=None, device=None):
        if device is None:
            device = feats.device if isinstance(feats, torch.Tensor) else "cpu"
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.labels = self._hold(labels, "labels")
        self.feats = self._hold(feats, "feats")
        self.sens = None if sensitive_feat is None else self._hold(sensitive_feat,
                                                                   "sensitive_feat")
        self.n_rows = int(self.labels.shape[0])
        held = [t for t in (self.labels, self.feats, self.sens) if t is not None]
        if self.n_rows < 1 or any(t.shape[0] != self.n_rows or t.shape[1] < 1 for t in held):
            raise ValueError("DeviceSplit needs labels, feats and sensitive_feat with the same "
                             "number (>= 1) of rows and at least one column each")
        self.order = torch.arange(self.n_rows, dtype=torch.int64, device=self.device)
        self.n_order = self.n_rows
        self.cursor = torch.zeros((), dtype=torch.int64, device=self.device)
        self.bad = torch.zeros((), dtype=torch.uint8, device=self.device)

    def _hold(self, x, name):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(_np().ascontiguousarray(x))
        if t.dtype not in _SPLIT_ELEMS:
            raise ValueError(f"DeviceSplit holds fp32, fp64, int32, int64 or uint8 ({name} is "
                             f"{t.dtype})")
        if t.dim() != 2:
            raise ValueError(f"DeviceSplit: {name} must be a 2-D matrix (got {tuple(t.shape)})")
        return t.detach().to(self.device).contiguous()

    # ----------------------------------------------------------------- order
    def _index_tensor(self, order):
        """``order`` as an int64 tensor on the split's device.  A numpy order is
        range-checked on the host first; a tensor is taken as it is."""
        if isinstance(order, torch.Tensor):
            if order.dim() != 1 or order.dtype.is_floating_point or order.dtype == torch.bool:
                raise ValueError("order must be a 1-D integer tensor")
            return order.detach().to(device=self.device, dtype=torch.int64).contiguous()
        np = _np()
        arr = np.asarray(order)
        if arr.ndim != 1 or arr.dtype.kind not in "iu":
            raise ValueError("order must be a 1-D array of integer row indices")
        if arr.size and (int(arr.min()) < 0 or int(arr.max()) >= self.n_rows):
            raise IndexError(f"order holds a row index outside [0, {self.n_rows}) "
                             f"(min {int(arr.min())}, max {int(arr.max())})")
        src = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64))
        if self.device.type != "cuda":
            return src.clone()
        return src.pin_memory().to(self.device, non_blocking=True)

    def set_order(self, order):
        """Upload an epoch's order (``data.train_idx`` after the caller's
        ``np.random.shuffle``; None: the identity) into the static order buffer
        and put the cursor at 0; returns its length.  No host sync."""
        if order is None:
            idx = torch.arange(self.n_rows, dtype=torch.int64, device=self.device)
        else:
            idx = self._index_tensor(order)
        n = int(idx.shape[0])
        if n > self.n_rows:
            raise ValueError(f"an epoch's order holds at most the split's {self.n_rows} rows "
                             f"(got {n})")
        self.order[:n].copy_(idx)
        if n < self.n_rows:
            self.order[n:].fill_(-1)
        self.n_order = n
        self.cursor.zero_()
        return n

    # ---------------------------------------------------------------- gather
    def _sources(self, sens):
        src = [(self.labels, torch.float32), (self.feats, torch.float32)]
        if sens:
            if self.sens is None:
                raise ValueError("this DeviceSplit holds no sensitive_feat")
            src.append((self.sens, self.sens.dtype))
        return src

    def _gather(self, idx, n_idx, B, start=0, pos=None, advance=False, out=None, sens=True):
        """Rows ``idx[p : p + B]`` (``idx`` None: rows p .. p + B) of every source,
        p = ``pos`` (a device int64 scalar) or ``start``; with ``advance`` the
        cursor ``pos`` moves by B afterwards."""
        B = int(B)
        if B < 1:
            raise ValueError(f"a batch needs at least one row (got B = {B})")
        if advance and pos is None:
            raise ValueError("advance needs a device cursor")
        src = self._sources(sens)
        if out is None:
            out = [torch.empty((B, t.shape[1]), dtype=dt, device=self.device) for t, dt in src]
        out = list(out)
        if len(out) != len(src) or any(
                o.shape != (B, t.shape[1]) or o.dtype != dt or o.device != self.device
                or not o.is_contiguous() for o, (t, dt) in zip(out, src)):
            raise ValueError("out must hold one contiguous (B, cols) tensor per source, on the "
                             "split's device: label fp32, feat fp32, sens in its own dtype")
        if self.device.type == "cuda":
            a = H.GatherArgs(n_sources=len(src), n_rows=self.n_rows, idx=H.ptr(idx),
                             n_idx=int(n_idx), B=B, start=int(start), pos=H.ptr(pos),
                             advance=int(bool(advance)), bad=H.ptr(self.bad))
            for k, ((t, dt), o) in enumerate(zip(src, out)):
                a.src[k], a.src_elem[k], a.cols[k] = t.data_ptr(), _SPLIT_ELEMS[t.dtype], t.shape[1]
                a.dst[k], a.dst_elem[k] = o.data_ptr(), _SPLIT_ELEMS[dt]
            H.check(H.load_library().mpv_gather_batch(ctypes.byref(a), H.stream_of(self.device)),
                    "mpv_gather_batch")
        else:
            self._gather_cpu(src, out, idx, int(n_idx), B, int(start), pos, advance)
        return tuple(out) if sens else (out[0], out[1], None)

    def _gather_cpu(self, src, out, idx, n_idx, B, start, pos, advance):
        """mpv_gather_batch's semantics on CPU tensors, in torch."""
        p = int(pos) if pos is not None else start
        r = torch.arange(B, dtype=torch.int64)
        ok = (-r <= p) & (n_idx - r > p)  # p + r in [0, n_idx), before the sum is formed
        q = torch.where(ok, r + (p if -B <= p <= n_idx else 0), torch.zeros_like(r))
        rows = q
        if idx is not None and n_idx > 0:
            rows = idx[q.clamp(0, n_idx - 1)]
        ok &= (rows >= 0) & (rows < self.n_rows)
        rows = rows.clamp(0, self.n_rows - 1)
        for (t, dt), o in zip(src, out):
            v = t[rows].to(dt)
            v[~ok] = float("nan") if dt.is_floating_point else 0
            o.copy_(v)
        if not bool(ok.all()):
            self.bad.fill_(1)
        if advance:
            pos += B

    def gather(self, order, start, B, out=None):
        """``(label fp32, feat fp32, sens)`` of rows ``order[start : start + B]``
        (``order`` None: rows ``start .. start + B``); ``sens`` is None when the
        split holds no sensitive_feat.  ``start`` is an int, or a 0-d int64
        tensor on the split's device (read there, no host sync).  ``out``: the
        tensors to write, as returned by an earlier call with the same B."""
        idx = None if order is None else self._index_tensor(order)
        n_idx = self.n_rows if idx is None else int(idx.shape[0])
        pos = start if isinstance(start, torch.Tensor) else None
        if pos is not None and (pos.dtype != torch.int64 or pos.numel() != 1
                                or pos.device != self.device):
            raise ValueError("a tensor start must be one int64 on the split's device")
        return self._gather(idx, n_idx, B, 0 if pos is not None else int(start), pos, False,
                            out, self.sens is not None)

    def next_batch(self, B, advance=True, out=None, sens=True):
        """The B rows of the current order at the device cursor, which then moves
        past them (``advance``): the feed of one step of an epoch."""
        # the bound is the buffer's capacity, not n_order, so that a captured
        # launch stays right for a later, longer order; the rows past the
        # current order hold -1 and are flagged like any other bad index
        return self._gather(self.order, self.n_rows, B, 0, self.cursor, advance, out, sens)

    def check(self):
        """One host sync: raises IndexError if a gather met a position outside its
        order or a row index outside the split since the last check (the rows it
        wrote are NaN / 0), and clears the flag."""
        if int(self.bad):
            self.bad.zero_()
            raise IndexError("DeviceSplit: a gathered batch held a position past the end of its "
                             f"order or a row index outside [0, {self.n_rows}) -- most likely "
                             "`order` holds an out-of-range index; those rows were written as "
                             "NaN / 0")


def epoch_batches(n, batch_size):
    """The reference's batches over n rows (fairsoft_train.py:48-56):
    ``range(n // B + 1)`` over ``[i B, min((i + 1) B, n))`` without the empty last
    one (n a multiple of B) -- ``(full batches, rows of the ragged last batch)``."""
    B = int(batch_size)
    if B < 1:
        raise ValueError(f"batch_size must be >= 1 (got {batch_size})")
    return int(n) // B, int(n) % B


def _np():
    import numpy
    return numpy


def step_args(args, advance_seed=True):
    """``args`` for one step's compute_loss or one batch's predict_proba: with a
    device seed, fresh probit noise every call, on the device -- the finalize
    (or predict) launch advances the key after the noise has read it
    (args.mpvae_seed_advance; no launch of its own)."""
    if advance_seed and isinstance(getattr(args, "mpvae_seed", None), torch.Tensor):
        args = copy.copy(args)
        args.mpvae_seed_advance = True
    return args


def _need_device_philox(args, who, r_draw=False):
    """A capture draws its noise (``r_draw``: and its per-step r_sqrt_sigma) on
    the device, from a key it reads there."""
    if getattr(args, "mpvae_noise", "torch_cpu") != "philox" or not isinstance(
            getattr(args, "mpvae_seed", None), torch.Tensor):
        raise ValueError(f"{who} needs args.mpvae_noise = 'philox' and a one-element int64 "
                         "device tensor as args.mpvae_seed"
                         + (" (args.mpvae_r_draw = 'philox' draws r_sqrt_sigma from the key the "
                            "noise reads, on the device at every replay)" if r_draw else ""))


def _r_draw_mode(args):
    """args.mpvae_r_draw as the steps take it: None (absent: the model's
    r_sqrt_sigma, no draw), "numpy" or "philox" (mpvae.draw_r_sqrt_sigma).  The
    reference redraws r_sqrt_sigma under residue_sigma == "random" alone."""
    import mpvae
    mode = getattr(args, "mpvae_r_draw", None)
    if mode is None:
        return None
    if mode not in mpvae.R_DRAWS:
        raise ValueError(f"args.mpvae_r_draw must be None or one of {mpvae.R_DRAWS} "
                         f"(got {mode!r})")
    if getattr(args, "residue_sigma", None) != "random":
        raise ValueError(f"args.mpvae_r_draw = {mode!r} needs args.residue_sigma = 'random' (got "
                         f"{getattr(args, 'residue_sigma', None)!r}): the model's r_sqrt_sigma is "
                         "trainable or zero there, and the reference never redraws it")
    return mode


def _need_capturable(opt, who):
    """A captured Adam keeps its step counter and bias corrections on the device."""
    if not all(g.get("capturable") for g in opt.param_groups):
        raise ValueError(f"{who} needs torch.optim.Adam(..., fused=True, capturable=True)")


class TrainStep(_Capturing):
    """The loop body of fairsoft_train.py:47-146 (penalty-free) as one call:
    ``model(label, feat)`` -> ``compute_loss`` -> ``backward`` ->
    ``clip_grad_norm_(10)`` -> finite-gradient gate -> optimizer step.

    The gate runs on the device: the optimizer must be a fused Adam
    (``torch.optim.Adam(..., fused=True)``), which takes ``found_inf`` and skips
    the update on the device, step counters included -- the reference's
    ``if has_finite_grad(model): optimizer.step()`` without the host sync.
    ``updates`` counts the applied steps (the reference's succses_updates) on
    the device.  ``scheduler``: the reference's StepLR (fairsoft_jaccard.py:
    67-68), stepped on the device after every applied update
    (fairsoft_train.py:142-145; DeviceStepLR, ``sync_scheduler()`` writes its
    state back to the host objects).  With ``args.mpvae_noise = "philox"`` and
    a device-tensor ``args.mpvae_seed`` nothing in the step waits for the
    host, so ``capture()`` records it in one HIP graph (input batches are
    copied into its static buffers before each replay).

    The batch is the step's argument list: ``inputs`` names the tensors that
    ``__call__`` / ``step``, ``capture``, ``_body`` and ``_objective`` take, in
    order, and that ``run_epoch`` gathers from a ``DeviceSplit``; a subclass
    with a third input declares it there and writes ``_body(self, label, feat,
    sens)``.  ``params`` (default: the model's trainable parameters) are the
    tensors the optimizer steps.

    r_sqrt_sigma is the model's.  Under ``residue_sigma == "random"`` the
    reference's loops draw a fresh one every step instead (fairsoft_train.py:
    60-69, train.py:120); ``args.mpvae_r_draw`` (absent / None: off) reproduces
    that, between the model forward and the loss, into ``r_drawn`` (fp64,
    allocated once), which compute_loss then takes without a gradient:
      "numpy"   ``np.random.uniform`` on the global numpy stream and an upload,
                the reference's line -- its values and stream position bit for
                bit; the step waits for the host, so ``capture()`` refuses it;
      "philox"  one mpv_r_uniform_philox launch keyed by ``args.mpvae_seed``: the
                same distribution from another stream (not numpy's bits); with
                a device seed the finalize launch advances the key afterwards,
                so every step and every replay of a captured step draws anew.
    Any other ``residue_sigma``, and an active ``args.mpvae_shard`` exchange
    (every rank would need the same draw), raise ValueError."""

    inputs = ("label", "feat")

    def __init__(self, model, optimizer, args, max_grad_norm=10.0, advance_seed=True,
                 native_adam=True, scheduler=None, params=None):
        if not optimizer.defaults.get("fused"):
            raise ValueError("TrainStep gates the update on the device: use a fused optimizer "
                             "(torch.optim.Adam(..., fused=True))")
        self.model, self.opt, self.args = model, optimizer, args
        self.max_grad_norm = max_grad_norm
        self.advance_seed = advance_seed
        # a plain fused Adam steps in mpv_adam_step (adam_step); others in torch
        self.native_adam = bool(native_adam) and _native_adam(optimizer)
        self.params = [p for p in model.parameters() if p.requires_grad] \
            if params is None else list(params)
        dev = self.params[0].device
        self.updates = torch.zeros((), dtype=torch.int64, device=dev)  # applied updates
        self.found_inf = torch.zeros((), dtype=torch.float32, device=dev)  # the gate's flag
        self._one = torch.ones((), dtype=torch.float32, device=dev)
        # args.mpvae_r_draw: every step's r_sqrt_sigma is drawn into r_drawn (one
        # buffer for the step's life, so a captured draw has a static address)
        self.r_draw = _r_draw_mode(args)
        self.r_drawn = None
        if self.r_draw is not None:
            self.r_drawn = torch.empty((int(args.label_dim), int(args.z_dim)),
                                       dtype=torch.float64, device=model.r_sqrt_sigma.device)
        self._drop_graphs()
        self.sched = None
        if scheduler is not None:
            if not self.native_adam:
                raise ValueError("a device StepLR needs the native Adam step (a plain fused "
                                 "torch.optim.Adam with a float lr)")
            self.sched = DeviceStepLR(scheduler, optimizer)

    def _drop_graphs(self):
        """No captured record: ``_captured`` is capture()'s, ``_epoch`` capture_epoch's."""
        self._captured = self._epoch = None

    def _grads_by_dtype(self):
        """``self.params``' gradients, one list per dtype (fp32 MLP grads, the
        fp64 r_sqrt_sigma grad): what a multi-tensor op takes in one launch."""
        by_dtype = {}
        for p in self.params:
            if p.grad is not None:
                by_dtype.setdefault(p.grad.dtype, []).append(p.grad)
        return by_dtype

    def _clip(self):
        """torch.nn.utils.clip_grad_norm_(params, max_grad_norm) (fairsoft_train.py:141)
        with the same total norm and coefficient (computed in the promoted
        dtype: fp64, as r_sqrt_sigma's gradient is fp64), but the coefficient
        cast to each gradient dtype before the multi-tensor multiply: torch's
        own version multiplies fp32 gradients by an fp64 0-d tensor, which
        leaves the multi-tensor fast path for one type-promoting multiply and
        one copy per tensor (52 launches at the VAE's 26 fp32 gradients).  A
        clipped fp32 gradient may differ from torch's by one ulp; an unclipped
        one (coefficient 1) is untouched either way."""
        by_dtype = self._grads_by_dtype()
        if not by_dtype:
            return
        # torch stacks the per-tensor norms of every dtype into one promoted
        # (fp64) vector, which casts each fp32 norm in a launch of its own (26
        # at the VAE); here each dtype's norms are stacked and cast once: the
        # same vector, in the same order
        wide = functools.reduce(torch.promote_types, by_dtype)
        parts = [torch.stack(torch._foreach_norm(grads, 2.0)).to(wide)
                 for grads in by_dtype.values()]
        total = torch.linalg.vector_norm(parts[0] if len(parts) == 1 else torch.cat(parts), 2.0)
        coef = torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0)
        for dt, grads in by_dtype.items():
            torch._foreach_mul_(grads, coef.to(dt))

    def _r_sqrt_sigma(self):
        """The r_sqrt_sigma of this step's compute_loss, taken between the model
        forward and the loss as the reference takes it (fairsoft_train.py:57-69):
        the model's, or with ``args.mpvae_r_draw`` a fresh draw into ``r_drawn``
        (no gradient: the frozen-R backward runs, and the model's own
        r_sqrt_sigma is neither read nor written)."""
        if self.r_draw is None:
            return self.model.r_sqrt_sigma
        import mpvae
        import mpvae_dist
        if mpvae_dist.exchange_active(self.args):
            raise ValueError(f"args.mpvae_r_draw = {self.r_draw!r} with an active args.mpvae_shard "
                             "exchange: every rank would have to draw the same r_sqrt_sigma, "
                             "which the sharded step does not arrange")
        return mpvae.draw_r_sqrt_sigma(self.args, self.r_drawn.device, out=self.r_drawn)

    def _need_capturable_draw(self, who):
        """A captured step's r_sqrt_sigma draw runs on the device too."""
        if self.r_draw == "numpy":
            raise ValueError(f"{who}: args.mpvae_r_draw = 'numpy' draws r_sqrt_sigma on the host "
                             "every step, which a HIP graph cannot contain; 'philox' draws on "
                             "the device")
        if self.r_draw == "philox":
            _need_device_philox(self.args, who, r_draw=True)

    def _objective(self, label, feat):
        """Forward and loss: ``(the tensor to backpropagate, the step's
        outputs)``.  Here compute_loss's total and its 8 outputs; a subclass
        adds its terms (FairTrainStep)."""
        import mpvae
        out = self.model(label, feat)
        res = mpvae.compute_loss(label, *out, self._r_sqrt_sigma(),
                                 step_args(self.args, self.advance_seed))
        return res[0], res

    def _body(self, *batch):
        self.opt.zero_grad(set_to_none=True)
        objective, res = self._objective(*batch)
        objective.backward()
        self._clip()
        self._gated_update()
        return res

    def _gated_update(self):
        """The finite-gradient gate and the optimizer step it gates, after a
        backward: the AMP multi-tensor check (one launch per dtype) sets
        found_inf if any gradient holds a NaN / inf; its unscale by 1.0 leaves
        every value as it is."""
        self.found_inf.zero_()
        for grads in self._grads_by_dtype().values():
            torch._amp_foreach_non_finite_check_and_unscale_(grads, self.found_inf, self._one)
        if self.native_adam:
            # the update, then the step counts, `updates` and the scheduler in
            # one finish launch (counted even when no parameter has a gradient,
            # as the reference's gate passes such a step)
            adam_step(self.opt, self.found_inf, self.updates, self.sched)
        else:
            self.opt.found_inf = self.found_inf
            try:
                self.opt.step()
            finally:
                del self.opt.found_inf
            self.updates.add_(1 - self.found_inf.to(torch.int64))

    def sync_scheduler(self):
        """The device StepLR's learning rates written back into the optimizer's
        param_groups and the scheduler (one host sync); returns them."""
        return None if self.sched is None else self.sched.sync()

    def release_scheduler(self):
        """Sync and give the StepLR back to host control (its step() works
        again); TrainStep then no longer steps it.  A graph captured before
        holds the device lr / epoch and the scheduler step in its Adam
        launches: every captured record is dropped, so later calls run eagerly
        on the host lr until capture() records the step again."""
        if self.sched is None:
            return None
        lrs, self.sched = self.sched.release(), None
        self._drop_graphs()
        return lrs

    def _check_batch(self, batch):
        if len(batch) != len(self.inputs):
            raise TypeError(f"{type(self).__name__} takes ({', '.join(self.inputs)}): "
                            f"{len(self.inputs)} tensors, got {len(batch)}")

    def __call__(self, *batch):
        """One step on the batch (``inputs``), a replay once captured; returns the
        step's outputs (here compute_loss's 8, device tensors)."""
        self._check_batch(batch)
        if self.sched is not None:
            self.sched.adopt_host_lr()
        if self._captured is not None:
            return self._captured.replay(*batch)
        return self._body(*batch)

    step = __call__

    def capture(self, *batch, warmup=2):
        """Record the step in a HIP graph on static copies of the batch; later
        calls copy their batch in and replay.  ``warmup`` eager steps on a side
        stream first (they update the model, as any step does).  The optimizer
        must be built with ``capturable=True`` (its step counter and bias
        corrections then live on the device)."""
        self._check_batch(batch)
        self._need_capturable_draw("capture()")
        _need_capturable(self.opt, "capture()")
        self._captured = _Captured(self._body, [t.clone() for t in batch], warmup,
                                   lambda: self.opt.zero_grad(set_to_none=True))
        return self.graph

    # ---------------------------------------------------------------- epochs
    def _next_batch(self, split, B, **kw):
        """The step's ``inputs`` of the next B rows of the split's order, gathered
        at its cursor."""
        n = len(self.inputs)
        return split.next_batch(B, sens=n > 2, **kw)[:n]

    def run_epoch(self, split, order, batch_size):
        """One epoch of the reference's loop (fairsoft_train.py:47-56) over a
        ``DeviceSplit``, fed on the device: ``order`` (the caller's shuffled
        ``data.train_idx``, numpy or tensor; None: every row in turn) is
        uploaded once, the cursor is put at 0, and every batch of the
        reference's -- ``range(N // B + 1)`` over ``[i B, min((i + 1) B, N))``, the
        empty last one skipped -- is gathered at the cursor by one
        ``mpv_gather_batch`` launch and stepped.  A full batch is a replay of the
        epoch graph when ``capture_epoch`` recorded one for this split and batch
        size (nothing else is enqueued between two replays), and the eager
        gather and step otherwise; the ragged last batch always runs eagerly,
        through the same kernel.  Afterwards the cursor is at ``N - N % B``.
        Returns the number of steps; no host sync (``read_totals()`` /
        ``split.check()`` are the caller's)."""
        B = int(batch_size)
        full, tail = epoch_batches(split.set_order(order), B)
        if self.sched is not None:
            self.sched.adopt_host_lr()
        ep = self._epoch
        if ep is not None and ep.split is split and ep.B == B:
            for _ in range(full):
                ep.replay()
        else:
            for _ in range(full):
                self._body(*self._next_batch(split, B))
        if tail:
            self._body(*self._next_batch(split, tail, advance=False))
        return full + (1 if tail else 0)

    def capture_epoch(self, split, batch_size, warmup=2):
        """Record one full-batch step of ``run_epoch`` in a HIP graph: the gather
        (it reads the split's static order buffer at the device cursor and moves
        the cursor on) followed by the step on the gathered static buffers.
        ``warmup`` eager steps on a side stream first, each on the first
        ``batch_size`` rows of the split's current order (they update the model,
        as capture()'s do); the cursor is back at 0 afterwards.  Needs what
        capture() needs -- ``args.mpvae_noise = "philox"``, a device-tensor
        ``args.mpvae_seed`` and ``torch.optim.Adam(..., fused=True,
        capturable=True)`` -- and a split on the model's GPU whose current order
        holds a full batch.  ``capture()`` and ``__call__`` keep their own graph
        and buffers."""
        B = int(batch_size)
        self._need_capturable_draw("capture_epoch()")
        _need_capturable(self.opt, "capture_epoch()")
        _need_device_philox(self.args, "capture_epoch()")
        if split.device.type != "cuda" or split.device != self.params[0].device:
            raise ValueError("capture_epoch() needs a DeviceSplit on the model's GPU")
        if B < 1 or split.n_order < B:
            raise ValueError(f"capture_epoch() needs a full batch of {B} rows in the split's "
                             f"current order (it holds {split.n_order})")
        bufs = [torch.empty((B, t.shape[1]), dtype=dt, device=split.device)
                for t, dt in split._sources(len(self.inputs) > 2)]
        warming = [True]

        def body(*bufs):
            if warming[0]:
                split.cursor.zero_()
            return self._body(*self._next_batch(split, B, out=bufs))

        def prepare():
            warming[0] = False
            self.opt.zero_grad(set_to_none=True)

        self._epoch = _Captured(body, bufs, warmup, prepare, split, B)
        split.cursor.zero_()
        return self._epoch.graph


class CalibrationStep(TrainStep):
    """The loop body of postprocess_threshold_one_epoch
    (fairsoft_train_postprocess.py:84-175) as one call: the frozen model's
    ``model(label, feat)`` -> ``compute_loss`` (for ``indiv_prob``) ->
    ``mpvae_fair.calibration_loss`` -> ``backward`` -> finite-gradient gate ->
    Adam step on ``threshold_`` -> StepLR, all on the device.

    ``step(label, feat, sensitive_feat)`` returns ``(total, bce, fair,
    cal_prob, contributed)`` as device tensors.  ``total`` is ``fair *
    args.fair_coeff + bce`` when at least one fairness term was added and
    compute_loss's own total otherwise (:163-165); in such a batch the
    threshold's gradient is multiplied by 0 on the device and the update still
    applies (weight decay and the Adam moments move the threshold), as the
    reference's ``optimizer.step()`` on its zeroed gradients did.  ``updates``
    counts the applied steps (succses_updates).  ``args`` is compute_loss's
    namespace plus ``fair_coeff`` and ``learn_logit``; ``args.mode`` is used as
    given ('train': ``n_train_sample`` noise draws, as the reference runs it).
    ``tables`` and ``centroids`` are those of ``calibration_loss``.  The model
    is put in ``eval()`` mode, as the reference does.

    Differences from the reference:
    * no autograd through ``compute_loss`` and the model (they run under
      ``torch.no_grad()``): the threshold's gradient does not depend on it, and
      the reference's own backward through them fed nothing that was read;
    * the reference accumulates model gradients that it never clears or reads;
      the step produces none;
    * r_sqrt_sigma is the model's unless ``args.mpvae_r_draw`` is set; with it
      the reference's ``residue_sigma == "random"`` per-step draw
      (fairsoft_train_postprocess.py:97-106) is reproduced as in TrainStep:
      bit for bit under "numpy", in distribution under "philox".

    The optimizer must be a plain fused ``torch.optim.Adam([threshold_], ...,
    fused=True)`` (it steps in ``adam_step``), with ``capturable=True`` for
    ``capture()``; ``scheduler`` is the reference's StepLR or None.  With Philox
    noise and a device seed nothing waits for the host."""

    inputs = ("label", "feat", "sensitive_feat")

    def __init__(self, model, threshold_, optimizer, args, tables, centroids, scheduler=None):
        if not _native_adam(optimizer):
            raise ValueError("CalibrationStep steps a plain fused Adam on the device: use "
                             "torch.optim.Adam([threshold_], ..., fused=True) with a float lr")
        if not (threshold_.is_leaf and threshold_.requires_grad):
            raise ValueError("threshold_ must be a leaf tensor that requires a gradient")
        super().__init__(model.eval(), optimizer, args, scheduler=scheduler, params=[threshold_])
        self.threshold_, self.tables, self.centroids = threshold_, tables, centroids

    def _body(self, label, feat, sens):
        import mpvae
        import mpvae_fair
        self.opt.zero_grad(set_to_none=True)
        args = step_args(self.args, self.advance_seed)
        with torch.no_grad():
            out = self.model(label, feat)
            res = mpvae.compute_loss(label, *out, self._r_sqrt_sigma(), args)
        bce, fair, cal_prob, active, contributed = mpvae_fair.calibration_loss(
            res[6], self.threshold_, label, sens, self.centroids, self.tables, args.learn_logit)
        cal_total = fair * args.fair_coeff + bce
        total = torch.where(active, cal_total.detach(), res[0].to(cal_total.dtype))
        (cal_total * active.to(cal_total.dtype)).backward()
        self._gated_update()  # no clip, as the reference
        return total, bce.detach(), fair.detach(), cal_prob, contributed


FairStepOut = collections.namedtuple(
    "FairStepOut", ["total", "nll", "nll_x", "c", "c_x", "kl", "indiv_prob", "indiv_prob_label",
                    "fairloss", "contributed", "metrics"])
# the running sums FairTrainStep keeps (the reference's smooth_* accumulators)
SUM_KEYS = ["total", "nll", "nll_x", "c", "c_x", "kl", "fairloss", "maF1", "miF1"]


class _Totals:
    """Device accumulators of one loop (training or validation): the fp64 sums
    of SUM_KEYS, the step count and the int64 contributed count."""

    def __init__(self, dev):
        import mpvae_fair
        self.sums = torch.zeros(len(SUM_KEYS), dtype=torch.float64, device=dev)
        self.counts = torch.zeros(2, dtype=torch.int64, device=dev)  # steps, contributed
        self._one = torch.ones((), dtype=torch.int64, device=dev)
        self._f1 = torch.tensor([mpvae_fair.METRIC_KEYS.index("maF1"),
                                 mpvae_fair.METRIC_KEYS.index("miF1")], device=dev)

    def add(self, out):
        losses = torch.stack([t.detach() for t in out[:6]]).to(torch.float64)
        self.sums += torch.cat([losses, out.fairloss.to(torch.float64).reshape(1),
                                out.metrics[self._f1]])
        self.counts += torch.stack([self._one, out.contributed.to(torch.int64)])

    def zero_(self):
        self.sums.zero_()
        self.counts.zero_()


class FairTrainStep(TrainStep):
    """The loop body of train_mpvae_softfair_one_epoch with ``penalize_unfair``
    (fairsoft_train.py:47-162) as one call: TrainStep's step with the fairness
    regulariser in the objective -- ``model(label, feat)`` -> ``compute_loss``
    -> ``mpvae_fair.fairness_penalty(fused=True)`` -> backward of total +
    fairloss -> clip -> finite-gradient gate -> Adam -> StepLR -> the per-step
    train metrics (after the update, :149-152) -> the running sums, all on the
    device.

    ``step(label, feat, sensitive_feat)`` returns a ``FairStepOut``:
    compute_loss's eight outputs, ``fairloss``, ``contributed`` (int32) and
    ``metrics`` ((8,) fp64 in ``mpvae_fair.METRIC_KEYS`` order).  ``total`` is
    fp32 and equals float32(float64(compute_loss's total) + fairloss), as the
    reference's in-place ``total_loss += fairloss`` (:137); the backward runs
    on the unrounded sum.  ``tables`` are the ``LabelDistanceTable``s of the
    target fair labels; ``[]`` is the reference's ``penalize_unfair=0``.
    ``args`` is TrainStep's namespace plus ``fair_coeff`` and
    ``fairness_loss_norm``; ``max_groups`` as in ``fairness_penalty`` -- a
    batch with more sensitive patterns than the bound makes the penalty NaN
    and the gate skips the update.

    In place of the reference's eight ``.item()`` calls per step and its
    ``contributed_reg_fair_sample`` (:154-173) the step adds to device sums
    (SUM_KEYS, a step count, ``contributed``) on every step, whether or not the
    gate skipped the update; ``read_totals()`` is the only host sync.
    ``validate()`` is the body of validate_mpvae_softfair with sums of its own.

    Differences from the reference:
    * r_sqrt_sigma is the model's unless ``args.mpvae_r_draw`` is set; with it
      the ``residue_sigma == "random"`` per-step draw (:60-69; ``validate``:
      :247-256) is reproduced as in TrainStep: bit for bit under "numpy", in
      distribution under "philox";
    * ``fairloss`` is always a tensor, zero when no term is active (the
      reference's Python float 0., which it does not add);
    * the penalty arithmetic is fp64 whatever the distance values are
      (mpvae_fair's module docstring).

    With Philox noise and a device seed nothing in ``step`` waits for the
    host; ``capture()`` records it, sums included, in one HIP graph."""

    # fairness_penalty's flag; False (set on an instance before capture) is the
    # unfused penalty, bit for bit the same step: tools/bench_fair_step.py's yardstick
    fused = True
    inputs = ("label", "feat", "sensitive_feat")

    def __init__(self, model, optimizer, args, tables, max_groups=None, scheduler=None):
        super().__init__(model, optimizer, args, scheduler=scheduler)
        self.tables, self.max_groups = list(tables), max_groups
        dev = self.params[0].device
        self.totals, self.valid_totals = _Totals(dev), _Totals(dev)

    def _forward(self, label, feat, sens, norm):
        """Forward, loss, penalty: (the unrounded total + fairloss, a
        FairStepOut without its metrics)."""
        import mpvae
        import mpvae_fair
        out = self.model(label, feat)
        res = mpvae.compute_loss(label, *out, self._r_sqrt_sigma(),
                                 step_args(self.args, self.advance_seed))
        fair, contributed = mpvae_fair.fairness_penalty(
            res[7], res[6], label, sens, self.tables, norm, self.args.fair_coeff,
            max_groups=self.max_groups, fused=self.fused)
        objective = res[0].to(torch.float64) + fair
        if self.tables and self.max_groups is not None:
            # a batch with more patterns than the bound: the penalty is NaN but
            # its gradients are zero; scaling by 1 (NaN in that case) hands
            # the gate NaN gradients, and changes no bit otherwise
            nan_or_zero = fair.detach() - fair.detach()
            objective = objective * (1.0 + nan_or_zero)
        return objective, FairStepOut(objective.detach().float(), *res[1:], fair.detach(),
                                      contributed, None)

    def _with_metrics(self, out, label, totals):
        import mpvae_fair
        metrics = mpvae_fair._train_metrics(out.indiv_prob.detach().contiguous().float(),
                                            label.contiguous().float(), 0.5)
        out = out._replace(metrics=metrics)
        totals.add(out)
        return out

    def _objective(self, label, feat, sens):
        return self._forward(label, feat, sens, self.args.fairness_loss_norm)

    def _body(self, label, feat, sens):
        return self._with_metrics(super()._body(label, feat, sens), label, self.totals)

    def validate(self, label, feat, sensitive_feat):
        """The loop body of validate_mpvae_softfair (fairsoft_train.py:234-331)
        on one batch: ``model.eval()`` and ``no_grad``, the same forward, loss,
        penalty and metrics, no backward and no update; a ``FairStepOut``,
        added to the validation sums.  The reference's validation penalty
        always squares (:305-308), whatever ``fairness_loss_norm`` says, so
        the norm here is "l2".  The model's train / eval mode is restored.
        Runs eagerly: it is not part of a captured graph."""
        with _eval_mode(self.model):
            _, out = self._forward(label, feat, sensitive_feat, "l2")
            return self._with_metrics(out, label, self.valid_totals)

    def validate_epoch(self, split, order, batch_size):
        """validate_mpvae_softfair's loop (fairsoft_train.py:233-331) over a
        ``DeviceSplit``: ``validate()`` on every batch of ``order``
        (``data.valid_idx``; run_epoch's batch rule), each gathered on the device
        at the split's cursor; eager.  The sums go to ``valid_totals``; returns
        the number of batches, no host sync."""
        B = int(batch_size)
        full, tail = epoch_batches(split.set_order(order), B)
        for _ in range(full):
            self.validate(*split.next_batch(B))
        if tail:
            self.validate(*split.next_batch(tail, advance=False))
        return full + (1 if tail else 0)

    def read_totals(self, reset=True):
        """The running sums as Python numbers, with one host sync: the SUM_KEYS
        sums (divide by ``steps`` for the reference's running_postfix),
        ``steps``, ``contributed`` and ``updates`` of the training steps, and
        under ``"valid"`` the same (without ``updates``) of the ``validate``
        calls.  ``reset`` zeroes the sums, step counts and contributed counts
        (``updates`` keeps counting, as TrainStep's)."""
        t, v = self.totals, self.valid_totals
        vals = torch.cat([t.sums, v.sums,
                          torch.cat([t.counts, v.counts, self.updates.reshape(1)])
                          .to(torch.float64)]).tolist()
        n = len(SUM_KEYS)
        out = dict(zip(SUM_KEYS, vals[:n]))
        out["valid"] = dict(zip(SUM_KEYS, vals[n:2 * n]))
        counts = [int(x) for x in vals[2 * n:]]
        out["steps"], out["contributed"], out["updates"] = counts[0], counts[1], counts[4]
        out["valid"]["steps"], out["valid"]["contributed"] = counts[2], counts[3]
        if reset:
            t.zero_()
            v.zero_()
        return out


EvalOut = collections.namedtuple("EvalOut", ["indiv_prob", "scores"])


class EvalPass(_Capturing):
    """fairsoft_evaluate.evaluate_mpvae's loop and scoring (:40-123) over one
    split as one call, on the model's device: the model's ``indiv_prob`` of
    every batch written into one preallocated (N, L) fp32 buffer (what
    fairsoft_prediction_extract's extract_prediction_mpvae collects), then
    ``mpvae_fair.split_scores`` on that buffer.

    ``run(labels, feats, sensitive_feat=None, weight_labels=None)`` takes the
    split's rows as tensors on the model's device and returns an ``EvalOut``:
    ``indiv_prob`` (N, L) and ``scores`` (a ``mpvae_fair.SplitScores``, device
    tensors).  ``read(out)`` is the only host sync: the reference's dict
    ``{'fair_mean_diff', 'miF1', 'maF1'}`` as Python floats, ``fair_mean_diff``
    None without ``tables`` (the reference's ``eval_fairness=False``).

    The batches are the reference's, ``range(N // B + 1)`` over rows ``[i B,
    min((i + 1) B, N))``; an empty last batch (N a multiple of B) is skipped:
    it draws nothing and adds no row.  ``label_free=False`` (default): a batch
    is ``model(label, feat)`` and ``mpvae.predict_proba(feat_out,
    model.r_sqrt_sigma, args)`` -- the reference's RNG stream and the bits of
    its ``compute_loss(...)[6]``: both encoders draw their reparameterisation
    noise, and ``torch_cpu`` probit noise comes from the CPU generator.
    ``label_free=True``: ``model.predict_proba(feat, args)``, the feature
    branch alone (another, equally distributed noise stream).

    ``args`` is read as ``predict_proba`` reads it (mode -> n_train_sample /
    n_test_sample, z_dim, mpvae_noise, mpvae_seed, mpvae_gemm, mpvae_shard).
    With a device-tensor ``args.mpvae_seed`` every batch advances the key
    (``mpvae_seed_advance``, as TrainStep does), so every batch draws fresh
    noise.  ``tables``, ``centroids``, ``weight_labels`` and ``slices`` are
    those of ``split_scores`` -- see there for the reference's choice of the
    rows its weights are looked up by.  ``definitions`` (instead of ``tables``:
    D lists of T weight sources each, as ``mpvae_fair.split_scores_defs`` takes
    them) scores the one (N, L) buffer under all D definitions -- the sweep of
    fairsoft_metric.evaluate_models_over_label_distances from one pass over
    the split; ``read`` then returns ``fair_mean_diff`` as a list of D floats,
    still with one host sync.  The model is put in ``eval()`` mode
    under ``no_grad`` and its previous mode is restored.

    With Philox noise and a device seed nothing in ``run`` waits for the host,
    and ``capture(labels, feats)`` records the full-batch body in one HIP
    graph on static buffers: each full batch is then a copy in, a replay and a
    device-to-device copy of the result into its rows; the ragged last batch
    and the scoring run eagerly.  CPU tensors run the model through
    libmpvae_host.so and the scoring in torch (``split_scores``)."""

    def __init__(self, model, args, batch_size, tables=None, centroids=None, label_free=False,
                 slices=None, definitions=None):
        if int(batch_size) < 1:
            raise ValueError(f"batch_size must be >= 1 (got {batch_size})")
        if tables is not None and definitions is not None:
            raise ValueError("EvalPass takes tables or definitions, not both")
        if (tables is not None or definitions is not None) and centroids is None:
            raise ValueError("EvalPass with tables needs the dataset's centroids")
        self.model, self.args, self.batch_size = model, args, int(batch_size)
        self.tables = None if tables is None else list(tables)
        self.definitions = None if definitions is None else [list(d) for d in definitions]
        self.centroids, self.label_free, self.slices = centroids, bool(label_free), slices

    def _batch(self, label, feat):
        """indiv_prob (B, L) of one batch."""
        import mpvae
        args = step_args(self.args)
        if self.label_free:
            return self.model.predict_proba(feat, args)
        out = self.model(label, feat)
        return mpvae.predict_proba(out[3], self.model.r_sqrt_sigma, args)

    def run(self, labels, feats, sensitive_feat=None, weight_labels=None):
        import mpvae_fair
        if (self.tables is not None or self.definitions is not None) and sensitive_feat is None:
            raise ValueError("EvalPass with tables needs the split's sensitive_feat")
        N, L = labels.shape
        B = self.batch_size
        full, tail = epoch_batches(N, B)
        with _eval_mode(self.model):
            buf = torch.empty((N, L), dtype=torch.float32, device=feats.device)
            for i in range(full + bool(tail)):
                rows = slice(i * B, min((i + 1) * B, N))
                if self._captured is not None and i < full:
                    prob = self._captured.replay(labels[rows], feats[rows])
                else:
                    prob = self._batch(labels[rows].float(), feats[rows])
                buf[rows].copy_(prob)
            if self.definitions is not None:
                scores = mpvae_fair.split_scores_defs(buf, labels, sensitive_feat, self.centroids,
                                                      self.definitions, weight_labels, self.slices)
            else:
                scores = mpvae_fair.split_scores(buf, labels, sensitive_feat, self.centroids,
                                                 self.tables, weight_labels, self.slices)
        return EvalOut(buf, scores)

    def run_split(self, split, order=None, weight_labels=None):
        """``run`` on the rows ``order`` of a ``DeviceSplit`` (None: all of them, in
        place): one ``mpv_gather_batch`` launch collects ``labels[order]`` (as
        fp32), ``feats[order]`` and ``sensitive_feat[order]`` on the device -- what
        a caller of ``run`` materialises on the host for a subset -- and ``run``
        takes them.  ``weight_labels`` is ``run``'s, row-aligned with ``order``."""
        if order is None and split.feats.dtype == torch.float32:
            labels, feats, sens = split.labels, split.feats, split.sens
        else:
            n = split.n_rows if order is None else len(order)
            labels, feats, sens = split.gather(order, 0, n)
        return self.run(labels, feats, sens, weight_labels)

    def capture(self, labels, feats, warmup=2):
        """Record the body of a full batch in a HIP graph on static copies of the
        first ``batch_size`` rows of (labels, feats).  ``warmup`` eager batches
        on a side stream first (they advance the device seed, as any batch
        does).  Needs ``args.mpvae_noise = "philox"`` and a device-tensor
        ``args.mpvae_seed``, TrainStep.capture's conditions: any other noise
        source is drawn on the host."""
        B = self.batch_size
        _need_device_philox(self.args, "capture()")
        if labels.shape[0] < B:
            raise ValueError(f"capture() needs a full batch of {B} rows (got {labels.shape[0]})")
        with _eval_mode(self.model):
            self._captured = _Captured(self._batch, [labels[:B].float().clone(), feats[:B].clone()],
                                       warmup)
        return self.graph

    @staticmethod
    def read(out):
        """The reference's result dict as Python floats, with one host sync."""
        s = out.scores
        if s.fair_mean_diff is not None and s.fair_mean_diff.dim() == 1:  # definitions
            vals = torch.cat([torch.stack([s.miF1, s.maF1]), s.fair_mean_diff]).cpu().tolist()
            return {"fair_mean_diff": vals[2:], "miF1": vals[0], "maF1": vals[1]}
        vals = step_scalars(miF1=s.miF1, maF1=s.maF1,
                            **({} if s.fair_mean_diff is None
                               else {"fair_mean_diff": s.fair_mean_diff}))
        return {"fair_mean_diff": vals.get("fair_mean_diff"), "miF1": vals["miF1"],
                "maF1": vals["maF1"]}
