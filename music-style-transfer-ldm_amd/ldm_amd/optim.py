"""Optimiser step of the train path on the HIP kernels.

``Adam`` / ``AdamW`` are torch.optim.Optimizer subclasses (same param_groups, state keys 'step',
'exp_avg', 'exp_avg_sq', state_dict format, so ReduceLROnPlateau and checkpoints work unchanged) whose
step() is ONE multi-tensor launch per param group (ldm_adam_step).  ``GradScaler`` mirrors
torch.amp.GradScaler's API and semantics (scale / unscale_ / step / update, backoff and growth) with
the unscale + inf check and the scale update as device kernels (ldm_unscale_check, ldm_update_scale).

Not in the reference, off by default: gradient-norm clipping (clip_grad_norm_, grad_norm_coef,
GradScaler.unscale_(optimizer, max_norm=): the norm is formed by the unscale launch, the coefficient multiplies
the gradients inside the Adam launch) and an EMA of the parameters updated inside the Adam launch (Adam.attach_ema).

Reference call sites: torch.optim.Adam + torch.amp.GradScaler in LDMTrainer (train.py:156-157,
:189-201); torch.optim.AdamW in train_autoencoder (train.py:44).
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from .ops import require_device, stream_handle

CHUNK = 1 << 12   # elements per workgroup-chunk of the multi-tensor kernels (4 float4 per thread)


class _SlotTable:
    """Device table of ldm_tensor_slot {param, grad, exp_avg, exp_avg_sq, numel} + chunk map.

    Tables are cached by the tensors' addresses (the same parameters, gradients and state give the same
    table every step).  The chunk map depends only on the sizes and is uploaded once per size list; the
    slot rows (whose gradient addresses move when zero_grad() drops the grads) go up with an asynchronous
    copy from pinned memory, so building a table never synchronises the host with the device.

    Inside a graph capture a table is neither allocated nor filled on the device.  Its rows go to a pinned
    host buffer and its device rows are a buffer reserved BEFORE the capture (reserve_capture_buffers), and
    fill_captured() uploads them after the capture has ended.  Why (round 6): a device buffer
    allocated while capturing comes from the graph's private pool and may be a block that a temporary of the
    SAME capture used and freed earlier (the forward / backward scratch).  Every replay then rewrites that
    block before the optimizer reads it, so a table written there once, outside the graph's own stream order,
    is garbage by the time unscale_check_kernel indexes slots[chunk_tensor[i]]: round 5's side-stream
    upload variant faulted on exactly that (HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION in unscale_check_kernel
    at the first replay).  A chunk map for a new size list would be a captured copy from a pageable numpy
    buffer that is freed after the capture; both are refused while capturing."""

    _cache = {}
    _maps = {}
    _captured = []
    _reserve = []   # (pinned host int64 buffer, device int64 buffer) pairs, allocated outside any capture

    def __new__(cls, params, grads, m, v):
        key = tuple((p.data_ptr(), g.data_ptr(), 0 if a is None else a.data_ptr(), 0 if b is None else b.data_ptr(),
                     p.numel()) for p, g, a, b in zip(params, grads, m, v))
        dev = params[0].device
        hit = cls._cache.get((dev, key))
        if hit is not None:
            return hit
        capturing = torch.cuda.is_current_stream_capturing()
        self = super().__new__(cls)
        rows = np.array(key, dtype=np.int64).reshape(-1, 5)
        numels = tuple(int(k[4]) for k in key)
        mp = cls._maps.get((dev, numels))
        if mp is None:
            if capturing:
                raise RuntimeError("ldm_amd.optim: a slot table's chunk map is built outside a graph capture only "
                                   "(run the step eagerly once before capturing it)")
            nch = (rows[:, 4] + CHUNK - 1) // CHUNK
            ct = np.repeat(np.arange(len(rows), dtype=np.int32), nch)
            first = np.repeat(np.cumsum(nch) - nch, nch)
            cs = (np.arange(int(nch.sum()), dtype=np.int64) - first) * CHUNK
            mp = (torch.from_numpy(ct).to(dev), torch.from_numpy(cs).to(dev), int(len(ct)))
            cls._maps[(dev, numels)] = mp
        self.chunk_tensor, self.chunk_start, self.nchunks = mp
        if capturing:
            res = cls._reserve[-1] if cls._reserve else None
            if res is None or res[0].numel() < rows.size or res[1].device != dev:
                raise RuntimeError("ldm_amd.optim: slot tables are built and filled outside a graph capture only; "
                                   "call reserve_capture_buffers(device=...) before capturing an optimizer step")
            host, dbuf = cls._reserve.pop()
            host = host[:rows.size].view(rows.shape)
            host.copy_(torch.from_numpy(rows))
            self._host = host
            self.slots = dbuf[:rows.size].view(rows.shape)   # reserved before the capture: never a graph-pool block
            self._filled = False
            cls._captured.append(self)
            self._captured_key = (dev, key)
        else:
            self.slots = torch.empty(rows.shape, dtype=torch.int64, device=dev)
            host = torch.from_numpy(rows).pin_memory()    # caching host allocator: reused once the copy ran
            self.slots.copy_(host, non_blocking=True)
        self.key = key
        if len(cls._cache) > 64:
            cls._cache.clear()
        cls._cache[(dev, key)] = self
        return self

    def __init__(self, *args):
        pass

    def args(self):
        """The five leading arguments of every multi-tensor entry: slots, chunk map, chunk count, chunk length."""
        return (self.slots.data_ptr(), self.chunk_tensor.data_ptr(), self.chunk_start.data_ptr(), self.nchunks, CHUNK)


def reserve_capture_buffers(n=4, words=1 << 14, device="cuda"):
    """Pinned host buffers and device buffers for the slot tables built while a step is being captured into
    a hipGraph (one pair per optimizer / unscale table in the step); call before torch.cuda.graph, outside
    the capture.  Returns the list that will hold the tables the capture builds: pass it to fill_captured()
    once the capture has ended (before the first replay), and to release_captured() when the graph is
    dropped."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("ldm_amd.optim.reserve_capture_buffers: call it before the capture starts")
    dev = torch.device(device)
    _SlotTable._reserve = [r for r in _SlotTable._reserve if r[1].device == dev]
    while len(_SlotTable._reserve) < n:
        _SlotTable._reserve.append((torch.empty(words, dtype=torch.int64, pin_memory=True),
                                    torch.empty(words, dtype=torch.int64, device=dev)))
    _SlotTable._captured = []
    return _SlotTable._captured


def fill_captured(tables):
    """Upload the rows of the slot tables a capture built (on the current stream, outside the capture; the
    graph's replays on this stream come after the copies).  Idempotent."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("ldm_amd.optim.fill_captured: the tables are filled after the capture has ended")
    for tab in tables:
        if not tab._filled:
            tab.slots.copy_(tab._host, non_blocking=True)
            tab._filled = True


def release_captured(tables):
    """Forget the slot tables (and their pinned host rows) of a captured graph that is being replaced: they
    leave the table cache, so the pinned buffers and device tables die with the graph."""
    if not tables:
        return
    for tab in tables:
        k = getattr(tab, "_captured_key", None)
        if k is not None and _SlotTable._cache.get(k) is tab:
            del _SlotTable._cache[k]
    tables.clear()
    _SlotTable._reserve.clear()


def scale_tensors_(tensors, factor):
    """t *= factor for every (contiguous fp32 device) tensor, one multi-tensor launch; returns a device
    int32 [1] flag, nonzero if any result is non-finite."""
    tensors = [t for t in tensors if t.numel()]
    if not tensors:
        return False
    require_device(*tensors, what="scale_tensors_")
    tab = _SlotTable(tensors, tensors, [None] * len(tensors), [None] * len(tensors))
    f = torch.full((1,), float(factor), dtype=torch.float32, device=tensors[0].device)
    bad = torch.zeros((1,), dtype=torch.int32, device=tensors[0].device)
    L.call("ldm_unscale_check", *tab.args(), f.data_ptr(), bad.data_ptr(), stream_handle())
    return bad


class _NormBuffers:
    """Device buffers of one gradient-norm pass: per-chunk fp64 partial sums, the [norm, coef] fp32 pair the
    finalize writes, and an inf/nan flag.  Like a slot table they are read by captured launches at every replay,
    so they are allocated outside any capture only (a buffer allocated while capturing comes from the graph's
    private pool and may be a block the same capture's scratch rewrites: see _SlotTable) and reused by every
    step.  Sized by the chunk count: a gradient set of other sizes gets another one, outside capture."""

    def __init__(self, dev, nchunks):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ldm_amd.optim: the gradient-norm buffers are allocated outside a graph capture only "
                               "(run the clipped step eagerly once before capturing it)")
        self.nchunks = int(nchunks)
        self.partials = torch.zeros(max(1, self.nchunks), dtype=torch.float64, device=dev)
        self.pair = torch.zeros(2, dtype=torch.float32, device=dev)
        self.found_inf = torch.zeros(1, dtype=torch.int32, device=dev)

    @classmethod
    def get(cls, cache, dev, nchunks):
        buf = cache.get((dev, nchunks))
        if buf is None:
            if len(cache) > 8:
                cache.clear()
            buf = cache[(dev, nchunks)] = cls(dev, nchunks)
        return buf


def _norm_pass(groups, max_norm, inv_scale, cache, found_inf=None):
    """ldm_unscale_check_norm over every list of parameters in `groups` (one table each), then one finalize
    over the concatenated partials: one global norm.  Returns (buffers, tables)."""
    groups = [ps for ps in groups if ps]
    tabs = []
    for ps in groups:
        _check_params(ps)
        tabs.append(_SlotTable(ps, [p.grad for p in ps], [None] * len(ps), [None] * len(ps)))
    dev = groups[0][0].device
    buf = _NormBuffers.get(cache, dev, sum(t.nchunks for t in tabs))
    flag = buf.found_inf if found_inf is None else found_inf
    off = 0
    for tab in tabs:
        L.call("ldm_unscale_check_norm", *tab.args(), None if inv_scale is None else inv_scale.data_ptr(),
               flag.data_ptr(), buf.partials.data_ptr() + 8 * off, stream_handle())
        off += tab.nchunks
    L.call("ldm_grad_norm_finalize", buf.partials.data_ptr(), buf.nchunks, float(max_norm), buf.pair.data_ptr(),
           stream_handle())
    return buf, tabs


_norm_cache = {}


def _grad_params(parameters):
    if torch.is_tensor(parameters):
        parameters = [parameters]
    return [p for p in parameters if p.grad is not None and p.numel()]


def grad_norm_coef(parameters, max_norm):
    """The global 2-norm of the parameters' gradients and torch.nn.utils.clip_grad_norm_'s coefficient
    min(1, max_norm / (norm + 1e-6)) as a device fp32 pair [norm, coef]; the gradients are left as they are.
    One norm launch plus a one-block finalize, fixed-order fp64 sums, no host synchronisation.  max_norm <= 0:
    norm only (coef = 1).  The pair is a buffer that the next call with gradients of the same sizes rewrites:
    pass pair[1:2] to Adam.step(grad_mul=...) for a clipped step that does not rewrite the gradients."""
    ps = _grad_params(parameters)
    if not ps:
        raise ValueError("ldm_amd.optim.grad_norm_coef: no parameter has a gradient")
    buf, tabs = _norm_pass([ps], max_norm, None, _norm_cache)
    buf.tabs = tabs   # keep alive until the launches ran
    return buf.pair


def clip_grad_norm_(parameters, max_norm):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type 2) on the device: the norm pass, the
    finalize, then grad *= coef in one ldm_unscale_check launch with the device coefficient as its factor.
    Returns the norm (before clipping) as a 0-d device tensor.  No host synchronisation; deterministic."""
    ps = _grad_params(parameters)
    if not ps:
        raise ValueError("ldm_amd.optim.clip_grad_norm_: no parameter has a gradient")
    buf, tabs = _norm_pass([ps], max_norm, None, _norm_cache)
    tab = tabs[0]
    L.call("ldm_unscale_check", *tab.args(), buf.pair.data_ptr() + 4, buf.found_inf.data_ptr(), stream_handle())
    buf.tabs = tabs
    return buf.pair[0].clone()


def ema_update_(ema_tensors, sources, decay, found_inf=None):
    """e <- e + (1 - decay) (src - e) for every pair, one multi-tensor launch (ldm_ema_update): the EMA update of
    Adam.attach_ema on its own, for callers that step with another optimizer."""
    _check_decay(decay)
    pairs = [(e, s) for e, s in zip(ema_tensors, sources) if e.numel()]
    if not pairs:
        return
    es, ss = [e for e, _ in pairs], [s for _, s in pairs]
    require_device(*es, *ss, what="ema_update_")
    tab = _SlotTable(es, ss, [None] * len(es), [None] * len(es))
    L.call("ldm_ema_update", *tab.args(), float(decay), None if found_inf is None else found_inf.data_ptr(),
           stream_handle())
    return tab


def _check_decay(decay):
    if not isinstance(decay, (int, float)) or isinstance(decay, bool) or not 0.0 <= decay < 1.0:
        raise ValueError(f"Invalid EMA decay: {decay} (0 <= decay < 1)")


def ema_state_dict(module, optimizer):
    """module.state_dict() with every parameter that `optimizer` keeps an EMA of replaced by that EMA; buffers
    and the other parameters are copied as they are."""
    sd = {k: v.detach().clone() for k, v in module.state_dict().items()}
    for name, p in module.named_parameters():
        e = optimizer.state.get(p, {}).get("ema")
        if e is not None and name in sd:
            sd[name] = e.detach().clone()
    return sd


def _check_params(params):
    for p in params:
        require_device(p, what="ldm_amd.optim")
        if not p.is_contiguous() or (p.grad is not None and not p.grad.is_contiguous()):
            raise RuntimeError("ldm_amd.optim: parameters and gradients must be contiguous")
        if p.grad is not None and p.grad.is_sparse:
            raise RuntimeError("ldm_amd.optim: sparse gradients are not supported")


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam (amsgrad=False, maximize=False, no capturable/differentiable) on one fused
    multi-tensor kernel per param group."""

    _decoupled = 0

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False,
                 capturable=False):
        if amsgrad:
            raise NotImplementedError("ldm_amd.optim.Adam: amsgrad is not supported")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False))
        self._tables = {}
        # capturable (torch.optim.Adam(capturable=True)): the step count is a device tensor advanced by the
        # kernel itself, so step() never reads it on the host and can be captured into a hipGraph
        self.capturable = bool(capturable)
        self.ema_decay = None     # attach_ema
        self._ema_ptrs = {}

    @torch.no_grad()
    def attach_ema(self, decay):
        """Keep an exponential moving average of every parameter, e <- e + (1 - decay) (p - e), updated inside the
        step's own launch from the parameter value the step just formed (skipped with the step on inf/nan).  The
        EMA tensors start at the parameters and live in state[p]["ema"], so state_dict / load_state_dict carry
        them."""
        _check_decay(decay)
        if self.ema_decay is not None:
            raise RuntimeError("ldm_amd.optim: attach_ema was already called on this optimizer")
        self.ema_decay = float(decay)
        self._init_ema()

    def _init_ema(self):
        """An EMA tensor for every parameter that has none (initialised to the parameter) and the device pointer
        arrays of the groups' full parameter lists (built here, outside any capture)."""
        self._ema_ptrs.clear()
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state[p]
                if "ema" not in st:
                    st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
            ps = list(group["params"])
            if ps and ps[0].device.type == "cuda":
                self._ema_pointer_array(ps)

    def ema_tensors(self):
        """[(parameter, its EMA tensor)] over all groups, in group order."""
        return [(p, self.state[p]["ema"]) for g in self.param_groups for p in g["params"] if "ema" in self.state[p]]

    def _ema_pointer_array(self, ps):
        """Device int64 array of the EMA tensors' addresses, one per slot of the table over `ps`.  Read by
        captured launches at every replay, so built and filled outside any capture only (see _SlotTable)."""
        es = [self.state[p]["ema"] for p in ps]
        key = tuple(e.data_ptr() for e in es)
        hit = self._ema_ptrs.get(key)
        if hit is not None:
            return hit[0]
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ldm_amd.optim: the EMA pointer array is built outside a graph capture only "
                               "(attach_ema builds it for a group's full parameter list; run the step eagerly "
                               "once before capturing a step over another set)")
        for p, e in zip(ps, es):
            require_device(e, what="ldm_amd.optim EMA")
            if not e.is_contiguous() or e.numel() != p.numel() or e.dtype != torch.float32:
                raise RuntimeError("ldm_amd.optim: an EMA tensor must be contiguous fp32 of its parameter's size")
        host = torch.tensor(key, dtype=torch.int64).pin_memory()
        arr = torch.empty(len(key), dtype=torch.int64, device=ps[0].device)
        arr.copy_(host, non_blocking=True)
        if len(self._ema_ptrs) > 16:
            self._ema_ptrs.clear()
        self._ema_ptrs[key] = (arr, host)
        return arr

    def _ext(self, ps, grad_mul):
        """The ldm_adam_ext record of a launch over `ps`, or None when neither option is set."""
        if grad_mul is None and self.ema_decay is None:
            return None
        ext = L.AdamExt(None, None, 0.0)
        if grad_mul is not None:
            require_device(grad_mul, what="ldm_amd.optim grad_mul")
            if grad_mul.dtype != torch.float32 or grad_mul.numel() != 1:
                raise RuntimeError("ldm_amd.optim: grad_mul is a device fp32 scalar")
            ext.grad_mul = grad_mul.data_ptr()
        if self.ema_decay is not None:
            ext.ema = self._ema_pointer_array(ps).data_ptr()
            ext.ema_decay = self.ema_decay
        return ext

    def _launch(self, tab, ps, group, found_inf, grad_mul, step, scalars=None):
        """The Adam launch over `tab`, the table of `ps`.  step: the host step count, or with `scalars` (the
        capturable form) the device step count's address.  The plain entry unless _ext gives a record."""
        beta1, beta2 = group["betas"]
        ext = self._ext(ps, grad_mul)
        name = "ldm_adam_step" + ("" if scalars is None else "_dev") + ("" if ext is None else "_ext")
        tail = () if scalars is None else (scalars.data_ptr(),)
        if ext is not None:
            tail += (ctypes.byref(ext),)
        L.call(name, *tab.args(), float(group["lr"]), float(beta1), float(beta2), float(group["eps"]),
               float(group["weight_decay"]), self._decoupled, step,
               None if found_inf is None else found_inf.data_ptr(), *tail, stream_handle())

    @torch.no_grad()
    def step(self, closure=None, found_inf=None, grad_mul=None):
        """One Adam update.  found_inf (device int32 [1], optional): skip on the device if set.  grad_mul (device
        fp32 scalar, optional): every gradient is multiplied by it as it is loaded (a clip coefficient);
        .grad itself is not rewritten."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            _check_params(params)
            if self.capturable:
                self._step_capturable(gi, group, params, found_inf, grad_mul)
                continue
            if "_ldm_step" in group:
                # leaving the capturable form: every param gets its own host step count again (the shared
                # device count must not be advanced once per param by the eager loop below)
                self._unshare_steps(group)
            # group the params by their step count (all equal unless params were added later)
            by_step = {}
            for p in params:
                st = self.state[p]
                if "step" not in st:     # (an attached EMA is in the state before the first step)
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                by_step.setdefault(int(st["step"].item()), []).append(p)
            for step, ps in by_step.items():
                grads = [p.grad for p in ps]
                tab = _SlotTable(ps, grads, [self.state[p]["exp_avg"] for p in ps],
                                 [self.state[p]["exp_avg_sq"] for p in ps])
                self._launch(tab, ps, group, found_inf, grad_mul, step)
                # the tables are read by the kernel asynchronously: keep them alive until it ran
                self._tables[(gi, step)] = tab
                # the kernel wrote the parameters through raw pointers: move their autograd versions the
                # way an in-place torch update does, so that version-keyed caches (packed conv weights,
                # ops.packed_weight; the UNet engine's step weights) re-pack them
                for p in ps:
                    torch.autograd.graph.increment_version(p)
        return loss


    _GROUP_PRIVATE = ("_ldm_step", "_ldm_scalars", "_ldm_tabs")

    def _unshare_steps(self, group):
        gstep = group.pop("_ldm_step")
        group.pop("_ldm_scalars", None)
        n = float(gstep)
        for p in group["params"]:
            st = self.state.get(p)
            if st and st.get("step") is gstep:
                st["step"] = torch.tensor(n)

    def state_dict(self):
        """torch.optim state_dict, with every param's 'step' a CPU tensor of its own (the capturable form
        shares one device count per group) and without this class's private per-group device tensors, so
        that it loads into torch.optim.Adam or into an eager / capturable instance of this class alike."""
        sd = super().state_dict()
        for g in sd["param_groups"]:
            for k in self._GROUP_PRIVATE:
                g.pop(k, None)
        state = {}
        for idx, st in sd["state"].items():
            st = dict(st)
            if "step" in st and torch.is_tensor(st["step"]):
                st["step"] = torch.tensor(float(st["step"]))
            state[idx] = st
        sd["state"] = state
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            for k in self._GROUP_PRIVATE:
                g.pop(k, None)
            for p in g["params"]:
                st = self.state.get(p)
                if st and "step" in st and torch.is_tensor(st["step"]):
                    st["step"] = torch.tensor(float(st["step"]))
        self._tables.clear()
        if self.ema_decay is not None:
            # the loaded EMA tensors are new ones; a state dict without them re-initialises the EMA from the parameters
            self._init_ema()
        # a captured train step holds the old state tensors: LDMTrainer re-captures when this moves
        self.state_epoch = getattr(self, "state_epoch", 0) + 1

    def _step_capturable(self, gi, group, params, found_inf, grad_mul=None):
        """One launch pair for the group: ldm_adam_step_dev advances the group's device step count (shared
        by its params' state["step"]) unless found_inf is set and forms the scalars from it on the device."""
        dev = params[0].device
        gstep = group.get("_ldm_step")
        if gstep is None:
            prev = [self.state[p]["step"] for p in params if "step" in self.state[p]]
            init = float(prev[0]) if prev else 0.0
            if any(float(s) != init for s in prev):
                raise RuntimeError("ldm_amd.optim.Adam(capturable=True): params of a group at different steps")
            gstep = torch.full((), init, dtype=torch.float32, device=dev)
            group["_ldm_step"] = gstep
            group["_ldm_scalars"] = torch.zeros(8, dtype=torch.float32, device=dev)
        for p in params:
            st = self.state[p]
            if len(st) == 0 or "exp_avg" not in st:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] = gstep
        tab = _SlotTable(params, [p.grad for p in params], [self.state[p]["exp_avg"] for p in params],
                         [self.state[p]["exp_avg_sq"] for p in params])
        self._launch(tab, params, group, found_inf, grad_mul, gstep.data_ptr(), group["_ldm_scalars"])
        self._tables[(gi, "dev")] = tab
        for p in params:
            torch.autograd.graph.increment_version(p)


class AdamW(Adam):
    """torch.optim.AdamW (decoupled weight decay, default 1e-2)."""

    _decoupled = 1

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False,
                 capturable=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                         capturable=capturable)


class GradScaler:
    """torch.amp.GradScaler('cuda') semantics: scale(loss) multiplies by the current scale, step()
    unscales the grads (device kernel), skips the optimiser step when any grad is inf/nan, update()
    backs the scale off (x0.5) on inf or grows it (x2) after growth_interval clean steps."""

    def __init__(self, device="cuda", init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5,
                 growth_interval=2000, enabled=True):
        self._device = device
        self._init_scale = init_scale
        self._growth_factor = growth_factor
        self._backoff_factor = backoff_factor
        self._growth_interval = growth_interval
        self._enabled = enabled
        self._scale = None
        self._tracker = None
        self._found_inf = None
        self._unscaled = set()
        self._divisor = 1.0
        self.last_grad_norm = None   # device 0-d fp32: the last unscale_(max_norm=...)'s gradient norm
        self._clip_coef = None       # device fp32 [1]: its clip coefficient, the next step()'s gradient multiplier
        self._norm_cache = {}

    def is_enabled(self):
        return self._enabled

    def set_grad_divisor(self, d):
        """Extra factor 1/d folded into unscale_ (data-parallel gradient averaging: d = world size)."""
        self._divisor = float(d)

    def _lazy_init(self, dev):
        if self._scale is None:
            self._scale = torch.full((1,), self._init_scale, dtype=torch.float32, device=dev)
            self._tracker = torch.zeros((1,), dtype=torch.int32, device=dev)
            self._found_inf = torch.zeros((1,), dtype=torch.int32, device=dev)

    def get_scale(self):
        return float(self._scale.item()) if self._scale is not None else self._init_scale

    def scale(self, outputs):
        if not self._enabled:
            return outputs
        self._lazy_init(outputs.device)
        return outputs * self._scale.to(outputs.device)

    def unscale_(self, optimizer, max_norm=None):
        """scaler.unscale_.  max_norm (optional): the same launches also form the global 2-norm of the unscaled
        gradients (ldm_unscale_check_norm) and a one-block finalize leaves [norm, coef] on the device:
        last_grad_norm (0-d) and _clip_coef, which step() hands to the optimizer as its gradient multiplier
        (torch.nn.utils.clip_grad_norm_'s coefficient; max_norm <= 0: norm only)."""
        if max_norm is not None and not self._enabled:
            raise RuntimeError("ldm_amd.optim.GradScaler: a disabled scaler does not clip; use clip_grad_norm_")
        if not self._enabled or id(optimizer) in self._unscaled:
            return
        self._lazy_init(next(p.device for g in optimizer.param_groups for p in g["params"]))
        # GradScaler: scale.double().reciprocal().float()  (x 1/divisor for data-parallel averaging)
        inv = torch.reciprocal(self._scale.double() * self._divisor).float()
        self._found_inf.zero_()
        if max_norm is not None:
            groups = [[p for p in g["params"] if p.grad is not None] for g in optimizer.param_groups]
            if any(groups):
                buf, tabs = _norm_pass(groups, max_norm, inv, self._norm_cache, self._found_inf)
                optimizer.param_groups[0].setdefault("_ldm_tabs", []).extend(tabs)   # keep alive until the launches ran
                self.last_grad_norm = buf.pair[0]
                self._clip_coef = buf.pair[1:2] if max_norm > 0 else None
            self._unscaled.add(id(optimizer))
            return
        self.last_grad_norm = self._clip_coef = None
        for group in optimizer.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            _check_params(ps)
            tab = _SlotTable(ps, [p.grad for p in ps], [None] * len(ps), [None] * len(ps))
            L.call("ldm_unscale_check", *tab.args(), inv.data_ptr(), self._found_inf.data_ptr(), stream_handle())
            group.setdefault("_ldm_tabs", []).append(tab)   # keep alive until the launch ran
        self._unscaled.add(id(optimizer))

    def step(self, optimizer, *args, **kwargs):
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        self.unscale_(optimizer)
        for group in optimizer.param_groups:
            group.pop("_ldm_tabs", None)
        if self._clip_coef is not None:
            kwargs["grad_mul"] = self._clip_coef
        if getattr(optimizer, "capturable", False):
            # device-side skip: the kernel pair reads found_inf and leaves the step count alone on inf/nan
            return optimizer.step(*args, found_inf=self._found_inf, **kwargs)
        # torch's GradScaler also syncs here (found_inf.item()) so that the optimiser's step counters
        # only advance on applied steps
        if int(self._found_inf.item()) == 0:
            return optimizer.step(*args, **kwargs)
        return None

    def update(self, new_scale=None):
        if not self._enabled:
            return
        if new_scale is not None:
            self._scale.fill_(float(new_scale))
        else:
            L.call("ldm_update_scale", self._scale.data_ptr(), self._tracker.data_ptr(), self._found_inf.data_ptr(),
                   float(self._growth_factor), float(self._backoff_factor), int(self._growth_interval),
                   stream_handle())
        self._unscaled.clear()
        self._clip_coef = None   # (last_grad_norm stays readable until the next unscale_)

    def state_dict(self):
        if not self._enabled:
            return {}
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor,
                "backoff_factor": self._backoff_factor, "growth_interval": self._growth_interval,
                "_growth_tracker": int(self._tracker.item()) if self._tracker is not None else 0}

    def load_state_dict(self, sd):
        if not sd:
            return
        self._init_scale = sd["scale"]
        self._growth_factor = sd["growth_factor"]
        self._backoff_factor = sd["backoff_factor"]
        self._growth_interval = sd["growth_interval"]
        if self._scale is not None:
            self._scale.fill_(sd["scale"])
            self._tracker.fill_(sd["_growth_tracker"])
