"""Fused multi-tensor Adam / AdamW on the HIP kernel hs_adam_step_multi.

Drop-in for torch.optim.Adam / AdamW as the reference uses them (scripts/train.py:257-261,
mibf_net/train_resnet.py:136-139): same hyper-parameters, param_groups (LR schedulers keep working),
state_dict layout (step / exp_avg / exp_avg_sq).  One launch per 32 tensors instead of torch's foreach chain.

MuonWithAuxAdam (scripts/train.py:262-307, `from muon import MuonWithAuxAdam`): Muon groups on csrc/muon.hip and batched hs_gemm
Newton-Schulz iterations, auxiliary groups on the same Adam kernel.

Global gradient-norm clipping (csrc/gradclip.hip; replaces torch.nn.utils.clip_grad_norm_, no reference counterpart):
`max_grad_norm=` on FusedAdam / FusedAdamW / FusedSGD clips inside the step without a host sync and leaves .grad unscaled;
`clip_grad_norm_` is the in-place stand-alone form for every other optimizer.
"""
import ctypes as C

import torch

from . import _lib as L
from . import rt


import os as _os
def _knock_adam():
    """measurement only (tools/knockout.sh): honoured only by a library built with -DHS_MEASURE, see csrc/blocks.hip knock()"""
    if not int(_os.environ.get("HAMSPINE_KNOCKOUT", "0")) & 32:
        return False
    return bool(L.lib().hs_measure_build())


_KNOCK_ADAM = None


# ------------------------------------------------------------------------------------------------------------------------
# global gradient-norm clipping on csrc/gradclip.hip (replaces torch.nn.utils.clip_grad_norm_; no reference counterpart)
# ------------------------------------------------------------------------------------------------------------------------
def _dense(t):
    """every element of t's memory span belongs to exactly one index (what a flat pass over numel() elements needs)"""
    if t.is_contiguous():
        return True
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda d: d[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def _clip_settings(max_grad_norm, nonfinite):
    """validated (max_grad_norm as a float or None, skip flag)"""
    if nonfinite not in ("propagate", "skip"):
        raise ValueError(f'nonfinite must be "propagate" or "skip", not {nonfinite!r}')
    if max_grad_norm is None:
        return None, nonfinite == "skip"
    max_grad_norm = float(max_grad_norm)
    if not max_grad_norm >= 0.0:
        raise ValueError(f"max_grad_norm must be >= 0 (float('inf') monitors only), not {max_grad_norm}")
    return max_grad_norm, nonfinite == "skip"


class _GradNorm:
    """The sum-of-squares and finish launches over one set of gradients, and the device record they leave:
    rec = [norm, clip coefficient, finite, skip] (include/hamspine.h).  Nothing is read back.

    Host cost (the note of _FusedAdamBase._update applies: a C2 step has ~400 gradient tensors): the pointer and size tables,
    the slot offsets of the launches and the buffers are built once per parameter set and revalidated against the gradient
    pointers of the step; the partials and the record are allocated once per device."""

    def __init__(self):
        self._tables = {}
        self._bufs = {}         # device -> {"rec": f32 [4], "partials": f64 [slots]}

    def _buffers(self, dev, slots, fresh_rec=False):
        b = self._bufs.get(dev)
        if b is None:
            b = self._bufs[dev] = {"rec": torch.empty(4, dtype=torch.float32, device=dev), "partials": None}
        if b["partials"] is None or b["partials"].numel() < slots:
            b["partials"] = torch.empty(max(slots, 1), dtype=torch.float64, device=dev)
        rec = torch.empty(4, dtype=torch.float32, device=dev) if fresh_rec else b["rec"]
        return rec, b["partials"]

    def rec(self, dev=None):
        """the record of the last measure() (on `dev`, or on the only device used so far), or None"""
        if dev is None:
            dev = next(iter(self._bufs), None)
        b = self._bufs.get(dev)
        return None if b is None else b["rec"]

    def measure(self, ps, max_norm, skip, fresh_rec=False):
        """ps: parameters with a gradient.  Enqueues the launches on the current stream -> (rec tensor, table entry)"""
        lib = L.lib()
        key = (len(ps), id(ps[0]), id(ps[-1]))
        ent = self._tables.get(key)
        ids = [id(p) for p in ps]
        if ent is None or ent["ids"] != ids:
            rt.need_gpu(*ps)
            dev = ps[0].device
            if any(p.device != dev for p in ps):
                raise L.HamspineError("gradient-norm clipping expects all parameters on one device")
            if len(self._tables) >= 8:          # parameter sets come and go (unused parameters): keep the cache small
                self._tables.clear()
            ent = self._tables[key] = {"ids": ids, "dev": dev, "gptrs": None, "chunks": None, "slots": 0}
        if any(p.grad.dtype != torch.float32 for p in ps):       # (every call: a pointer and a size say nothing about the type)
            raise L.HamspineError("gradient-norm clipping expects f32 gradients")
        gptrs = [(p.grad.data_ptr(), p.grad.numel()) for p in ps]
        if gptrs != ent["gptrs"]:
            rt.need_gpu(*[p.grad for p in ps])
            for p in ps:
                g = p.grad
                if not _dense(g):          # rare: an expanded or strided gradient produced outside our nodes
                    g2 = torch.empty_like(p, memory_format=torch.preserve_format)
                    g2.copy_(g)
                    p.grad = g2
            gptrs = [(p.grad.data_ptr(), p.grad.numel()) for p in ps]
            chunks, off = [], 0
            for base in range(0, len(ps), L.GRADCLIP_MAX):
                sel = ps[base:base + L.GRADCLIP_MAX]
                n = len(sel)
                cnt = (C.c_int64 * n)(*[gn for _, gn in gptrs[base:base + n]])
                slots = int(lib.hs_grad_norm_partials(n, cnt))
                if slots < 0:
                    raise L.HamspineError("hs_grad_norm_partials refused the sizes")
                chunks.append({"n": n, "garr": (C.c_void_p * n)(*[gp for gp, _ in gptrs[base:base + n]]), "cnt": cnt, "off": off})
                off += slots
            ent["gptrs"], ent["chunks"], ent["slots"] = gptrs, chunks, off
        rec, partials = self._buffers(ent["dev"], ent["slots"], fresh_rec)
        s, base = rt.stream(), partials.data_ptr()
        for ch in ent["chunks"]:
            L.check(lib.hs_grad_sumsq_multi(ch["n"], ch["garr"], ch["cnt"], base + 8 * ch["off"], s), "hs_grad_sumsq_multi")
        L.check(lib.hs_grad_norm_finish(base, ent["slots"], max_norm, 1 if skip else 0, rec.data_ptr(), s), "hs_grad_norm_finish")
        return rec, ent

    def scale(self, ent, rec):
        lib, s = L.lib(), rt.stream()
        for ch in ent["chunks"]:
            L.check(lib.hs_grad_scale_multi(ch["n"], ch["garr"], ch["cnt"], rec.data_ptr(), s), "hs_grad_scale_multi")


_standalone = _GradNorm()


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """torch.nn.utils.clip_grad_norm_ on the HIP kernels of csrc/gradclip.hip: one read of every gradient for the norm (f64
    sums in a fixed order), one finish launch, one in-place scaling pass that writes nothing when the coefficient is 1.
    Returns the pre-clip global norm as a 0-dim f32 device tensor (a CPU zero when no parameter has a gradient, as torch does);
    nothing is read back, except that error_if_nonfinite=True
    reads the `finite` flag and raises RuntimeError before scaling, as torch does.  norm_type other than 2 raises
    NotImplementedError.  The route for optimizers without a fused one (MuonWithAuxAdam); FusedAdam / FusedAdamW / FusedSGD
    take max_grad_norm= instead and never scale .grad."""
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"hamspine.optim.clip_grad_norm_: only norm_type=2 is implemented, not {norm_type}")
    max_norm, _ = _clip_settings(float(max_norm), "propagate")          # (None: TypeError, as in torch)
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    ps = [p for p in parameters if p.grad is not None]
    if not ps:
        return torch.zeros(())
    rec, ent = _standalone.measure(ps, max_norm, False, fresh_rec=True)
    if error_if_nonfinite and float(rec[2].item()) == 0.0:
        raise RuntimeError("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot be "
                           "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                           "`error_if_nonfinite=False`")
    _standalone.scale(ent, rec)
    return rec[0]


class _ClipMixin:
    """max_grad_norm / nonfinite of the fused optimizers.  The settings are attributes: param_groups and state_dict() keep
    torch.optim's layout."""

    def _clip_init(self, max_grad_norm, nonfinite):
        self.max_grad_norm, self._skip_nonfinite = _clip_settings(max_grad_norm, nonfinite)
        self.nonfinite = nonfinite
        self._gradnorm = _GradNorm() if self.max_grad_norm is not None else None

    # torch.optim.Optimizer pickles defaults, state and param_groups only: carry the two settings, rebuild the launch cache
    def __getstate__(self):
        st = dict(super().__getstate__())
        st["max_grad_norm"], st["nonfinite"] = getattr(self, "max_grad_norm", None), getattr(self, "nonfinite", "propagate")
        return st

    def __setstate__(self, state):
        super().__setstate__(state)
        self._clip_init(self.__dict__.get("max_grad_norm"), self.__dict__.get("nonfinite", "propagate"))

    def _clip_measure(self, grad_scale):
        """enqueues the norm launches over the gradients of ALL groups -> the device record, or None without any gradient"""
        if grad_scale != 1.0:
            raise L.HamspineError("max_grad_norm together with step(grad_scale != 1) is not supported: the norm is taken of "
                                  ".grad as it stands")
        ps = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
        if not ps:
            return None
        return self._gradnorm.measure(ps, self.max_grad_norm, self._skip_nonfinite)[0]

    def _rec_view(self, i):
        rec = None if getattr(self, "_gradnorm", None) is None else self._gradnorm.rec()
        return None if rec is None else rec[i]

    @property
    def grad_norm(self):
        """0-dim f32 device view: the global gradient norm before clipping of the last step (None before the first, or without
        max_grad_norm).  Rewritten by the next step: clone it to keep it."""
        return self._rec_view(0)

    @property
    def grad_clip_coef(self):
        """0-dim device view of the coefficient the last step multiplied the gradients by (see grad_norm)"""
        return self._rec_view(1)

    @property
    def grad_finite(self):
        """0-dim device view: 1.0 if the last step's norm was finite, else 0.0 (see grad_norm)"""
        return self._rec_view(2)


class _FusedAdamBase(_ClipMixin, torch.optim.Optimizer):
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, overlap_backward=None,
                 overlap_chunk=8 << 20, max_grad_norm=None, nonfinite="propagate"):
        """overlap_backward: update parameters while backward is still running -- as soon as `overlap_chunk` elements
        worth of gradients are final (post-accumulate hooks) their fused update is enqueued on a side stream ordered
        behind the streams that produced them; step() flushes the rest and joins.  Same arithmetic as stepping after
        backward; valid whenever nothing between backward and step() reads all gradients at once (no global-norm
        clipping, no gradient accumulation over several backwards), which is how the reference trains
        (scripts/train.py:373-385, mibf_net/train_resnet.py:29-33).

        max_grad_norm: clip the global 2-norm of the gradients of ALL param groups to this value, as
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm) in front of step() would, without a host sync and
        without the scaling pass: step() reads every gradient once for the norm (csrc/gradclip.hip), the coefficient
        min(max_grad_norm / (norm + 1e-6), 1) stays on the device and the step kernel multiplies by it.  Departure from the torch
        route: .grad is left UNSCALED.  float("inf") monitors only.  After a step `grad_norm`, `grad_clip_coef` and `grad_finite`
        are 0-dim device views of the result (no .item() needed to log them; the next step rewrites them).  None (default): step()
        is the code path it was.  Refused together with overlap_backward=True (the norm needs every gradient) and with
        step(grad_scale != 1).
        nonfinite: "propagate" (default) lets an inf / NaN norm follow torch's arithmetic (coefficient 0 / NaN); "skip" leaves
        parameters, moments and bf16 shadows untouched for that step.  A skipped step still advances state["step"]: the counter
        is a host integer and the host never learns that the step was skipped."""
        self._clip_init(max_grad_norm, nonfinite)
        if overlap_backward and self.max_grad_norm is not None:
            raise ValueError("max_grad_norm needs all gradients before the first update: it cannot be combined with "
                             "overlap_backward=True")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if overlap_backward is None:       # (HAMSPINE_ADAM_OVERLAP=1: A/B measurements of the mode without touching the caller)
            overlap_backward = _os.environ.get("HAMSPINE_ADAM_OVERLAP", "0") == "1" and self.max_grad_norm is None
        self._overlap = bool(overlap_backward)
        self._chunk = int(_os.environ.get("HAMSPINE_ADAM_CHUNK", "0")) << 20 or int(overlap_chunk)
        self._pending, self._pending_n = [], 0
        self._pending_streams = {}      # streams the pending gradients became final on (id -> torch.cuda.Stream)
        self._stream = None
        self._done = set()
        if self._overlap:
            self._group_of = {}
            for g in self.param_groups:
                for p in g["params"]:
                    self._group_of[p] = g
                    p.register_post_accumulate_grad_hook(self._on_grad)

    # -- optimizer-in-backward -------------------------------------------------------------------------------------
    def _on_grad(self, p):
        """post-accumulate hook: runs on the autograd thread with the AccumulateGrad node's stream current; the engine
        has already ordered that stream behind the node that produced the gradient."""
        if p in self._done:
            raise RuntimeError(
                "FusedAdam(overlap_backward=True): a parameter received a second gradient after its update was enqueued "
                "(a second backward() before step(): gradient accumulation) -- step after backward instead")
        s = torch.cuda.current_stream(p.device)
        self._pending_streams[s.cuda_stream] = s
        if not any(q is p for q in self._pending):
            self._pending.append(p)
            self._pending_n += p.numel()
        if self._pending_n >= self._chunk or len(self._pending) >= 96:
            self._flush()

    @torch.no_grad()
    def _flush(self):
        if not self._pending:
            return
        ps, self._pending, self._pending_n = self._pending, [], 0
        dev = ps[0].device
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=dev)
        # Order the update behind EVERY stream a pending gradient became final on -- not only the stream of the hook that
        # happens to trigger the flush.  (Round-1 bug: the image tower's backward runs first, on the ambient stream; the
        # stem's small gradients stayed pending below the chunk size and were flushed later from a BERT parameter's hook,
        # whose current stream is the text tower's: the update then waited for the tower stream only and could read the
        # stem's weight gradient before its GEMM had finished.)
        streams, self._pending_streams = self._pending_streams, {}
        cur = torch.cuda.current_stream(dev)
        streams[cur.cuda_stream] = cur
        for s in streams.values():
            self._stream.wait_stream(s)
        with torch.cuda.stream(self._stream):
            by_group = {}
            for p in ps:
                by_group.setdefault(id(self._group_of[p]), (self._group_of[p], []))[1].append(p)
            for group, sel in by_group.values():
                self._update(group, sel, 1.0)
        self._done.update(ps)

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._overlap and closure is None and grad_scale == 1.0:
            self._flush()
            done, self._done = self._done, set()
            for group in self.param_groups:                 # parameters whose hook never fired this step (none, normally)
                rest = [p for p in group["params"] if p.grad is not None and p not in done]
                if rest:
                    self._update(group, rest, 1.0)
            if self._stream is not None:
                torch.cuda.current_stream(self._stream.device).wait_stream(self._stream)
            return loss
        rec = self._clip_measure(grad_scale) if getattr(self, "max_grad_norm", None) is not None else None
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if ps:
                self._update(group, ps, grad_scale, rec)
        return loss

    def _update(self, group, ps, grad_scale, rec=None):
        """one fused launch (per 32 tensors) for the parameters `ps` of `group`, on the current stream.

        Host cost matters here (a C2 step has ~400 parameter tensors; the first version spent 1.5 ms per step in this
        function): everything that does not move between steps -- parameter / moment pointer tables, sizes, strides, the
        per-tensor checks -- is built once per parameter set, the step counter is ONE shared 0-dim tensor per chunk
        (state[p]["step"] of every tensor in it), and the gradient pointer table is rebuilt only when a gradient pointer
        changed (the tower executors and hamspine.ddp hand out the same gradient memory every step).

        rec: the device record of the step's gradient norm (_GradNorm): the launch is hs_adam_step_multi_clip."""
        global _KNOCK_ADAM
        if _KNOCK_ADAM is None:
            _KNOCK_ADAM = _knock_adam()
        if not ps or _KNOCK_ADAM:
            return
        lib = L.lib()
        key = (id(group), len(ps), id(ps[0]), id(ps[-1]))
        cache = self.__dict__.setdefault("_tables", {})
        ent = cache.get(key)
        if ent is None or ent["ids"] != [id(p) for p in ps]:
            rt.need_gpu(*ps)
            by_step = {}
            for p in ps:
                st = self.state[p]
                if not st:
                    st["step"] = torch.zeros((), dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if p.dtype != torch.float32:
                    raise L.HamspineError("FusedAdam expects f32 parameters and gradients")
                by_step.setdefault(int(st["step"]), []).append(p)
            ent = {"ids": [id(p) for p in ps], "chunks": []}
            for step0, sel in by_step.items():      # tensors of a group normally share the step count
                n = len(sel)
                arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
                shared = torch.tensor(float(step0), dtype=torch.float32)
                for p in sel:
                    self.state[p]["step"] = shared                       # one counter object for the whole chunk
                ent["chunks"].append({
                    "sel": sel, "n": n, "p": arr(sel), "m": arr([self.state[p]["exp_avg"] for p in sel]),
                    "v": arr([self.state[p]["exp_avg_sq"] for p in sel]), "cnt": (C.c_int64 * n)(*[p.numel() for p in sel]),
                    "ptrs": [p.data_ptr() for p in sel], "strides": [p.stride() for p in sel], "step": shared,
                    "step_host": int(step0), "gptrs": None, "garr": None, "shadow_epoch": -1, "h": None})
            cache[key] = ent
        b1, b2 = group["betas"]
        for ch in ent["chunks"]:
            sel, n = ch["sel"], ch["n"]
            if [p.data_ptr() for p in sel] != ch["ptrs"]:     # a parameter was re-allocated (.to(), load)
                cache.pop(key, None)
                return self._update(group, ps, grad_scale, rec)
            gptrs = [p.grad.data_ptr() for p in sel]
            if gptrs != ch["gptrs"]:
                for p, st in zip(sel, ch["strides"]):
                    g = p.grad
                    if g.dtype != torch.float32:
                        raise L.HamspineError("FusedAdam expects f32 parameters and gradients")
                    if g.stride() != st:    # rare: a gradient produced outside our nodes in another layout
                        g2 = torch.empty_like(p, memory_format=torch.preserve_format)
                        g2.copy_(g)
                        p.grad = g2
                gptrs = [p.grad.data_ptr() for p in sel]
                ch["gptrs"], ch["garr"] = gptrs, (C.c_void_p * n)(*gptrs)
            # Every tensor of the chunk must still share THIS chunk's counter object.  load_state_dict replaces the counters;
            # so does another table of the same group built for a different set of parameters-with-gradients (an unused
            # parameter, an expert without tokens, set_to_none): it rebinds state[p]["step"] of its own subset, and a check of
            # the first tensor alone would let this table's stale step_host through for the rest.  On a mismatch the table
            # is rebuilt from the per-parameter counters (by_step above), which keeps torch.optim's per-parameter step count.
            st_all = self.state
            if any(st_all[p]["step"] is not ch["step"] for p in sel):
                cache.pop(key, None)
                return self._update(group, ps, grad_scale, rec)
            ch["step_host"] += 1
            ch["step"].fill_(ch["step_host"])                  # 0-dim CPU tensor: no device work
            # bf16 shadows the towers registered for these parameters (hamspine.rt): written by the same kernel, so the next
            # forward needs no cast.  The pointer table follows the registry's epoch.
            if ch["shadow_epoch"] != rt.shadow_epoch():
                hp = [rt.shadow_ptr_of(p) for p in sel]
                ch["h"] = (C.c_void_p * n)(*hp) if any(hp) else None
                ch["shadow_epoch"] = rt.shadow_epoch()
            if rec is not None:
                L.check(lib.hs_adam_step_multi_clip(
                    n, ch["p"], ch["garr"], ch["m"], ch["v"], ch["h"], ch["cnt"], float(group["lr"]), b1, b2, group["eps"],
                    group["weight_decay"], ch["step_host"], 1 if self._decoupled else 0, float(grad_scale), rec.data_ptr(),
                    rt.stream()), "hs_adam_step_multi_clip")
                continue
            L.check(lib.hs_adam_step_multi_shadow(
                n, ch["p"], ch["garr"], ch["m"], ch["v"], ch["h"], ch["cnt"], float(group["lr"]), b1, b2, group["eps"],
                group["weight_decay"], ch["step_host"], 1 if self._decoupled else 0, float(grad_scale), rt.stream()),
                "hs_adam_step_multi_shadow")


class FusedAdamW(_FusedAdamBase):
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kw):
        super().__init__(params, lr, betas, eps, weight_decay, **kw)


class FusedAdam(_FusedAdamBase):
    _decoupled = False


class MuonWithAuxAdam(_FusedAdamBase):
    """The optimizer of `configs/ham/ham_optimizer_muon_v1.yml` (reference scripts/train.py:262-307, `from muon import
    MuonWithAuxAdam`): every param group carries `use_muon`.

    use_muon=True   (lr=0.02, momentum=0.95, weight_decay=0; parameters with ndim >= 2)
        m <- m + (1-beta)(g-m);  u = g + beta(m-g);  O = NewtonSchulz5(u as (shape[0], -1));
        p <- p (1 - lr wd) - lr sqrt(max(1, shape[-2] / shape[-1])) O
      on csrc/muon.hip: one pre-pass and one apply pass over all tensors, and per (rows, cols) shape group ONE
      hs_muon_orthogonalize call whose fifteen products are batched hs_gemm launches in the compute dtype.
    use_muon=False  (lr=3e-4, betas=(0.9, 0.95), eps=1e-10, weight_decay=0)
        Adam with bias correction and decoupled weight decay: _FusedAdamBase._update as it is.

    state_dict layout: momentum_buffer / step, exp_avg, exp_avg_sq.  Parameters without a gradient are skipped (the published
    package substitutes zeros to keep data-parallel ranks in lock-step; under hamspine.ddp every rank sees every gradient).
    f32 parameters and gradients only; there is no overlap_backward and no max_grad_norm: clip with
    hamspine.optim.clip_grad_norm_(parameters, max_norm) in front of step()."""
    _decoupled = True

    def __init__(self, param_groups):
        groups = []
        for g in param_groups:
            if not isinstance(g, dict) or "use_muon" not in g:
                raise ValueError("MuonWithAuxAdam: every param group needs a `use_muon` entry")
            g = dict(g)
            g["params"] = list(g["params"])
            if g["use_muon"]:
                for k, v in (("lr", 0.02), ("momentum", 0.95), ("weight_decay", 0.0)):
                    g.setdefault(k, v)
                if any(p.ndim < 2 for p in g["params"]):
                    raise ValueError("MuonWithAuxAdam: a use_muon group holds a parameter with ndim < 2")
            else:
                for k, v in (("lr", 3e-4), ("betas", (0.9, 0.95)), ("eps", 1e-10), ("weight_decay", 0.0)):
                    g.setdefault(k, v)
            groups.append(g)
        self._clip_init(None, "propagate")      # no fused clipping here: hamspine.optim.clip_grad_norm_ in front of step()
        torch.optim.Optimizer.__init__(self, groups, dict())
        self._plans = {}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            if group["use_muon"]:
                self._muon_update(group, ps)
            else:
                self._update(group, ps, 1.0)
        return loss

    def _muon_plan(self, group, ps, dt):
        """everything that does not move between steps (the host-cost note of _FusedAdamBase._update applies): shape groups,
        the packed compute-dtype buffer, pointer tables of parameters / momenta / packed matrices, sizes and scales"""
        rt.need_gpu(*ps)
        lib = L.lib()
        by_shape = {}
        for p in ps:
            if p.dtype != torch.float32:
                raise L.HamspineError("MuonWithAuxAdam expects f32 parameters and gradients")
            if p.ndim < 2 or p.numel() == 0:
                raise L.HamspineError("MuonWithAuxAdam: a use_muon parameter needs ndim >= 2 and elements")
            rows, cols = p.shape[0], p.numel() // p.shape[0]
            # the parameter's memory is read as it lies, as a (rows, cols) matrix: dense, dimension 0 outermost.  For a
            # channels_last filter that is a column permutation of the (K, C R S) view, which Newton-Schulz commutes with
            dense = p.is_contiguous() or (p.ndim == 4 and p.is_contiguous(memory_format=torch.channels_last))
            if not dense or (rows > 1 and p.stride(0) != cols):
                raise L.HamspineError("MuonWithAuxAdam: a parameter must be dense with dimension 0 outermost in memory")
            st = self.state[p]
            if "momentum_buffer" not in st:
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            by_shape.setdefault((rows, cols), []).append(p)
        esz = 2 if dt == torch.bfloat16 else 4
        c8 = lambda v: (v + 7) // 8 * 8
        order, shapes, offs, off, ws_bytes = [], [], [], 0, 0
        hs_dt = rt.hs_dtype(dt)
        for (rows, cols), sel in by_shape.items():
            shapes.append((rows, cols, len(sel), off))
            for p in sel:
                order.append(p)
                offs.append(off)
                off += c8(rows) * c8(cols) * esz
            off = (off + 255) // 256 * 256
            ws_bytes = max(ws_bytes, int(lib.hs_muon_ws_bytes(hs_dt, len(sel), rows, cols)))
        n = len(order)
        dev = order[0].device
        packed = torch.empty(off, dtype=torch.uint8, device=dev)
        base = packed.data_ptr()
        moms = [self.state[p]["momentum_buffer"] for p in order]
        return {
            "ids": [id(p) for p in ps], "order": order, "n": n, "dt": dt, "hs_dt": hs_dt, "packed": packed, "shapes": shapes,
            "ws_bytes": ws_bytes, "partials": torch.empty(n * L.MUON_PARTIALS, dtype=torch.float32, device=dev),
            "p": (C.c_void_p * n)(*[p.data_ptr() for p in order]), "m": (C.c_void_p * n)(*[m.data_ptr() for m in moms]),
            "x": (C.c_void_p * n)(*[base + o for o in offs]),
            "rows": (C.c_int32 * n)(*[p.shape[0] for p in order]),
            "cols": (C.c_int32 * n)(*[p.numel() // p.shape[0] for p in order]),
            "scale": (C.c_float * n)(*[max(1.0, p.shape[-2] / p.shape[-1]) ** 0.5 for p in order]),
            "ptrs": [p.data_ptr() for p in order], "mptrs": [m.data_ptr() for m in moms],
            "strides": [p.stride() for p in order], "gptrs": None, "garr": None, "shadow_epoch": -1, "h": None}

    def _muon_update(self, group, ps):
        import hamspine
        dt = hamspine.compute_dtype()
        key = (id(group), len(ps), id(ps[0]), id(ps[-1]))
        pl = self._plans.get(key)
        if pl is not None:
            order = pl["order"]
            state = self.state
            if (pl["dt"] != dt or pl["ids"] != [id(p) for p in ps] or [p.data_ptr() for p in order] != pl["ptrs"] or
                    any("momentum_buffer" not in state[p] for p in order) or
                    [state[p]["momentum_buffer"].data_ptr() for p in order] != pl["mptrs"]):
                pl = None            # another mode, another parameter set, a re-allocated parameter, a loaded state
        if pl is None:
            live = {id(g) for g in self.param_groups}      # load_state_dict replaces the group dicts: let their plans' buffers go
            self._plans = {k: v for k, v in self._plans.items() if k[0] in live and k != key}
            pl = self._plans[key] = self._muon_plan(group, ps, dt)
        order, n = pl["order"], pl["n"]
        gptrs = [p.grad.data_ptr() for p in order]
        if gptrs != pl["gptrs"]:
            for p, st in zip(order, pl["strides"]):
                g = p.grad
                if g.dtype != torch.float32:
                    raise L.HamspineError("MuonWithAuxAdam expects f32 parameters and gradients")
                if g.stride() != st:    # rare: a gradient produced outside our nodes in another layout
                    g2 = torch.empty_like(p, memory_format=torch.preserve_format)
                    g2.copy_(g)
                    p.grad = g2
            gptrs = [p.grad.data_ptr() for p in order]
            pl["gptrs"], pl["garr"] = gptrs, (C.c_void_p * n)(*gptrs)
        if pl["shadow_epoch"] != rt.shadow_epoch():
            hp = [rt.shadow_ptr_of(p) for p in order]
            pl["h"] = (C.c_void_p * n)(*hp) if any(hp) else None
            pl["shadow_epoch"] = rt.shadow_epoch()
        lib, s, hs_dt = L.lib(), rt.stream(), pl["hs_dt"]
        L.check(lib.hs_muon_prepare_multi(hs_dt, n, pl["m"], pl["garr"], pl["x"], pl["rows"], pl["cols"], float(group["momentum"]),
                                          pl["partials"].data_ptr(), s), "hs_muon_prepare_multi")
        ws = rt.workspace(pl["ws_bytes"], order[0].device)
        base = pl["packed"].data_ptr()
        for rows, cols, count, off in pl["shapes"]:        # one ABI call per shape group
            L.check(lib.hs_muon_orthogonalize(hs_dt, count, rows, cols, base + off, ws.data_ptr(), ws.numel(), s),
                    "hs_muon_orthogonalize")
        L.check(lib.hs_muon_apply_multi(hs_dt, n, pl["p"], pl["h"], pl["x"], pl["rows"], pl["cols"], pl["scale"],
                                        float(group["lr"]), float(group["weight_decay"]), s), "hs_muon_apply_multi")


class FusedSGD(_ClipMixin, torch.optim.Optimizer):
    """torch.optim.SGD (weight decay, momentum with dampening 0, Nesterov) on hs_sgd_step_multi: the reference's fallback
    optimizer (scripts/train.py:309).  Same hyper-parameters, param_groups and state_dict layout (momentum_buffer).

    max_grad_norm / nonfinite: global gradient-norm clipping inside the step, as FusedAdam documents it (hs_sgd_step_multi_clip;
    .grad stays unscaled; with nonfinite="skip" a skipped step leaves parameters and momentum buffers untouched.  A buffer whose
    seeding step was skipped holds zeros, and the next step's momentum * 0 + g seeds it exactly as torch would have)."""

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, nesterov=False, max_grad_norm=None, nonfinite="propagate"):
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum")
        self._clip_init(max_grad_norm, nonfinite)
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov))

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.lib()
        rec = self._clip_measure(grad_scale) if getattr(self, "max_grad_norm", None) is not None else None
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            rt.need_gpu(*ps)
            mom = float(group["momentum"])
            # tensors seeing their first momentum step are seeded with the gradient (torch.optim.SGD): partition first
            fresh = [p for p in ps if mom != 0 and "momentum_buffer" not in self.state[p]]
            seen = [p for p in ps if not (mom != 0 and "momentum_buffer" not in self.state[p])]
            for first, sel in ((True, fresh), (False, seen)):
                if not sel:
                    continue
                n = len(sel)
                for p in sel:
                    if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                        raise L.HamspineError("FusedSGD expects f32 parameters and gradients")
                    if p.grad.stride() != p.stride():
                        g2 = torch.empty_like(p, memory_format=torch.preserve_format)
                        g2.copy_(p.grad)
                        p.grad = g2
                    if mom != 0 and first:
                        # the kernel seeds the buffer with the gradient (first = 1).  A clipped launch may be skipped on the
                        # device and then stores nothing: the buffer starts as zeros, so that the next step (first = 0:
                        # momentum * 0 + g) seeds it with the same bits
                        new = torch.zeros_like if rec is not None else torch.empty_like
                        self.state[p]["momentum_buffer"] = new(p, memory_format=torch.preserve_format)
                arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
                bufs = arr([self.state[p]["momentum_buffer"] for p in sel]) if mom != 0 else None
                cnt = (C.c_int64 * n)(*[p.numel() for p in sel])
                if rec is not None:
                    L.check(lib.hs_sgd_step_multi_clip(n, arr(sel), arr([p.grad for p in sel]), bufs, cnt, float(group["lr"]), mom,
                                                       float(group["weight_decay"]), 1 if group["nesterov"] else 0,
                                                       1 if first else 0, float(grad_scale), rec.data_ptr(), rt.stream()),
                            "hs_sgd_step_multi_clip")
                else:
                    L.check(lib.hs_sgd_step_multi(n, arr(sel), arr([p.grad for p in sel]), bufs, cnt, float(group["lr"]), mom,
                                                  float(group["weight_decay"]), 1 if group["nesterov"] else 0, 1 if first else 0,
                                                  float(grad_scale), rt.stream()), "hs_sgd_step_multi")
                rt.shadows_stale(sel)      # this kernel does not write the bf16 weight shadows: the next forward re-casts them
        return loss
