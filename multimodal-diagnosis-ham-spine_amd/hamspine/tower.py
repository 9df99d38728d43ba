"""Whole-tower autograd nodes: one C call per tower per direction (hs_resnet_fwd/bwd, hs_bert_fwd/bwd).

The reference loop calls the model once per step (scripts/train.py:373-385, mibf_net/train_resnet.py:30-32); with one
autograd node per residual block / BertLayer a C2 step cost ~70 Python -> C round trips (descriptor rebuild, three layout
passes and several tensor allocations each): 11 ms of host time against 12.6 ms of GPU time.  Here the descriptors of a
whole tower are built ONCE per (module, shape, mode) and reused; a step pays one Function.apply, one saved-arena
allocation and one C call per tower and direction.

Parameter gradients of a tower live in one flat f32 buffer owned by the cache entry (fresh view objects are handed to
autograd every step, so AccumulateGrad adopts them without a copy); with hamspine.ddp the bucket slots are used instead.
The per-block modules stay the hookable path: a tower falls back to them whenever any of its submodules carries a hook
(Grad-CAM: reference scripts/run_analysis.py:126-133).
"""
import os
import ctypes as C

import torch
from torch.autograd import Function
from torch.nn.modules import module as _nn_module

import hamspine

from . import _lib as L
from . import desc as DL
from . import rt

_CACHE_ATTR = "_hamspine_tower_cache"
DEBUG_KEEP = None      # tests set this to a list: every ResNet tower forward appends (cache entry, saved arena)


def _has_hooks(root):
    """any forward / backward hook on `root` or below it, or registered globally"""
    if (_nn_module._global_forward_hooks or _nn_module._global_forward_pre_hooks or _nn_module._global_backward_hooks or
            getattr(_nn_module, "_global_backward_pre_hooks", None)):
        return True
    # the walk over root.modules() costs 0.27 ms on ResNet50 / BERT-base (three towers a step): the module list is kept
    # on the root, keyed by the identity of its direct children (a tower whose inner structure is edited in place after its
    # first forward also invalidates the descriptor cache below, which is rebuilt from the same walk)
    key = tuple(map(id, root._modules.values()))
    cached = root.__dict__.get("_hamspine_module_list")
    if cached is None or cached[0] != key:
        cached = (key, list(root.modules()))
        root.__dict__["_hamspine_module_list"] = cached
    for m in cached[1]:
        if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None):
            return True
    return False


def towers_enabled():
    """The whole-tower nodes are the default everywhere, data parallelism included: hamspine.ddp gets one HIP event per
    gradient bucket from inside the tower's backward (hs_grad_milestones), so a bucket's exchange starts behind its own last
    gradient while the rest of the tower still runs; under torch's DistributedDataParallel (reference
    mibf_net/train_resnet.py:134) the tower's gradients become ready together at its end, which costs overlap, not
    correctness.  HAMSPINE_TOWER_EXEC=0 selects the per-block nodes."""
    return os.environ.get("HAMSPINE_TOWER_EXEC", "1") != "0"


def _with_milestones(ent, params, call):
    """run `call()` (one hs_*_bwd) with the data-parallel wrappers' bucket milestones registered: each gets the event of
    every bucket recorded at the point of this stream where that bucket's last gradient has been enqueued"""
    stream = torch.cuda.current_stream()
    # (parameters that get no gradient from this backward are passed as None: the wrapper books only what is produced)
    mp = getattr(ent, "_ms_params", None)              # (the same list object every step: the wrapper caches its bookkeeping on it)
    if mp is None or mp[0] is not ent.grad_ptrs:
        mp = ent._ms_params = (ent.grad_ptrs, [p if ent.grad_ptrs[i] else None for i, p in enumerate(params)])
    asked = rt.grad_milestones(mp[1], stream) if ent.store is None else []
    flat = [(ent.grad_ptrs[i], ev) for _, ms in asked for i, ev, _ in ms if ent.grad_ptrs[i]]
    lib = L.lib()
    if flat:
        n = len(flat)
        L.check(lib.hs_grad_milestones(n, (C.c_void_p * n)(*[q for q, _ in flat]), (C.c_void_p * n)(*[e for _, e in flat])),
                "hs_grad_milestones")
    try:
        call()
    finally:
        if flat:
            lib.hs_grad_milestones(0, None, None)
    for o, ms in asked:
        o._milestones_recorded([k for _, _, k in ms])


class _GradStore:
    """flat f32 gradient buffer of a tower + the slot (offset, shape, strides) of every parameter"""

    def __init__(self, params, needs, device):
        self.slots = []
        n = 0
        for p, need in zip(params, needs):
            if need:
                self.slots.append((n, tuple(p.shape), tuple(p.stride())))
                n += (p.numel() + 63) // 64 * 64
            else:
                self.slots.append(None)
        self.flat = torch.empty(max(n, 1), dtype=torch.float32, device=device)
        self.base = self.flat.data_ptr()

    def ptr(self, i):
        s = self.slots[i]
        return None if s is None else self.base + 4 * s[0]

    def views(self):
        f = self.flat
        return [None if s is None else f.as_strided(s[1], s[2], s[0]) for s in self.slots]


def _param_grad_ptrs(params, needs, device):
    """where the backward writes d(param): DDP bucket slots when hamspine.ddp registered them, else a private flat buffer.
    Returns (store or None, pointer list, view factory)."""
    arena = [rt._grad_arena.get(p.data_ptr()) if need else None for p, need in zip(params, needs)]
    if any(a is not None for a in arena):
        if not all((a is not None and a.shape == p.shape) or not need for a, p, need in zip(arena, params, needs)):
            raise L.HamspineError("hamspine.tower: only some parameters of a tower have DDP bucket slots")
        return None, [None if a is None else a.data_ptr() for a in arena], (lambda: [None if a is None else a.detach() for a in arena])
    store = _GradStore(params, needs, device)
    return store, [store.ptr(i) for i in range(len(params))], store.views


# =====================================================================================================================
# ResNet
# =====================================================================================================================
def resnet_blocks(model):
    return [b for layer in (model.layer1, model.layer2, model.layer3, model.layer4) for b in layer]


def resnet_params(model):
    """stem (w, gamma, beta), then per block its main stages and the optional downsample pair, each (w, gamma, beta)"""
    pairs = [(model.conv1, model.bn1)] + [cn for b in resnet_blocks(model) for cn in DL.block_pairs(b)]
    return [p for c, n in pairs for p in DL.conv_bn_params(c, n)], [n for _, n in pairs]


bert_params = DL.bert_params      # the embeddings' parameters, then every layer's (desc.BERT_EMBED_SLOTS, BERT_LAYER_SLOTS)


def _stage(conv, bn):
    if not conv.weight.is_contiguous(memory_format=torch.channels_last):
        raise L.HamspineError("hamspine.tower: conv filters must be channels_last (KRSC) in memory")
    return (conv.geo(), *DL.conv_bn_params(conv, bn), bn.running_mean, bn.running_var)


def resnet_desc(model, x_shape, dtype, training, inference, taps, grad_ptrs):
    """hs_resnet_desc of `model` for one input shape and mode (no library call: the entry below asks for the plan)"""
    blocks = resnet_blocks(model)
    if len(blocks) > L.RESNET_MAX_BLOCKS:
        raise L.HamspineError(f"hamspine.tower: {len(blocks)} residual blocks (max {L.RESNET_MAX_BLOCKS})")
    d = L.ResnetDesc()
    N, _, H, W = x_shape
    hd = rt.hs_dtype(dtype)
    eps, mom = model.bn1.eps, DL.bn_momentum(model.bn1)
    DL.fill_stem(d.stem, hd, N, H, W, training, eps, mom, *_stage(model.conv1, model.bn1), inference=inference)
    H, W = DL.stem_out(H), DL.stem_out(W)
    d.n_blocks = len(blocks)
    for i, b in enumerate(blocks):
        stages = [_stage(c, n) for c, n in DL.block_pairs(b)]
        if any(n.eps != eps or DL.bn_momentum(n) != mom for _, n in b._pairs()):
            raise L.HamspineError("hamspine.tower: BatchNorm layers of a tower must share eps / momentum")
        DL.fill_resblock(d.blocks[i], hd, N, H, W, training, eps, mom, stages, b.downsample is not None, inference=inference)
        for _, _, R, stride, pad in (c.geo() for c, _ in b._pairs()):
            H, W = DL.conv_out(H, R, stride, pad), DL.conv_out(W, R, stride, pad)
    d.n_taps, d.tap_block[:len(taps)] = len(taps), taps
    DL.set_grads(d, grad_ptrs)
    return d


class _Entry:
    """what a tower keeps per (module, shape, mode): its descriptor, where its parameter gradients go, its arena sizes"""

    def __init__(self, params, needs, device, dtype):
        self.store, self.grad_ptrs, self.make_views = _param_grad_ptrs(params, needs, device)
        self.param_ptrs = [p.data_ptr() for p in params]
        self.dtype = dtype
        self.arena_version = rt.arena_version()
        self.outstanding = self.peak = 0

    def valid_for(self, params):
        return self.arena_version == rt.arena_version() and all(p.data_ptr() == q for p, q in zip(params, self.param_ptrs))


class _ResnetEntry(_Entry):
    def __init__(self, model, x_shape, dtype, training, inference, taps, params, needs, device):
        super().__init__(params, needs, device, dtype)
        self.desc = resnet_desc(model, x_shape, dtype, training, inference, taps, self.grad_ptrs)
        self.plan = L.ResnetPlan()
        L.check(L.lib().hs_resnet_query(C.byref(self.desc), C.byref(self.plan)), "hs_resnet_query")
        self.saved_bytes, self.ws_bytes = int(self.plan.saved_bytes), int(self.plan.ws_bytes)
        es = 2 if dtype == torch.bfloat16 else 4
        self.taps = [(int(self.plan.tap_offset[t]), (x_shape[0], int(self.plan.tap_H[t]), int(self.plan.tap_W[t]), int(self.plan.tap_C[t])), es)
                     for t in range(len(taps))]
        self.shadow_groups = DL.resnet_shadow_groups(params) if dtype == torch.bfloat16 else []      # for rt.ensure_shadows


class _Pending:
    """one differentiable forward of a tower whose backward has not run yet (released by the backward, or when the graph
    is dropped without one)"""

    def __init__(self, ent):
        self.ent = ent
        ent.outstanding += 1
        ent.peak = max(ent.peak, ent.outstanding)

    def finish(self):
        ent, self.ent = self.ent, None
        if ent is not None:
            ent.outstanding = max(0, ent.outstanding - 1)
            if ent.outstanding == 0:
                ent.peak = 0

    __del__ = finish


def _shared_buffer_unsafe(ent, params):
    """may this backward write into the entry's cached gradient buffer?  Not when the tower ran more than once in the graph
    being differentiated (gate / global-local models: reference model.py:257-281,334-337 -- autograd sums the gradients of
    the passes AFTER all of them were produced, so each pass needs memory of its own), and not when a parameter still holds
    the buffer from an earlier backward (accumulation without zero_grad)."""
    if ent.store is None:
        return ent.peak > 1            # DDP bucket slots: zero-copy is only registered for single-pass models (hamspine.ddp)
    if ent.peak > 1:
        return True
    return any(p.grad is not None and p.grad.data_ptr() == ent.store.ptr(i) for i, p in enumerate(params))


def _tower_forward_begins(ctx, model, key, make_entry, params, needs, device):
    """-> the cached entry of `key` (make_entry() builds a missing or outdated one), a fresh saved arena, the workspace"""
    cache = model.__dict__.setdefault(_CACHE_ATTR, {})
    ent = cache.get(key)
    if ent is None or not ent.valid_for(params):
        ent = cache[key] = make_entry()
    rt.ensure_shadows(ent.shadow_groups)
    saved = torch.empty(ent.saved_bytes, dtype=torch.uint8, device=device)
    ctx.ent, ctx.saved_buf, ctx.params = ent, saved, params
    ctx.counted = _Pending(ent) if any(needs) else None      # a forward that will be backpropagated: its backward is pending
    return ent, saved, rt.workspace(ent.ws_bytes, device)


def _tower_backward(ctx, n_lead, call):
    """a tower node's backward: call(desc, saved, ws) makes its one C call; -> None for the n_lead leading inputs, then d(params)"""
    ent, saved, params = ctx.ent, ctx.saved_buf, ctx.params
    if saved is None:
        raise RuntimeError("hamspine.tower: backward through a tower a second time: its saved activations are freed by the "
                           "first backward (retain_graph=True is not supported on the tower nodes)")
    _ = ctx.saved_tensors                        # raises if an output was modified in place since the forward
    rt.wgrad_defer_flush_all()                   # the head path's deferred weight gradients: one grouped grid in front of the tower
    desc, views = ent.desc, ent.make_views
    if _shared_buffer_unsafe(ent, params):      # one-off private gradient buffers for this backward
        store = _GradStore(params, tuple(ctx.needs_input_grad[n_lead:]), saved.device)
        desc, views = DL.with_fresh_grads(ent.desc, store), store.views
    ws = rt.workspace(ent.ws_bytes, saved.device)
    if desc is ent.desc:
        _with_milestones(ent, params, lambda: call(desc, saved, ws))
    else:
        call(desc, saved, ws)
    ctx.saved_buf = None
    if ctx.counted is not None:
        ctx.counted.finish()
    return (*[None] * n_lead, *views())


class ResNetTowerFn(Function):
    """image (N,3,H,W) f32 -> the requested block outputs (NCHW-shaped, NHWC memory, compute dtype)"""

    @staticmethod
    def forward(ctx, image, holder, *params):
        model, taps, training = holder
        rt.need_gpu(image, *params)
        image = image.contiguous()
        if image.dtype != torch.float32:
            image = image.float()
        dtype = hamspine.compute_dtype()
        needs = tuple(ctx.needs_input_grad[2:])
        inference = not (training or any(needs))
        key = ("resnet", tuple(image.shape), dtype, training, inference, taps, needs)
        ent, saved, ws = _tower_forward_begins(
            ctx, model, key, lambda: _ResnetEntry(model, image.shape, dtype, training, inference, taps, params, needs, image.device),
            params, needs, image.device)
        L.check(L.lib().hs_resnet_fwd(C.byref(ent.desc), image.data_ptr(), saved.data_ptr(), saved.numel(), ws.data_ptr(),
                                      ws.numel(), rt.stream()), "hs_resnet_fwd")
        outs = [saved[off:off + n * h * w * c * es].view(dtype).view(n, h, w, c).permute(0, 3, 1, 2)
                for off, (n, h, w, c), es in ent.taps]
        if DEBUG_KEEP is not None:
            DEBUG_KEEP.append((ent, saved))
        # the outputs are views into the arena the backward reads (ReLU masks, BatchNorm inputs): registering them makes
        # autograd's version counters catch a consumer that modifies one in place (it would corrupt the backward silently)
        ctx.save_for_backward(*outs)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dys):
        dys = [None if dy is None else rt.as_cl(dy, ctx.ent.dtype) for dy in dys]
        ptrs = (C.c_void_p * len(dys))(*[None if dy is None else dy.data_ptr() for dy in dys])

        def call(desc, saved, ws):
            L.check(L.lib().hs_resnet_bwd(C.byref(desc), ptrs, saved.data_ptr(), saved.numel(), ws.data_ptr(), ws.numel(),
                                          rt.stream()), "hs_resnet_bwd")
        return _tower_backward(ctx, 2, call)


def resnet_taps(model, x, tap_layers):
    """run `model` (hamspine.nn.ResNet) up to layer4 through the tower executor; tap_layers: which of
    ("layer2", "layer3", "layer4") to return.  Returns None when the tower path does not apply (hooks, CPU)."""
    if not (towers_enabled() and x.is_cuda and x.dim() == 4 and x.shape[1] == 3):
        return None
    if _has_hooks(model):
        return None
    counts = [len(model.layer1), len(model.layer2), len(model.layer3), len(model.layer4)]
    ends = {"layer1": counts[0] - 1, "layer2": sum(counts[:2]) - 1, "layer3": sum(counts[:3]) - 1, "layer4": sum(counts) - 1}
    taps = tuple(ends[t] for t in tap_layers)
    params, bns = resnet_params(model)
    training = model.training
    if training:
        for bn in bns:
            bn.bump()
    return ResNetTowerFn.apply(x, (model, taps, training), *params)


# =====================================================================================================================
# BERT
# =====================================================================================================================
def bert_desc(model, B, Lq, dtype, training, pack_rows, params, grad_ptrs):
    """hs_bert_desc of `model` for one input shape and mode (no library call; seed is set per call)"""
    layers = model.encoder.layer
    if len(layers) > L.BERT_MAX_LAYERS:
        raise L.HamspineError(f"hamspine.tower: {len(layers)} BertLayers (max {L.BERT_MAX_LAYERS})")
    d = L.BertDesc()
    hd = rt.hs_dtype(dtype)
    e, H = model.embeddings, model.config.hidden_size
    d.dtype, d.B, d.L, d.hidden = hd, B, Lq, H
    d.vocab, d.max_pos, d.n_types = e.word_embeddings.weight.shape[0], e.position_embeddings.weight.shape[0], e.token_type_embeddings.weight.shape[0]
    d.pad_id = -1 if e.word_embeddings.padding_idx is None else int(e.word_embeddings.padding_idx)
    d.ln_eps, d.embed_dropout = float(e.LayerNorm.eps), float(e.dropout.p) if training else 0.0
    DL.fill_bert_embeddings(d, params[:len(DL.BERT_EMBED_SLOTS)])
    d.n_layers, d.pack_rows = len(layers), 1 if pack_rows else 0
    for i, layer in enumerate(layers):
        a, so = layer.attention.self, layer.attention.output
        DL.fill_bert_layer(d.layers[i], hd, B, Lq, H, layer._heads, layer._inter, float(so.LayerNorm.eps),
                          float(so.dropout.p) if training else 0.0, float(a.dropout.p) if training else 0.0,
                          params[DL.bert_layer_slice(i)])
    DL.set_grads(d, grad_ptrs)
    return d


class _BertEntry(_Entry):
    def __init__(self, model, B, Lq, dtype, training, params, needs, device, pack_rows=False):
        super().__init__(params, needs, device, dtype)
        self.pack_rows = bool(pack_rows)
        self.desc = bert_desc(model, B, Lq, dtype, training, pack_rows, params, self.grad_ptrs)
        sv, ws, off = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        L.check(L.lib().hs_bert_query(C.byref(self.desc), C.byref(sv), C.byref(ws), C.byref(off)), "hs_bert_query")
        self.saved_bytes, self.ws_bytes, self.out_off = sv.value, ws.value, off.value
        self.shape = (B, Lq, model.config.hidden_size)
        self.shadow_groups = DL.bert_shadow_groups(params, len(model.encoder.layer)) if dtype == torch.bfloat16 else []


class BertTowerFn(Function):
    """(input_ids, attention_mask) -> last_hidden_state (B, L, hidden) in the compute dtype"""

    @staticmethod
    def forward(ctx, ids, mask, holder, *params):
        model, training, pack_rows = holder
        rt.need_gpu(ids, mask, *params)
        ids = ids.contiguous()
        if ids.dtype != torch.int64:
            ids = ids.long()
        B, Lq = ids.shape
        if Lq > model.embeddings.position_embeddings.weight.shape[0]:
            raise ValueError(f"sequence length {Lq} exceeds max_position_embeddings")
        dtype = hamspine.compute_dtype()
        needs = tuple(ctx.needs_input_grad[3:])
        pack_rows = bool(pack_rows) and bert_pack_supported(model, B, Lq, dtype, mask, needs)
        key = ("bert", B, Lq, dtype, training, needs, pack_rows)
        ent, saved, ws = _tower_forward_begins(
            ctx, model, key, lambda: _BertEntry(model, B, Lq, dtype, training, params, needs, ids.device, pack_rows),
            params, needs, ids.device)
        seed = (rt.next_seed() * 64) & 0xFFFFFFFFFFFFFFFF if training else 0
        ent.desc.seed = seed
        L.check(L.lib().hs_bert_fwd(C.byref(ent.desc), ids.data_ptr(), rt.p(mask), saved.data_ptr(), saved.numel(),
                                    ws.data_ptr(), ws.numel(), rt.stream()), "hs_bert_fwd")
        Bq, Lq2, H = ent.shape
        es = 2 if dtype == torch.bfloat16 else 4
        out = saved[ent.out_off:ent.out_off + Bq * Lq2 * H * es].view(dtype).view(Bq, Lq2, H)
        ctx.seed, ctx.ids, ctx.mask = seed, ids, mask
        ctx.save_for_backward(out)                  # a view into the arena: in-place edits by a consumer are caught at backward
        return out

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        if dy.dtype != ctx.ent.dtype:
            dy = dy.to(ctx.ent.dtype)

        def call(desc, saved, ws):
            desc.seed = ctx.seed
            L.check(L.lib().hs_bert_bwd(C.byref(desc), ctx.ids.data_ptr(), rt.p(ctx.mask), dy.data_ptr(), saved.data_ptr(),
                                        saved.numel(), ws.data_ptr(), ws.numel(), rt.stream()), "hs_bert_bwd")
        return _tower_backward(ctx, 3, call)       # bert_params order: the backward finishes params[0] (embeddings) last


def bert_pack_supported(model, B, Lq, dtype, mask, needs=None):
    """whether the tower can run on the valid tokens only (hs_bert_desc.pack_rows): bf16, head dim 64, at most 128 tokens (the
    packed fused-attention kernels), a mask to take the rows from, the q / k / v weights of a layer all trained or all frozen
    (their gradients come from one fused GEMM; `needs` = needs_input_grad of bert_params(model)), and the library's latched
    switches leaving it its kernels (hs_bert_pack_rows_available: asked of the library, so the two sides cannot disagree).
    HAMSPINE_BERT_PACK=0 forces the padded path (read on every call: it is the A/B switch).  Anything else: the padded tower,
    silently."""
    if os.environ.get("HAMSPINE_BERT_PACK", "1") == "0" or mask is None or dtype != torch.bfloat16:
        return False
    if not L.lib().hs_bert_pack_rows_available():
        return False
    c = model.config
    H = c.hidden_size
    if Lq > 128 or (B * Lq) % 8 != 0 or H % 8 != 0:
        return False
    if needs is not None and not DL.qkv_trained_together(needs, len(model.encoder.layer)):
        return False
    return all(H == 64 * layer._heads and layer._inter % 8 == 0 for layer in model.encoder.layer)


def bert_ran_packed(hidden):
    """whether the tower call that produced `hidden` (a last_hidden_state that still carries its autograd node) ran on packed
    rows; None when it did not come from the tower executor"""
    ent = getattr(getattr(hidden, "grad_fn", None), "ent", None)
    return getattr(ent, "pack_rows", None)


def bert_hidden(model, input_ids, attention_mask, skip_padded_rows=False):
    """last_hidden_state of `model` (hamspine.nn.BertModel) through the tower executor, or None when it does not apply.

    skip_padded_rows: compute only the tokens whose attention_mask is non-zero (see hs_bert_desc.pack_rows in
    include/hamspine.h).  The result then holds ZEROS at masked positions and the backward ignores the cotangent there, so only a
    consumer that never reads those positions (a key-masked attention) may ask for it.  For right-padded masks every dropout draw
    is the padded path's; for masks with holes the attention-probability draws differ (their index counts keys in packed order).
    Shapes the packed kernels do not cover take the padded path."""
    if not (towers_enabled() and input_ids.is_cuda and input_ids.dim() == 2):
        return None
    if _has_hooks(model):
        return None
    return BertTowerFn.apply(input_ids, attention_mask, (model, model.training, bool(skip_padded_rows)), *bert_params(model))
