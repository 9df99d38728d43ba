"""Layout of the composite descriptors of the C ABI (hs_conv_bn, hs_stem_desc, hs_resblock_desc, hs_linear, hs_bert_layer_desc,
hs_resnet_desc, hs_bert_desc): which parameter fills which field, written once for the per-block autograd nodes
(hamspine.functional) and the whole-tower executors (hamspine.tower), a tower descriptor being an array of block descriptors.
The order of a composite's parameters (the argument order of its node, hence of its gradients) is read off the tables here; a
new descriptor field or parameter is added in this file.  Pure: struct classes come from hamspine._lib, the library is never
loaded and no device is asked anything -- a CPU tensor's data_ptr() fills a descriptor as well as any.
"""
import ctypes as C
import operator

from . import _lib as L

# one conv + BatchNorm pair: (field of hs_conv_bn, its gradient field) of conv.weight, bn.weight, bn.bias
CONV_BN_SLOTS = (("w", "dw"), ("gamma", "dgamma"), ("beta", "dbeta"))

# one BertLayer: (parameter as reached from the module, member of hs_bert_layer_desc it fills, that member's gradient field)
BERT_LAYER_SLOTS = (
    ("attention.self.query.weight", "q.w", "q.dw"),
    ("attention.self.query.bias", "q.b", "q.db"),
    ("attention.self.key.weight", "k.w", "k.dw"),
    ("attention.self.key.bias", "k.b", "k.db"),
    ("attention.self.value.weight", "v.w", "v.dw"),
    ("attention.self.value.bias", "v.b", "v.db"),
    ("attention.output.dense.weight", "ao.w", "ao.dw"),
    ("attention.output.dense.bias", "ao.b", "ao.db"),
    ("attention.output.LayerNorm.weight", "ln1.gamma", "ln1.dgamma"),
    ("attention.output.LayerNorm.bias", "ln1.beta", "ln1.dbeta"),
    ("intermediate.dense.weight", "inter_l.w", "inter_l.dw"),
    ("intermediate.dense.bias", "inter_l.b", "inter_l.db"),
    ("output.dense.weight", "out_l.w", "out_l.dw"),
    ("output.dense.bias", "out_l.b", "out_l.db"),
    ("output.LayerNorm.weight", "ln2.gamma", "ln2.dgamma"),
    ("output.LayerNorm.bias", "ln2.beta", "ln2.dbeta"),
)

# the embeddings of a BertModel: (parameter as reached from the model, field of hs_bert_desc, its gradient field)
BERT_EMBED_SLOTS = (
    ("embeddings.word_embeddings.weight", "word", "dword"),
    ("embeddings.position_embeddings.weight", "pos", "dpos"),
    ("embeddings.token_type_embeddings.weight", "type0", "dtype0"),
    ("embeddings.LayerNorm.weight", "gamma", "dgamma"),
    ("embeddings.LayerNorm.bias", "beta", "dbeta"),
)

# the BertLayer table resolved once at import (the per-block nodes build a descriptor on every call): the parameter-owning
# modules, each fetched once per call; every parameter as (module number, attribute) and as (member, field, gradient field)
_LAYER_MODULES, _LAYER_LEAVES, _LAYER_FIELDS = [], [], []
for _path, _field, _grad in BERT_LAYER_SLOTS:
    _module, _, _leaf = _path.rpartition(".")
    if _module not in _LAYER_MODULES:
        _LAYER_MODULES.append(_module)
    _LAYER_LEAVES.append((_LAYER_MODULES.index(_module), _leaf))
    _LAYER_FIELDS.append((*_field.split("."), _grad.split(".")[1]))
_layer_modules = operator.attrgetter(*_LAYER_MODULES)
_embed_params = operator.attrgetter(*(path for path, _, _ in BERT_EMBED_SLOTS))
# positions, among a layer's parameters, of the Linear weights and of q / k / v among them (one fused weight-gradient GEMM)
_LAYER_W = [i for i, (_, field, _) in enumerate(_LAYER_FIELDS) if field == "w"]
BERT_QKV_W = [i for i in _LAYER_W if _LAYER_FIELDS[i][0] in ("q", "k", "v")]


def _p(t, byte_offset=0):
    return None if t is None else t.data_ptr() + byte_offset


def block_pairs(block):
    """(conv, bn) of a residual block's main stages, then of its downsample branch when it has one"""
    ds = block.downsample
    return block._pairs() + ([(ds[0], ds[1])] if ds is not None else [])


def conv_bn_params(conv, bn):
    return [conv.weight, bn.weight, bn.bias]


def conv_bn_triples(params):
    """a flat list of conv + BatchNorm parameters as (w, gamma, beta) tuples"""
    return list(zip(*[iter(params)] * len(CONV_BN_SLOTS)))


def resnet_shadow_groups(params):
    """bf16 shadows of resnet_params(model): every block filter on its own (the stem's filter is re-packed, not cast)"""
    return [[w] for w, _, _ in conv_bn_triples(params)[1:]]


def bn_momentum(bn):
    return bn.momentum if bn.momentum is not None else 0.1


def bert_layer_params(layer):
    mods = _layer_modules(layer)
    return [getattr(mods[m], leaf) for m, leaf in _LAYER_LEAVES]


def bert_params(model):
    """the embeddings' parameters, then every layer's"""
    return [p for ps in (_embed_params(model), *map(bert_layer_params, model.encoder.layer)) for p in ps]


def bert_layer_slice(i):
    """where layer i's parameters sit in bert_params(model)"""
    return slice(len(BERT_EMBED_SLOTS) + len(BERT_LAYER_SLOTS) * i, len(BERT_EMBED_SLOTS) + len(BERT_LAYER_SLOTS) * (i + 1))


def bert_shadow_groups(params, n_layers):
    """bf16 shadows of bert_params(model): per layer q, k, v as the segments of one buffer (the fused [3H][H] weight), the rest singly"""
    layers = [params[bert_layer_slice(i)] for i in range(n_layers)]
    return [g for ps in layers for g in [[ps[k] for k in BERT_QKV_W]] + [[ps[k]] for k in _LAYER_W if k not in BERT_QKV_W]]


def qkv_trained_together(needs, n_layers):
    """`needs` = needs_input_grad of bert_params(model): the q / k / v weights of every layer are all trained or all frozen"""
    qkv = [[bool(needs[bert_layer_slice(i).start + k]) for k in BERT_QKV_W] for i in range(n_layers)]
    return all(all(q) or not any(q) for q in qkv)


def conv_out(h, R, stride, pad):
    return (h + 2 * pad - R) // stride + 1


def stem_out(h):
    """conv7x7/2 pad 3, then maxpool3x3/2 pad 1"""
    return conv_out(conv_out(h, 7, 2, 3), 3, 2, 1)


# The fill functions write into a zeroed struct (a fresh one, or a member of a fresh tower descriptor); set_grads adds the gradients.
def fill_conv_bn(cb, geo, w, gamma, beta, running_mean, running_var):
    cb.Cin, cb.Cout, cb.R, cb.stride, cb.pad = geo
    cb.w, cb.gamma, cb.beta = _p(w), _p(gamma), _p(beta)
    cb.running_mean, cb.running_var = _p(running_mean), _p(running_var)


def fill_stem(d, dtype, N, H, W, training, eps, momentum, geo, w, gamma, beta, running_mean, running_var, inference=False):
    d.dtype, d.N, d.H, d.W = dtype, N, H, W
    d.training, d.eps, d.momentum, d.inference = int(training), eps, momentum, int(inference)
    fill_conv_bn(d.cb, geo, w, gamma, beta, running_mean, running_var)


def fill_resblock(d, dtype, N, H, W, training, eps, momentum, stages, has_ds, inference=False):
    """stages: (geo, w, gamma, beta, running_mean, running_var) of every main stage, then of the downsample pair if has_ds"""
    d.dtype, d.N, d.H, d.W = dtype, N, H, W
    d.training, d.eps, d.momentum, d.inference = int(training), eps, momentum, int(inference)
    d.n_main, d.has_ds = len(stages) - int(has_ds), int(has_ds)
    for i, st in enumerate(stages):
        fill_conv_bn(d.main[i] if i < d.n_main else d.ds, *st)


def linear(in_f, out_f, w, b, dw=None, db=None, w_off=0, b_off=0):
    """a fresh hs_linear; w_off / b_off: element offsets into w, b and their gradients (one projection of a packed weight)"""
    l = L.Linear()
    l.in_f, l.out_f = in_f, out_f
    l.w, l.b, l.dw, l.db = _p(w, w_off * 4), _p(b, b_off * 4), _p(dw, w_off * 4), _p(db, b_off * 4)
    return l


def fill_bert_layer(d, dtype, B, Lq, hidden, heads, inter, ln_eps, hidden_dropout, attn_dropout, params):
    """params: the layer's parameters in BERT_LAYER_SLOTS order; seed and attention_mask are the caller's"""
    d.dtype, d.B, d.L, d.hidden, d.heads, d.inter = dtype, B, Lq, hidden, heads, inter
    d.ln_eps, d.hidden_dropout, d.attn_dropout = ln_eps, hidden_dropout, attn_dropout
    for (member, field, _), p in zip(_LAYER_FIELDS, params):
        s = getattr(d, member)
        setattr(s, field, p.data_ptr())
        if field == "w":
            s.out_f, s.in_f = p.shape                         # an hs_linear; nn.Linear keeps [out][in]


def fill_bert_embeddings(d, params):
    """params: the embeddings' parameters in BERT_EMBED_SLOTS order"""
    for (_, field, _), p in zip(BERT_EMBED_SLOTS, params):
        setattr(d, field, p.data_ptr())


def _grad_fields(d):
    """(struct, gradient field) of every parameter of the descriptor `d`, in the composite's parameter order.  Built flat, no
    recursion: a tower that runs twice in one graph walks its descriptor on every backward (with_fresh_grads)."""
    own, layers, cbs, blocks = [], [], [], []
    if isinstance(d, L.ResblockDesc):                          # (the per-call types first)
        blocks = [d]
    elif isinstance(d, L.BertLayerDesc):
        layers = [d]
    elif isinstance(d, L.StemDesc):
        cbs = [d.cb]
    elif isinstance(d, L.ResnetDesc):
        cbs, blocks = [d.stem.cb], [d.blocks[i] for i in range(d.n_blocks)]
    else:
        own, layers = [(d, g) for _, _, g in BERT_EMBED_SLOTS], [d.layers[i] for i in range(d.n_layers)]
    cbs += [cb for b in blocks for cb in [b.main[j] for j in range(b.n_main)] + [b.ds] * b.has_ds]
    return (own + [(cb, g) for cb in cbs for _, g in CONV_BN_SLOTS]
            + [(getattr(ld, member), g) for ld in layers for member, _, g in _LAYER_FIELDS])


def set_grads(desc, ptrs):
    """assign every gradient field of `desc` from the flat list `ptrs` (addresses, None = frozen), in parameter order"""
    slots = _grad_fields(desc)
    if len(slots) != len(ptrs):
        raise L.HamspineError(f"hamspine.desc: {len(ptrs)} gradient pointers for {len(slots)} gradient fields")
    for (s, g), q in zip(slots, ptrs):
        setattr(s, g, q)


def with_fresh_grads(desc, store):
    """a copy of `desc` whose gradients go to the slots of `store` (ptr(i) of parameter i); `desc` is left as it is"""
    d = type(desc)()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(d))
    set_grads(d, [store.ptr(i) for i in range(len(store.slots))])
    return d
