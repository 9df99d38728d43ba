"""hamspine.desc on the host: every pointer of a stem / residual-block / BertLayer / tower descriptor sits in the field its
state-dict name says, the tower executors and the per-block nodes fill the same values, and the gradient walkers address
every gradient field in parameter order.  No library and no GPU: a CPU tensor's data_ptr() fills a descriptor as well as any.

What is expected is stated here by state-dict name, not through the tables of hamspine.desc."""
import ctypes

import pytest
import torch

import hamspine
from hamspine import _lib as L
from hamspine import desc as D
from hamspine import functional as F
from hamspine import tower
from hamspine.nn import bert, resnet

IMAGE = (2, 3, 32, 32)
B, LQ = 2, 16
# side of the (square) input of every residual block for a 32 x 32 image: 8 after the stem, halved by layer2.0, 3.0, 4.0
BLOCK_INPUT = {"resnet18": [8, 8, 8, 4, 4, 2, 2, 1], "resnet50": [8, 8, 8, 8, 4, 4, 4, 4, 2, 2, 2, 2, 2, 2, 1, 1]}
LAYERS = {"resnet18": [2, 2, 2, 2], "resnet50": [3, 4, 6, 3]}
N_MAIN = {"resnet18": 2, "resnet50": 3}
GRAD_OF = {"w": "dw", "b": "db", "gamma": "dgamma", "beta": "dbeta", "word": "dword", "pos": "dpos", "type0": "dtype0"}

STEM = {"stem.cb.w": "conv1.weight", "stem.cb.gamma": "bn1.weight", "stem.cb.beta": "bn1.bias",
        "stem.cb.running_mean": "bn1.running_mean", "stem.cb.running_var": "bn1.running_var"}
# resnet18: the first block (no downsample) and the first downsample block, layer2.0 = block 2
RESNET18_NAMED = {
    **STEM,
    "blocks[0].main[0].w": "layer1.0.conv1.weight", "blocks[0].main[0].gamma": "layer1.0.bn1.weight",
    "blocks[0].main[0].beta": "layer1.0.bn1.bias", "blocks[0].main[0].running_mean": "layer1.0.bn1.running_mean",
    "blocks[0].main[0].running_var": "layer1.0.bn1.running_var",
    "blocks[0].main[1].w": "layer1.0.conv2.weight", "blocks[0].main[1].gamma": "layer1.0.bn2.weight",
    "blocks[0].main[1].beta": "layer1.0.bn2.bias", "blocks[0].main[1].running_mean": "layer1.0.bn2.running_mean",
    "blocks[0].main[1].running_var": "layer1.0.bn2.running_var",
    "blocks[2].main[0].w": "layer2.0.conv1.weight", "blocks[2].main[0].gamma": "layer2.0.bn1.weight",
    "blocks[2].main[0].beta": "layer2.0.bn1.bias", "blocks[2].main[0].running_mean": "layer2.0.bn1.running_mean",
    "blocks[2].main[0].running_var": "layer2.0.bn1.running_var",
    "blocks[2].main[1].w": "layer2.0.conv2.weight", "blocks[2].main[1].gamma": "layer2.0.bn2.weight",
    "blocks[2].main[1].beta": "layer2.0.bn2.bias", "blocks[2].main[1].running_mean": "layer2.0.bn2.running_mean",
    "blocks[2].main[1].running_var": "layer2.0.bn2.running_var",
    "blocks[2].ds.w": "layer2.0.downsample.0.weight", "blocks[2].ds.gamma": "layer2.0.downsample.1.weight",
    "blocks[2].ds.beta": "layer2.0.downsample.1.bias", "blocks[2].ds.running_mean": "layer2.0.downsample.1.running_mean",
    "blocks[2].ds.running_var": "layer2.0.downsample.1.running_var",
}
# resnet50: the first block is a Bottleneck with a downsample pair
RESNET50_NAMED = {
    **STEM,
    "blocks[0].main[0].w": "layer1.0.conv1.weight", "blocks[0].main[0].gamma": "layer1.0.bn1.weight",
    "blocks[0].main[0].beta": "layer1.0.bn1.bias", "blocks[0].main[0].running_mean": "layer1.0.bn1.running_mean",
    "blocks[0].main[0].running_var": "layer1.0.bn1.running_var",
    "blocks[0].main[1].w": "layer1.0.conv2.weight", "blocks[0].main[1].gamma": "layer1.0.bn2.weight",
    "blocks[0].main[1].beta": "layer1.0.bn2.bias", "blocks[0].main[1].running_mean": "layer1.0.bn2.running_mean",
    "blocks[0].main[1].running_var": "layer1.0.bn2.running_var",
    "blocks[0].main[2].w": "layer1.0.conv3.weight", "blocks[0].main[2].gamma": "layer1.0.bn3.weight",
    "blocks[0].main[2].beta": "layer1.0.bn3.bias", "blocks[0].main[2].running_mean": "layer1.0.bn3.running_mean",
    "blocks[0].main[2].running_var": "layer1.0.bn3.running_var",
    "blocks[0].ds.w": "layer1.0.downsample.0.weight", "blocks[0].ds.gamma": "layer1.0.downsample.1.weight",
    "blocks[0].ds.beta": "layer1.0.downsample.1.bias", "blocks[0].ds.running_mean": "layer1.0.downsample.1.running_mean",
    "blocks[0].ds.running_var": "layer1.0.downsample.1.running_var",
}
BERT_NAMED = {
    "word": "embeddings.word_embeddings.weight", "pos": "embeddings.position_embeddings.weight",
    "type0": "embeddings.token_type_embeddings.weight", "gamma": "embeddings.LayerNorm.weight", "beta": "embeddings.LayerNorm.bias",
    "layers[0].q.w": "encoder.layer.0.attention.self.query.weight", "layers[0].q.b": "encoder.layer.0.attention.self.query.bias",
    "layers[0].k.w": "encoder.layer.0.attention.self.key.weight", "layers[0].k.b": "encoder.layer.0.attention.self.key.bias",
    "layers[0].v.w": "encoder.layer.0.attention.self.value.weight", "layers[0].v.b": "encoder.layer.0.attention.self.value.bias",
    "layers[0].ao.w": "encoder.layer.0.attention.output.dense.weight", "layers[0].ao.b": "encoder.layer.0.attention.output.dense.bias",
    "layers[0].ln1.gamma": "encoder.layer.0.attention.output.LayerNorm.weight",
    "layers[0].ln1.beta": "encoder.layer.0.attention.output.LayerNorm.bias",
    "layers[0].inter_l.w": "encoder.layer.0.intermediate.dense.weight", "layers[0].inter_l.b": "encoder.layer.0.intermediate.dense.bias",
    "layers[0].out_l.w": "encoder.layer.0.output.dense.weight", "layers[0].out_l.b": "encoder.layer.0.output.dense.bias",
    "layers[0].ln2.gamma": "encoder.layer.0.output.LayerNorm.weight", "layers[0].ln2.beta": "encoder.layer.0.output.LayerNorm.bias",
    "layers[1].q.w": "encoder.layer.1.attention.self.query.weight", "layers[1].q.b": "encoder.layer.1.attention.self.query.bias",
    "layers[1].k.w": "encoder.layer.1.attention.self.key.weight", "layers[1].k.b": "encoder.layer.1.attention.self.key.bias",
    "layers[1].v.w": "encoder.layer.1.attention.self.value.weight", "layers[1].v.b": "encoder.layer.1.attention.self.value.bias",
    "layers[1].ao.w": "encoder.layer.1.attention.output.dense.weight", "layers[1].ao.b": "encoder.layer.1.attention.output.dense.bias",
    "layers[1].ln1.gamma": "encoder.layer.1.attention.output.LayerNorm.weight",
    "layers[1].ln1.beta": "encoder.layer.1.attention.output.LayerNorm.bias",
    "layers[1].inter_l.w": "encoder.layer.1.intermediate.dense.weight", "layers[1].inter_l.b": "encoder.layer.1.intermediate.dense.bias",
    "layers[1].out_l.w": "encoder.layer.1.output.dense.weight", "layers[1].out_l.b": "encoder.layer.1.output.dense.bias",
    "layers[1].ln2.gamma": "encoder.layer.1.output.LayerNorm.weight", "layers[1].ln2.beta": "encoder.layer.1.output.LayerNorm.bias",
}
# the order in which a BertModel's parameters are handed to its nodes, hence of its gradient pointers
BERT_LAYER_ORDER = ["attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight",
                    "attention.self.key.bias", "attention.self.value.weight", "attention.self.value.bias",
                    "attention.output.dense.weight", "attention.output.dense.bias", "attention.output.LayerNorm.weight",
                    "attention.output.LayerNorm.bias", "intermediate.dense.weight", "intermediate.dense.bias",
                    "output.dense.weight", "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias"]
BERT_ORDER = (["embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight",
               "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
              + [f"encoder.layer.{i}.{n}" for i in range(2) for n in BERT_LAYER_ORDER])


def _resnet_named(arch):
    """field -> state-dict key of every block of the tower, by torchvision's naming"""
    named, order = dict(STEM), ["conv1.weight", "bn1.weight", "bn1.bias"]
    blocks = [f"layer{s + 1}.{j}" for s, n in enumerate(LAYERS[arch]) for j in range(n)]
    for i, name in enumerate(blocks):
        pairs = [(f"blocks[{i}].main[{k}]", f"{name}.conv{k + 1}", f"{name}.bn{k + 1}") for k in range(N_MAIN[arch])]
        if name.endswith(".0") and (arch == "resnet50" or not name.startswith("layer1")):
            pairs.append((f"blocks[{i}].ds", f"{name}.downsample.0", f"{name}.downsample.1"))
        for field, conv, bn in pairs:
            named.update({f"{field}.w": f"{conv}.weight", f"{field}.gamma": f"{bn}.weight", f"{field}.beta": f"{bn}.bias",
                          f"{field}.running_mean": f"{bn}.running_mean", f"{field}.running_var": f"{bn}.running_var"})
            order += [f"{conv}.weight", f"{bn}.weight", f"{bn}.bias"]
    return named, order


def _get(d, path):
    for part in path.split("."):
        name, _, index = part.partition("[")
        d = getattr(d, name)
        if index:
            d = d[int(index[:-1])]
    return d


def _fields(s, prefix=""):
    """{dotted path: value} of every scalar / pointer field of a ctypes struct, nested structs and arrays included"""
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, ctypes.Structure):
            out.update(_fields(v, f"{prefix}{name}."))
        elif isinstance(v, ctypes.Array):
            for i, e in enumerate(v):
                out.update(_fields(e, f"{prefix}{name}[{i}].") if isinstance(e, ctypes.Structure) else {f"{prefix}{name}[{i}]": e})
        else:
            out[prefix + name] = v
    return out


def _is_grad(path):
    return path.rpartition(".")[2] in GRAD_OF.values()


def _fake_ptrs(n):
    return [0x10000 + 64 * i for i in range(n)]


def _check_named(d, state, named, params, order, ptrs):
    """every named field holds its tensor's address; its gradient field holds the address at its parameter's index"""
    index = {id(p): i for i, p in enumerate(params)}
    assert [index[id(state[k])] for k in order] == list(range(len(params))), "parameter order"
    for field, key in named.items():
        assert _get(d, field) == state[key].data_ptr(), (field, key)
        leaf = field.rpartition(".")[2]
        if leaf in GRAD_OF:
            grad = field[:len(field) - len(leaf)] + GRAD_OF[leaf]
            assert _get(d, grad) == ptrs[order.index(key)], (grad, key)


@pytest.fixture(scope="module", params=["resnet18", "resnet50"])
def image_tower(request):
    torch.manual_seed(0)
    model = getattr(resnet, request.param)().train()
    params, _ = tower.resnet_params(model)
    ptrs = _fake_ptrs(len(params))
    d = tower.resnet_desc(model, IMAGE, torch.float32, True, False, (len(tower.resnet_blocks(model)) - 1,), ptrs)
    return request.param, model, params, ptrs, d


@pytest.fixture(scope="module")
def text_tower():
    torch.manual_seed(0)
    cfg = bert.BertConfig(vocab_size=50, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256)
    model = bert.BertModel(cfg).train()
    params = tower.bert_params(model)
    ptrs = _fake_ptrs(len(params))
    d = tower.bert_desc(model, B, LQ, torch.float32, True, False, params, ptrs)
    return model, params, ptrs, d


def _state(model):
    return dict(model.state_dict(keep_vars=True))


# ------------------------------------------------------------------------------------------------ named pointers
def test_resnet_named_pointers(image_tower):
    arch, model, params, ptrs, d = image_tower
    named, order = _resnet_named(arch)
    literal = RESNET18_NAMED if arch == "resnet18" else RESNET50_NAMED
    assert all(named[f] == k for f, k in literal.items()), "the naming rule of this test and its literal pairs disagree"
    assert len(order) == len(params)
    _check_named(d, _state(model), {**named, **literal}, params, order, ptrs)
    assert d.n_blocks == len(BLOCK_INPUT[arch]) and [d.blocks[i].H for i in range(d.n_blocks)] == BLOCK_INPUT[arch]
    assert [d.blocks[i].has_ds for i in range(d.n_blocks)] == [int(f"blocks[{i}].ds.w" in named) for i in range(d.n_blocks)]
    assert len([f for f, v in _fields(d).items() if _is_grad(f) and v is not None]) == len(params), "a gradient field outside the walk"


def test_bert_named_pointers(text_tower):
    model, params, ptrs, d = text_tower
    assert len(BERT_ORDER) == len(params) == 37
    _check_named(d, _state(model), BERT_NAMED, params, BERT_ORDER, ptrs)
    assert (d.n_layers, d.hidden, d.vocab, d.B, d.L) == (2, 128, 50, B, LQ)
    for i in range(2):
        ld = d.layers[i]
        assert [(l.in_f, l.out_f) for l in (ld.q, ld.k, ld.v, ld.ao, ld.inter_l, ld.out_l)] == [(128, 128)] * 4 + [(128, 256), (256, 128)]
        assert (ld.hidden, ld.heads, ld.inter) == (128, 2, 256)
    assert len([f for f, v in _fields(d).items() if _is_grad(f) and v is not None]) == len(params), "a gradient field outside the walk"


# ------------------------------------------------------------------------------------------------ tower == block node
def _node_args(monkeypatch, fn, module, *inputs):
    """what `module`'s forward hands to its autograd node `fn` (fn.apply is replaced: nothing runs)"""
    monkeypatch.setattr(fn, "apply", lambda *args: args)
    return module(*inputs)


@pytest.mark.parametrize("training", [True, False])
def test_resnet_tower_blocks_equal_block_nodes(image_tower, training, monkeypatch):
    arch, model, params, _, _ = image_tower
    model.train(training)
    try:
        d = tower.resnet_desc(model, IMAGE, hamspine.compute_dtype(), training, False, (0,), [None] * len(params))
        for i, block in enumerate(tower.resnet_blocks(model)):
            side = BLOCK_INPUT[arch][i]
            x, cfg, *ps = _node_args(monkeypatch, F.ResBlockFn, block, torch.zeros(IMAGE[0], block.conv1.in_channels, side, side))
            node = F.ResBlockFn._desc(cfg, x.shape, ps)
            assert _fields(node) == _fields(d.blocks[i]), f"block {i}"
    finally:
        model.train()


@pytest.mark.parametrize("training", [True, False])
def test_bert_tower_layers_equal_layer_nodes(text_tower, training, monkeypatch):
    model, params, _, _ = text_tower
    model.train(training)
    try:
        d = tower.bert_desc(model, B, LQ, hamspine.compute_dtype(), training, False, params, [None] * len(params))
        x = torch.zeros(B, LQ, 128)
        for i, layer in enumerate(model.encoder.layer):
            _, mask, cfg, *ps = _node_args(monkeypatch, F.BertLayerFn, layer, x, None)
            node = _fields(F.BertLayerFn._desc(cfg, x, mask, ps, 1234))
            want = _fields(d.layers[i])
            assert node.pop("seed") == 1234 and want.pop("seed") == 0       # the tower sets seed and mask per call
            assert node.pop("attention_mask") is None and want.pop("attention_mask") is None
            assert node == want, f"layer {i}"
            assert (want["hidden_dropout"] > 0) == training and (want["attn_dropout"] > 0) == training
    finally:
        model.train()


# ------------------------------------------------------------------------------------------------ set_grads, with_fresh_grads
def _check_fresh(d, params, needs):
    before = bytes(d)
    store = tower._GradStore(params, needs, torch.device("cpu"))
    fresh = D.with_fresh_grads(d, store)
    assert bytes(d) == before, "the original descriptor changed"
    old, new = _fields(d), _fields(fresh)
    assert {f: v for f, v in old.items() if not _is_grad(f)} == {f: v for f, v in new.items() if not _is_grad(f)}
    return store, fresh


def test_resnet_fresh_grads(image_tower):
    arch, model, params, ptrs, d = image_tower
    named, order = _resnet_named(arch)
    needs = [True] * len(params)
    store, fresh = _check_fresh(d, params, needs)
    _check_named(fresh, _state(model), named, params, order, [store.ptr(i) for i in range(len(params))])
    assert len({store.ptr(i) for i in range(len(params))}) == len(params)


def test_bert_fresh_grads(text_tower):
    model, params, ptrs, d = text_tower
    store, fresh = _check_fresh(d, params, [True] * len(params))
    _check_named(fresh, _state(model), BERT_NAMED, params, BERT_ORDER, [store.ptr(i) for i in range(len(params))])


def test_block_and_layer_set_grads(image_tower, text_tower, monkeypatch):
    """the per-block backward's use: one flat list per composite, in the order of its node's parameters"""
    arch, model, _, _, _ = image_tower
    block = model.layer2[0]
    x, cfg, *ps = _node_args(monkeypatch, F.ResBlockFn, block, torch.zeros(2, block.conv1.in_channels, 8, 8))
    d = F.ResBlockFn._desc(cfg, x.shape, ps, forward=False)
    assert all(v is None for f, v in _fields(d).items() if _is_grad(f) or "running" in f)
    ptrs = _fake_ptrs(len(ps))
    D.set_grads(d, ptrs)
    n = N_MAIN[arch]
    got = [(cb.dw, cb.dgamma, cb.dbeta) for cb in [d.main[k] for k in range(n)] + [d.ds]]
    assert [q for t in got for q in t] == ptrs and d.has_ds == 1 and d.n_main == n
    with pytest.raises(L.HamspineError):
        D.set_grads(d, ptrs[:-1])
    stem = L.StemDesc()            # the stem's backward form: no running statistics, inference off
    D.fill_stem(stem, L.HS_F32, 2, 32, 32, True, 1e-5, 0.1, (3, 64, 7, 2, 3), model.conv1.weight, model.bn1.weight, model.bn1.bias, None, None)
    D.set_grads(stem, [11, 22, 33])
    assert (stem.cb.dw, stem.cb.dgamma, stem.cb.dbeta) == (11, 22, 33) and stem.cb.running_mean is None and stem.inference == 0
    assert stem.cb.w == model.conv1.weight.data_ptr() and stem.cb.beta == model.bn1.bias.data_ptr()
    bmodel = text_tower[0]
    layer = bmodel.encoder.layer[1]
    x, mask, cfg, *ps = _node_args(monkeypatch, F.BertLayerFn, layer, torch.zeros(B, LQ, 128), None)
    ld = F.BertLayerFn._desc(cfg, x, mask, ps, 7)
    ptrs = _fake_ptrs(16)
    D.set_grads(ld, ptrs)
    assert [ld.q.dw, ld.q.db, ld.k.dw, ld.k.db, ld.v.dw, ld.v.db, ld.ao.dw, ld.ao.db, ld.ln1.dgamma, ld.ln1.dbeta,
            ld.inter_l.dw, ld.inter_l.db, ld.out_l.dw, ld.out_l.db, ld.ln2.dgamma, ld.ln2.dbeta] == ptrs


# ------------------------------------------------------------------------------------------------ frozen parameters
def test_resnet_frozen_parameters(image_tower):
    arch, model, params, _, _ = image_tower
    state = _state(model)
    frozen = {"conv1.weight", "layer1.0.bn1.bias", "layer2.0.downsample.0.weight", "layer4.1.conv2.weight"}
    needs = [not any(p is state[k] for k in frozen) for p in params]
    assert needs.count(False) == len(frozen)
    store, ptrs, _ = tower._param_grad_ptrs(params, needs, torch.device("cpu"))
    assert [s is None for s in store.slots] == [not n for n in needs]
    d = tower.resnet_desc(model, IMAGE, torch.float32, True, False, (0,), ptrs)
    ds = "blocks[2].ds.dw" if arch == "resnet18" else "blocks[3].ds.dw"
    last = "blocks[7].main[1].dw" if arch == "resnet18" else "blocks[14].main[1].dw"
    for field in ("stem.cb.dw", "blocks[0].main[0].dbeta", ds, last):
        assert _get(d, field) is None, field
    assert len([f for f, v in _fields(d).items() if _is_grad(f) and v is not None]) == len(params) - len(frozen)
    assert _get(d, "stem.cb.dgamma") == store.ptr(1) and _get(d, "blocks[0].main[0].dw") == store.ptr(3)


def test_bert_frozen_parameters_and_pack_rule(text_tower):
    model, params, _, _ = text_tower
    state = _state(model)

    def needs_without(*keys):
        return [not any(p is state[k] for k in keys) for p in params]

    k1, v1 = "encoder.layer.1.attention.self.key.weight", "encoder.layer.1.attention.self.value.weight"
    q1 = "encoder.layer.1.attention.self.query.weight"
    needs = needs_without(k1, v1, "embeddings.word_embeddings.weight")
    store, ptrs, _ = tower._param_grad_ptrs(params, needs, torch.device("cpu"))
    assert [s is None for s in store.slots] == [not n for n in needs] and needs.count(False) == 3
    d = tower.bert_desc(model, B, LQ, torch.float32, True, False, params, ptrs)
    assert d.dword is None and d.layers[1].k.dw is None and d.layers[1].v.dw is None
    assert d.layers[1].q.dw == store.ptr(BERT_ORDER.index(q1)) and d.layers[1].k.db == store.ptr(BERT_ORDER.index(k1.replace("weight", "bias")))
    assert len([f for f, v in _fields(d).items() if _is_grad(f) and v is not None]) == len(params) - 3
    # q trained, k and v frozen: the fused q/k/v weight gradient cannot serve the layer, so the packed tower is refused
    assert not D.qkv_trained_together(needs, 2)
    assert D.qkv_trained_together([True] * len(params), 2)
    assert D.qkv_trained_together(needs_without(q1, k1, v1), 2)                      # all three frozen
    assert D.qkv_trained_together(needs_without(q1.replace("weight", "bias")), 2)    # a bias does not matter
    assert not D.qkv_trained_together(needs_without("encoder.layer.0.attention.self.query.weight"), 2)


# ------------------------------------------------------------------------------------------------ shadow groups
def test_shadow_groups(image_tower, text_tower):
    arch, model, params, _, _ = image_tower
    state = _state(model)
    _, order = _resnet_named(arch)
    filters = [k for k in order if state[k].dim() == 4 and k != "conv1.weight"]
    groups = D.resnet_shadow_groups(params)
    assert len(groups) == len(filters) and all(len(g) == 1 and g[0] is state[k] for g, k in zip(groups, filters))
    bmodel, bparams, _, _ = text_tower
    state = _state(bmodel)
    want = []
    for i in range(2):
        pre = f"encoder.layer.{i}."
        want += [[pre + "attention.self.query.weight", pre + "attention.self.key.weight", pre + "attention.self.value.weight"],
                 [pre + "attention.output.dense.weight"], [pre + "intermediate.dense.weight"], [pre + "output.dense.weight"]]
    groups = D.bert_shadow_groups(bparams, 2)
    assert len(groups) == len(want)
    for g, names in zip(groups, want):
        assert len(g) == len(names) and all(p is state[k] for p, k in zip(g, names))


def test_output_sizes():
    assert [D.conv_out(h, R, s, p) for h, R, s, p in [(224, 7, 2, 3), (112, 3, 2, 1), (56, 3, 1, 1), (56, 1, 2, 0), (7, 3, 2, 1)]] == [112, 56, 56, 28, 4]
    assert [D.stem_out(h) for h in (224, 32, 33, 31)] == [56, 8, 9, 8]
