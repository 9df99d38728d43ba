"""The BERT tower on its valid tokens only (BertModel(skip_padded_rows=True), hs_bert_desc.pack_rows) against the CPU oracle.

Every comparison is against the oracle's BERT (oracle/towers.py:OBertModel), never against the new code: the packed tower's
error and the padded bf16 tower's error are measured against that oracle on the same inputs, and

    err_packed <= 1.25 * err_padded + 1e-6 * max|ref|

must hold on the valid rows of the hidden state and on every parameter gradient.  A wrong row map, a stale partial row or
another dropout draw is an O(1) error.  Cotangents are zero at masked positions.

For RIGHT-PADDED masks more is required: the packed tower is bitwise the padded tower, on valid hidden states and on every
gradient.  Row-wise kernels and GEMM rows do not depend on where a row sits; the kernels that sum over tokens (weight and bias
gradients through their transposed operands, LayerNorm backward, column sums, embedding gradients) walk the padded positions
and leave out the masked ones, where the padded tower adds exact zeros -- the same terms in the same order.

The rule is held twice: on the ROOT-MEAN-SQUARE error over the tensor's elements with the factor 1.25, and on the largest
single error -- with the factor 1.25 wherever the masks are right-padded (there both measures give a ratio of exactly 1), and
with the factor 2 where a mask has holes, over three seeds.  Why 2 there: err (RMS) is the ROOT-MEAN-SQUARE error over the tensor's elements (the normwise measure the other bf16 gradient checks of this suite
use), not the largest single error.  For right-padded masks the two towers agree bitwise in the forward pass and either measure
gives a ratio of 1.00.  With holes in a mask the keys of a sequence sit at other positions of the fused attention's tiles, the
f32 sums over keys round differently and a few bf16 results flip by one ulp: both towers are then equally good bf16
approximations with DIFFERENT rounding noise, and the largest of a few hundred noise terms is an extreme-value statistic that
differs by more than 25 % between two correct implementations (measured on the hole case: max-abs 4.81e-01 against 3.85e-01 on
a LayerNorm weight gradient of magnitude 66, 2.08e-01 against 1.64e-01 on a value bias gradient of magnitude 42 -- 0.7 % and
0.5 % errors both ways), while the RMS over the same elements is stable to a few per cent.  A fault in ONE row cannot hide
in the mean because the largest error is bounded too: a wrong, stale or missing row is an error of the size of the values
themselves, a hundred times the bf16 noise, where the bound allows twice the padded tower's own largest error."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from hamspine import _lib as L  # noqa: E402
from hamspine import rt  # noqa: E402
from hamspine import tower  # noqa: E402
from oracle import towers  # noqa: E402
from oracle.procedural import load_procedural  # noqa: E402

DEV = "cuda"


@pytest.fixture(autouse=True)
def _bf16_mode():
    hamspine.set_compute_dtype("bf16")
    yield
    hamspine.set_compute_dtype("bf16")


TINY = dict(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
            max_position_embeddings=128, type_vocab_size=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def _pair(cfg, seed, double=True):
    from hamspine.nn import BertConfig, BertModel
    o = load_procedural(towers.OBertModel(**cfg), seed)
    p = BertModel(BertConfig(**cfg))
    p.load_state_dict(o.state_dict(), strict=False)
    return p.to(DEV), (o.double() if double else o)


def _inputs(B, L, lengths, H, vocab, seed, holes=()):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab, (B, L), generator=g)
    mask = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    for b, l in holes:
        mask[b, l] = 0
    cot = torch.randn(B, L, H, generator=g) * mask[..., None]
    return ids, mask, cot


def _product(p, ids, mask, cot, pack, seed=None, expect=None):
    """-> (hidden f32 on the CPU, {name: grad}) of one forward + backward with packing asked for / not; expect: whether the tower
    must have run packed (default: as asked)"""
    p.zero_grad(set_to_none=True)
    p.skip_padded_rows = pack
    if seed is not None:
        rt.reset_seed(seed)
    h = p(input_ids=ids.to(DEV), attention_mask=mask.to(DEV)).last_hidden_state
    assert tower.bert_ran_packed(h) == (pack if expect is None else expect), "the tower did not run in the mode the test expects"
    (h.float() * cot.to(DEV)).sum().backward()
    grads = {k: v.grad.detach().double().cpu() for k, v in p.named_parameters() if v.grad is not None}
    return h.detach().double().cpu(), grads


def _oracle(o, ids, mask, cot):
    o.zero_grad(set_to_none=True)
    dt = next(o.parameters()).dtype
    h = o(ids, mask)
    (h * cot.to(dt)).sum().backward()
    return h.detach().double(), {k: v.grad.detach().double() for k, v in o.named_parameters() if v.grad is not None}


def _hold_to_rule(what, packed, padded, ref, valid=None, bitwise=False):
    """packed / padded / ref: (hidden, grads).  Prints every figure before it asserts.  bitwise (right-padded masks): packed must
    EQUAL padded too, and the largest single error is held to the factor 1.25; otherwise (holes) to the factor 2."""
    bad = []
    differ = []

    def one(name, a, b, r):
        ea, eb, scale = (a - r).pow(2).mean().sqrt().item(), (b - r).pow(2).mean().sqrt().item(), r.abs().max().item()
        print(f"{what:28s} {name:55s} rms err_packed {ea:.4e} err_padded {eb:.4e} max|ref| {scale:.3e} "
              f"(max-abs {(a - r).abs().max().item():.3e} / {(b - r).abs().max().item():.3e})")
        assert math.isfinite(ea), f"{what} {name}: packed result is not finite"
        if ea > 1.25 * eb + 1e-6 * scale:
            bad.append(f"{name}: rms packed {ea:.4e} padded {eb:.4e} max|ref| {scale:.3e}")
        ma, mb = (a - r).abs().max().item(), (b - r).abs().max().item()
        if ma > (1.25 if bitwise else 2.0) * mb + 1e-6 * scale:
            bad.append(f"{name}: max-abs packed {ma:.4e} padded {mb:.4e} max|ref| {scale:.3e}")
        if bitwise and not torch.equal(a, b):
            differ.append(f"{name}: max |packed - padded| {(a - b).abs().max().item():.3e}")
    v = valid if valid is not None else torch.ones(ref[0].shape[:2], dtype=torch.bool)
    one("hidden (valid rows)", packed[0][v], padded[0][v], ref[0][v])
    missing = [k for k in padded[1] if not k.startswith("pooler") and k not in packed[1]]
    assert not missing, f"{what}: the packed run returned no gradient for {missing}"
    for k in sorted(ref[1]):
        if k.startswith("pooler") or k not in padded[1]:
            continue
        one(k, packed[1][k], padded[1][k], ref[1][k])
    assert not bad, f"{what}: packed rows miss the 1.25x rule: {bad}"
    assert not differ, f"{what}: right-padded masks, yet the packed tower is not bitwise the padded tower: {differ}"


def _lengths(L):
    return [L, 1, (L + 1) // 2 + 3, L - 1]


# 1. tiny model, eval mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["L24", "L128", "hole-s0", "hole-s1", "hole-s2", "empty"])
def test_packed_tower_matches_oracle_like_the_padded_tower(case):
    """hidden 128, 2 heads (head dim 64), inter 256, 2 layers, eval mode, B = 4.  L = 24 and L = 128 with lengths
    [L, 1, ceil(L/2)+3, L-1] (L = 128: T = 323 tokens -- not a multiple of 64, and it crosses a 256-row tile); a mask with holes
    (valid tokens keep their order), three seeds of inputs; a sequence without any valid token (its sample is outside the
    comparison as it is outside every cotangent; the packed output there must be zero and finite, and since that sample adds
    exact zeros to every sum of the padded tower, the rest is bitwise the padded tower's)."""
    L_ = 24 if case == "L24" else 128
    lengths, holes = _lengths(L_), ()
    hole_seed = int(case[-1]) if case.startswith("hole") else 0
    if case.startswith("hole"):
        holes = ((0, 5), (0, 6), (2, 0), (3, 77))
    if case == "empty":
        lengths = [L_, 0, (L_ + 1) // 2 + 3, L_ - 1]
    p, o = _pair(TINY, 31)
    p.eval()
    o.eval()
    ids, mask, cot = _inputs(4, L_, lengths, 128, 100, 7 + L_ + 1000 * hole_seed, holes)
    if case == "L128":
        assert int(mask.sum()) == 323
    packed = _product(p, ids, mask, cot, True)
    padded = _product(p, ids, mask, cot, False)
    ref = _oracle(o, ids, mask, cot)
    valid = mask.bool()
    _hold_to_rule(case, packed, padded, ref, valid, bitwise=not case.startswith("hole"))
    assert torch.isfinite(packed[0]).all() and (packed[0][~valid] == 0).all(), "masked positions must hold exact zeros"


# 2. tiny model, train mode -----------------------------------------------------------------------------------------------
def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def _keep_scale(seed, n, p):
    """the product's dropout scale (0 or 1/(1-p)) of flat indices 0..n-1 under `seed` (csrc/hs_common.h: dropout_scale)"""
    seed &= (1 << 64) - 1
    i = np.arange(n, dtype=np.uint64)
    q = i >> np.uint64(2)
    s0, s1 = np.uint32(seed & 0xffffffff), np.uint32(seed >> 32)
    with np.errstate(over="ignore"):
        x = (q & np.uint64(0xffffffff)).astype(np.uint32) * np.uint32(0x9E3779B1) + s0 + (q >> np.uint64(32)).astype(np.uint32) * np.uint32(0x85EBCA77)
        r0 = _mix32(x ^ s1)
        r1 = _mix32(r0 + np.uint32(0x6C8E9CF5) + s1)
    w = np.where((i & np.uint64(2)) != 0, r1, r0)
    f = np.where((i & np.uint64(1)) != 0, w >> np.uint32(16), w & np.uint32(0xffff))
    thresh = int(p * 4294967296.0) >> 16
    return torch.from_numpy(np.where(f >= thresh, 1.0 / (1.0 - p), 0.0))


class _FixedDropout(torch.nn.Module):
    def __init__(self, scale):
        super().__init__()
        self.scale = scale

    def forward(self, x):
        return x * self.scale.view(x.shape).to(x.dtype)


def _install_product_masks(o, base_seed, B, L, H, heads, p_hidden, p_attn):
    """the oracle's nn.Dropout modules replaced by the masks the product draws after rt.reset_seed(base_seed): tower seed =
    next_seed() * 64; embeddings use it, layer i uses s = seed + 16 (i + 1): attention 8 s + 1 (index ((b heads + h) L + q) L + k),
    attention-output dense 8 s + 2, FFN output dense 8 s + 3 (index row * hidden + column)."""
    seed = ((base_seed + 16) * 64) & ((1 << 64) - 1)
    o.embeddings.dropout = _FixedDropout(_keep_scale(seed, B * L * H, p_hidden))
    for i, layer in enumerate(o.encoder.layer):
        s = seed + 16 * (i + 1)
        layer.attention.self.dropout = _FixedDropout(_keep_scale(s * 8 + 1, B * heads * L * L, p_attn))
        layer.attention.output.dropout = _FixedDropout(_keep_scale(s * 8 + 2, B * L * H, p_hidden))
        layer.output.dropout = _FixedDropout(_keep_scale(s * 8 + 3, B * L * H, p_hidden))


def test_packed_tower_train_mode_draws_the_padded_towers_masks():
    """hidden dropout 0.25, attention dropout 0.2, rt.reset_seed before each evaluation, right-padded masks: every draw of the
    packed run is the padded run's (the draw of a packed row is the one of its padded position), so both are held against the
    oracle evaluated with the product's masks, at the 1.25x rule; and a repeated packed run is bitwise the same."""
    cfg = dict(TINY, hidden_dropout_prob=0.25, attention_probs_dropout_prob=0.2)
    p, o = _pair(cfg, 33)
    p.train()
    o.train()
    B, L_ = 4, 24
    ids, mask, cot = _inputs(B, L_, _lengths(L_), 128, 100, 11)
    _install_product_masks(o, 1234, B, L_, 128, 2, 0.25, 0.2)
    packed = _product(p, ids, mask, cot, True, seed=1234)
    again = _product(p, ids, mask, cot, True, seed=1234)
    padded = _product(p, ids, mask, cot, False, seed=1234)
    rt.reset_seed(None)
    ref = _oracle(o, ids, mask, cot)
    _hold_to_rule("train", packed, padded, ref, mask.bool(), bitwise=True)
    assert torch.equal(packed[0], again[0]), "a repeated packed run differs"
    for k in packed[1]:
        assert torch.equal(packed[1][k], again[1][k]), f"a repeated packed run differs in the gradient of {k}"


# 3. BERT-base dims, the bodies the flagship runs ------------------------------------------------------------------------
def test_packed_tower_bert_base_dims_on_the_flagship_kernel_bodies(tmp_path):
    """hidden 768, 12 heads, inter 3072, 2 layers, B = 22, L = 128: B*L = 2816 is the smallest multiple of 128 at which
    csrc/gemm.hip's selection takes every body the flagship uses on this tower -- p8_cfg: M % 256 == 0 and (M / 256) * (N / 256)
    >= 128 at N = 3072 (FFN up-projection; the 256 x 256 phase-pipelined body, cfg 7) needs M >= 2816; auto_cfg: K >= 2048 and
    ceil(M / 128) * (768 / 64) >= 256 (FFN down-projection, the 128 x 64 body, cfg 1) needs M >= 2688; gemm_group_add: K = M >= 2048
    and M % 64 == 0 puts the 8 weight gradients of the two layers in ONE grouped 256 x 256 grid (combo 8, cfg 7).  Which ran is
    read from the launch log (hs_prof_dump) below.  Ragged lengths, T = 1707 valid tokens: off every multiple of 64, 128 and 256."""
    cfg = dict(vocab_size=500, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072,
               max_position_embeddings=128, type_vocab_size=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    p, o = _pair(cfg, 35, double=False)
    p.eval()
    o.eval()
    B, L_ = 22, 128
    lengths = [128, 109, 117, 119, 43, 26, 17, 1, 127, 64, 65, 100, 90, 33, 77, 128, 5, 111, 96, 71, 120, 60]
    ids, mask, cot = _inputs(B, L_, lengths, 768, 500, 13)
    T = int(mask.sum())
    assert T == 1707 and T % 64 and T % 128 and T % 256
    lib = L.lib()
    lib.hs_prof_enable.argtypes = [C.c_int32]
    log = str(tmp_path / "launches.csv")
    lib.hs_prof_enable(1)
    try:
        packed = _product(p, ids, mask, cot, True)
        L.check(lib.hs_prof_dump(log.encode()), "hs_prof_dump")
    finally:
        lib.hs_prof_enable(0)
    rows = [tuple(float(x) for x in line.split(",")) for line in open(log).read().split()]
    ran = {(int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5])) for r in rows}        # (combo, cfg, M, N, K)
    assert (0, 7, 2816, 3072, 768) in ran, f"the FFN up-projection did not take the 256x256 phase-pipelined body: {sorted(ran)}"
    assert (0, 1, 2816, 768, 3072) in ran, f"the FFN down-projection did not take the 128x64 body: {sorted(ran)}"
    assert (8, 7, 8, 0, 0) in ran, f"the two layers' weight gradients did not run as one grouped 256x256 grid: {sorted(ran)}"
    padded = _product(p, ids, mask, cot, False)
    ref = _oracle(o, ids, mask, cot)
    _hold_to_rule("bert-base dims", packed, padded, ref, mask.bool(), bitwise=True)


# 4. model-level opt-in --------------------------------------------------------------------------------------------------
def _small_model(tmp_path, fusion_type, **kw):
    import golden_cases as gc
    import model as product_model
    cfg = dict(TINY, vocab_size=gc.TINY_BERT["vocab_size"], max_position_embeddings=40)
    d = gc.save_bert_dir(cfg, str(tmp_path / ("bert_" + fusion_type)))
    common = dict(gc.E2E_COMMON, text_feature_dim=128)
    m = product_model.MultimodalBaselineModel(pretrained_image=False, image_weights_path=None, text_model_name=d,
                                              fusion_type=fusion_type, classifier_type="mlp", **common, **kw)
    load_procedural(m, 41)
    return m.to(DEV).train(), cfg, common


def test_model_turns_packing_on_for_key_masked_fusions_only(tmp_path, monkeypatch):
    """MultimodalBaselineModel(fusion_type="basic") runs the text tower on packed rows, and with HAMSPINE_BERT_PACK=0 on every
    row: logits and all gradients of both are held against the oracle model at the 1.25x rule.  A pooled fusion (mean over all L
    text rows) keeps the padded tower: asserted on the flag the tower ran with."""
    import golden_cases as gc
    from oracle import models as om
    m, cfg, common = _small_model(tmp_path, "basic")
    o = load_procedural(om.OMultimodalBaselineModel(bert_cfg=cfg, fusion_type="basic", classifier_type="mlp", **common), 41).double().train()
    images, ids, mask, labels, _ = gc.e2e_inputs({})
    cot = torch.randn(4, 7, generator=torch.Generator().manual_seed(5))
    bert = m.text_encoder.model
    assert bert.skip_padded_rows
    seen = []
    m.text_encoder.register_forward_hook(lambda mod, args, out: seen.append(tower.bert_ran_packed(out)))

    def run(flag):
        m.zero_grad(set_to_none=True)
        logits = m(images.to(DEV), ids.to(DEV), mask.to(DEV))
        assert seen and seen[-1] == flag
        (logits.float() * cot.to(DEV)).sum().backward()
        return logits.detach().double().cpu(), {k: v.grad.detach().double().cpu() for k, v in m.named_parameters() if v.grad is not None}
    packed = run(True)
    monkeypatch.setenv("HAMSPINE_BERT_PACK", "0")
    padded = run(False)
    monkeypatch.delenv("HAMSPINE_BERT_PACK")
    o.zero_grad(set_to_none=True)
    lo = o(images.double(), ids, mask)
    (lo * cot.double()).sum().backward()
    ref = (lo.detach(), {k: v.grad.detach() for k, v in o.named_parameters() if v.grad is not None})

    def as_rows(t):
        return (t[0][:, None, :], t[1])
    _hold_to_rule("model basic", as_rows(packed), as_rows(padded), as_rows(ref), bitwise=True)

    pooled, _, _ = _small_model(tmp_path, "concat", text_pool="mean")
    assert not pooled.text_encoder.model.skip_padded_rows
    seen_pooled = []
    pooled.text_encoder.register_forward_hook(lambda mod, args, out: seen_pooled.append(tower.bert_ran_packed(out)))
    pooled(images.to(DEV), ids.to(DEV), mask.to(DEV))
    assert seen_pooled == [False]


# 4b. frozen parameters --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L_", [(16, 128), (4, 24)])
@pytest.mark.parametrize("frozen", ["query", "qkv"])
def test_frozen_attention_weights(B, L_, frozen):
    """B*L = 2048 (where a generic Linear backward switches to transposed operands) and below it.  With ONLY the query weight
    of a layer frozen the three Q/K/V weight gradients no longer come from one fused GEMM, and the per-matrix paths have no
    packed form: the tower must take the padded path silently.  With query, key and value weights all frozen it stays packed
    (their bias gradients are column sums over the padded positions).  Either way every gradient that is returned equals the
    padded tower's bit for bit, and a frozen weight gets none."""
    p, o = _pair(TINY, 39)
    p.eval()
    o.eval()
    att = p.encoder.layer[1].attention.self
    names = ["query"] if frozen == "query" else ["query", "key", "value"]
    for n in names:
        getattr(att, n).weight.requires_grad_(False)
        getattr(o.encoder.layer[1].attention.self, n).weight.requires_grad_(False)
    lengths = [L_, 1, (L_ + 1) // 2 + 3, L_ - 1] + [max(1, (7 * i) % L_) for i in range(B - 4)]
    ids, mask, cot = _inputs(B, L_, lengths, 128, 100, 19 + L_)
    asked = _product(p, ids, mask, cot, True, expect=frozen == "qkv")
    padded = _product(p, ids, mask, cot, False)
    ref = _oracle(o, ids, mask, cot)
    for n in names:
        assert f"encoder.layer.1.attention.self.{n}.weight" not in asked[1]
    _hold_to_rule(f"frozen {frozen} {B}x{L_}", asked, padded, ref, mask.bool(), bitwise=True)


# 5. masked positions ----------------------------------------------------------------------------------------------------
def test_masked_positions_give_zeros_and_take_no_gradient():
    """the output at masked positions is exactly zero, and a cotangent that is non-zero ONLY at masked positions yields all-zero
    gradients (the backward gathers the valid rows and ignores the rest)."""
    p, _ = _pair(TINY, 37)
    p.eval()
    ids, mask, _ = _inputs(4, 24, _lengths(24), 128, 100, 17, holes=((0, 3),))
    cot = torch.randn(4, 24, 128, generator=torch.Generator().manual_seed(3)) * (1 - mask)[..., None]
    h, grads = _product(p, ids, mask, cot, True)
    assert (h[~mask.bool()] == 0).all() and torch.isfinite(h).all()
    assert grads, "no gradient came back"
    for k, g in grads.items():
        assert (g == 0).all(), f"{k}: a cotangent at masked positions reached a gradient"
