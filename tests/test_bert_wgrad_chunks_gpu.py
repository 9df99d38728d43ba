"""Packed text tower: the grouped weight gradients walk only the 32-token chunks that hold a valid token (hs_set_bert_wgrad_chunks),
and the GEMMs with tokens on M deal their workgroups over the live tile rows (hs_set_pack_xcd_spread).  Both keep every result bit
for bit, so the assertions are equalities:

  * right-padded masks: every parameter gradient torch.equal to the PADDED tower's (skip_padded_rows = False), hidden states equal
    on the valid rows -- the bitwise rule of tests/test_bert_packed_gpu.py;
  * masks with holes (where the packed attention rounds differently from the padded one, so the padded tower is no bitwise
    reference): every gradient torch.equal to the packed tower with hs_set_bert_wgrad_chunks(0), the parent's code path, AND that
    file's rule against the CPU oracle (oracle/towers.py:OBertModel): rms error within 1.25x, largest error within 2x of the
    padded tower's, plus 1e-6 max|ref| -- the same bounds for the same reason, the reference is never the code under test;
  * a repeated run is bitwise the first; train mode with dropout on draws the padded tower's masks.

Shapes.  A BertLayer groups its weight gradients only when the four outputs give at least 128 tiles of 256 x 128 (bert_layer_bwd_run:
big_tiles; hidden 256 / inter 512 gives 16), so at hidden 256 no grouped grid runs, the weight gradients go through split-K launches
and the operands must KEEP the padded columns: those shapes ("n-*") check that the one predicate leaves layout and walk alone
together (hs_gemm_k_cols_queued does not move).  The grouped grids themselves need BERT-base widths ("w-*": hidden 768, 12 heads,
inter 3072; 216 tiles): B*L = 2048 takes the phase-pipelined 256 x 256 grid (combo 8 / cfg 7), B*L = 1024 and 1600 the generic
256 x 128 one (combo 8 / cfg 4) -- read from the launch log (hs_prof_dump), and the counter must rise by the 8 problems of the two
layers.  L = 100 makes the 32-position chunks straddle sequences."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from hamspine import _lib as L  # noqa: E402
from hamspine import rt  # noqa: E402
from test_bert_packed_gpu import _hold_to_rule, _inputs, _oracle, _pair, _product  # noqa: E402

DEV = "cuda"


@pytest.fixture(autouse=True)
def _bf16_mode_and_switches():
    hamspine.set_compute_dtype("bf16")
    L.lib().hs_set_bert_wgrad_chunks(1)
    L.lib().hs_set_pack_xcd_spread(1)
    yield
    L.lib().hs_set_bert_wgrad_chunks(1)
    L.lib().hs_set_pack_xcd_spread(1)
    hamspine.set_compute_dtype("bf16")


def _cfg(hidden, heads, inter, **kw):
    return dict(dict(vocab_size=300, hidden_size=hidden, num_hidden_layers=2, num_attention_heads=heads, intermediate_size=inter,
                     max_position_embeddings=128, type_vocab_size=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), **kw)


NARROW, WIDE = _cfg(256, 4, 512), _cfg(768, 12, 3072)
# name -> (config, B, L, grouped cfg expected in the launch log or None)
SHAPES = {"n-a": (NARROW, 16, 128, None), "n-b": (NARROW, 8, 128, None), "n-c": (NARROW, 16, 100, None),
          "w-a": (WIDE, 16, 128, 7), "w-b": (WIDE, 8, 128, 4), "w-c": (WIDE, 16, 100, 4)}
EDGES = [128, 1, 31, 32, 33, 64, 65, 96, 97, 127, 0, 50, 77, 3, 120, 16]     # both sides of every chunk edge, one empty sequence


def _mask_case(name, B, L_):
    """-> (lengths, holes, right_padded)"""
    if name in ("edges", "edges2"):            # B = 8 holds the eleven lengths in two masks
        pick = EDGES if B >= 16 else (EDGES[:8] if name == "edges" else EDGES[8:11] + [64, 33, 0, 1, 128])
        return [min(n, L_) for n in pick[:B]], (), True
    if name == "full":
        return [L_] * B, (), True
    if name == "one":                           # kc_n = 1: the one-tile clamp
        return [0] * (B - 1) + [1], (), True
    lengths = [min(n, L_) for n in (EDGES * 2)[3:3 + B]]
    if name == "hole-mid":                      # positions 32..63 of sequence 1 masked, 64..90 valid: a middle chunk drops out
        lengths[1] = 91
        return lengths, tuple((1, l) for l in range(32, 64)), False
    assert name == "hole-none"                  # holes that empty no chunk
    lengths[1] = 91
    return lengths, ((1, 5), (1, 6), (1, 40), (2, 0)), False


_models = {}


def _model(cfg, train=False):
    key = (cfg["hidden_size"], cfg["hidden_dropout_prob"])
    if key not in _models:
        _models[key] = _pair(cfg, 43, double=False)
    p, o = _models[key]
    (p.train if train else p.eval)()
    (o.train if train else o.eval)()
    return p, o


def _same(what, a, b, valid):
    assert torch.equal(a[0][valid], b[0][valid]), f"{what}: hidden states differ on valid rows"
    assert set(a[1]) == set(b[1])
    bad = [f"{k}: max |diff| {(a[1][k] - b[1][k]).abs().max().item():.3e}" for k in sorted(a[1]) if not torch.equal(a[1][k], b[1][k])]
    assert not bad, f"{what}: gradients differ: {bad}"


def _logged(run):
    """run() with the launch log on -> (its result, {(combo, cfg)} of the launches)"""
    import tempfile
    lib = L.lib()
    lib.hs_prof_enable.argtypes = [C.c_int32]
    lib.hs_prof_enable(1)
    try:
        out = run()
        with tempfile.TemporaryDirectory() as tmp:
            log = tmp + "/launches.csv"
            L.check(lib.hs_prof_dump(log.encode()), "hs_prof_dump")
            rows = [tuple(float(x) for x in line.split(",")) for line in open(log).read().split()]
    finally:
        lib.hs_prof_enable(0)
    return out, {(int(r[1]), int(r[2])) for r in rows}


CASES = [(s_, m_) for s_ in sorted(SHAPES) for m_ in ["edges", "edges2", "full", "one", "hole-mid", "hole-none"]
         if m_ != "edges2" or SHAPES[s_][1] < 16]          # (at B = 16 one mask holds all the lengths)


@pytest.mark.parametrize("shape,mask_name", CASES)
def test_chunk_compacted_weight_gradients_are_bitwise(shape, mask_name):
    cfg, B, L_, grouped_cfg = SHAPES[shape]
    lengths, holes, right_padded = _mask_case(mask_name, B, L_)
    p, o = _model(cfg)
    H = cfg["hidden_size"]
    ids, mask, cot = _inputs(B, L_, lengths, H, cfg["vocab_size"], 23 + B + L_, holes)
    valid = mask.bool()
    lib = L.lib()
    before = lib.hs_gemm_k_cols_queued()
    on, ran = _logged(lambda: _product(p, ids, mask, cot, True))
    queued = lib.hs_gemm_k_cols_queued() - before
    if grouped_cfg is None:
        assert not any(c == 8 for c, _ in ran) and queued == 0, f"{shape}: no grouped grid expected, so no compacted operand: {sorted(ran)} {queued}"
    else:
        assert (8, grouped_cfg) in ran, f"{shape}: the weight gradients did not run as one grouped grid of cfg {grouped_cfg}: {sorted(ran)}"
        assert queued == 8, f"{shape}: {queued} problems were queued with a compacted K walk, 8 expected"
    again = _product(p, ids, mask, cot, True)
    _same(f"{shape} {mask_name} repeated run", on, again, valid)
    lib.hs_set_bert_wgrad_chunks(0)
    before = lib.hs_gemm_k_cols_queued()
    off = _product(p, ids, mask, cot, True)
    assert lib.hs_gemm_k_cols_queued() == before, "hs_set_bert_wgrad_chunks(0) left the compacted walk on"
    lib.hs_set_bert_wgrad_chunks(1)
    _same(f"{shape} {mask_name} chunks on / off", on, off, valid)
    assert torch.isfinite(on[0]).all() and (on[0][~valid] == 0).all()
    padded = _product(p, ids, mask, cot, False)
    if right_padded:
        _same(f"{shape} {mask_name} packed / padded", on, padded, valid)
    else:
        _hold_to_rule(f"{shape} {mask_name}", on, padded, _oracle(o, ids, mask, cot), valid, bitwise=False)


def test_train_mode_with_dropout_equals_the_padded_tower():
    """dropout 0.1 / 0.1, right-padded lengths, the phase-pipelined grouped grid: the draws do not depend on the layout"""
    cfg, B, L_, _ = SHAPES["w-a"]
    cfg = dict(cfg, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    p, _ = _model(cfg, train=True)
    lengths, holes, _ = _mask_case("edges", B, L_)
    ids, mask, cot = _inputs(B, L_, lengths, cfg["hidden_size"], cfg["vocab_size"], 29, holes)
    before = L.lib().hs_gemm_k_cols_queued()
    packed = _product(p, ids, mask, cot, True, seed=4321)
    assert L.lib().hs_gemm_k_cols_queued() - before == 8
    padded = _product(p, ids, mask, cot, False, seed=4321)
    rt.reset_seed(None)
    _same("train mode", packed, padded, mask.bool())


# ---- the row map and the compacted operand themselves ------------------------------------------------------------------------
def _numpy_map(mask):
    """(T, row_of, packed_of, kc_pos) of a [B][L] 0/1 array, as include/hamspine.h describes hs_bert_row_map"""
    flat = mask.reshape(-1) != 0
    row_of = np.flatnonzero(flat)
    packed_of = np.full(flat.size, -1, np.int32)
    packed_of[row_of] = np.arange(row_of.size)
    nch = (flat.size + 31) // 32
    kc_pos = np.array([c for c in range(nch) if flat[c * 32:(c + 1) * 32].any()], np.int32)
    return row_of.size, row_of, packed_of, kc_pos


@pytest.mark.parametrize("B,L_,kind", [(5, 40, "ragged"), (16, 128, "ragged"), (3, 40, "empty"), (2, 100, "holes"), (600, 128, "ragged")])
def test_row_map_chunks_and_compacted_transpose(B, L_, kind):
    """B*L = 200 (no multiple of 32 or 64: the last chunk is short and chunks straddle sequences), 2048, 120 with no valid token
    (kc_n = 0: one K tile of zeros), holes that empty a middle chunk, and 2400 chunks (more than the 256 one step of the map kernel
    takes).  The device map against numpy; then the transpose through its C entry with that map against a numpy gather: valid
    columns in place, zeros from 32 * kc_n to the end of the last 64-column K tile, nothing written behind it."""
    g = np.random.default_rng(B * 1000 + L_)
    mask = np.zeros((B, L_), np.int64)
    if kind == "ragged":
        for b in range(B):
            mask[b, :g.integers(0, L_ + 1) if b % 3 else (L_ if b % 2 else 1)] = 1
        if B >= 16:
            mask[4:9] = 0                       # whole sequences (and so whole chunks) without a token
    elif kind == "holes":
        mask[0, :91] = 1
        mask[0, 32:64] = 0
        mask[1, 5:60] = 1
        mask[1, 7] = 0
    T, row_of, packed_of, kc_pos = _numpy_map(mask)
    R, nch = B * L_, (B * L_ + 31) // 32
    lib = L.lib()
    words = lib.hs_bert_row_map_bytes(B, L_) // 4
    cu_pad = (B + 1 + 3) // 4 * 4
    assert words >= 4 + cu_pad + 2 * R + nch
    dmap = torch.full((words,), -7, dtype=torch.int32, device=DEV)
    dmask = torch.from_numpy(mask).to(DEV)
    L.check(lib.hs_bert_row_map(dmask.data_ptr(), B, L_, dmap.data_ptr(), rt.stream()), "hs_bert_row_map")
    m = dmap.cpu().numpy()
    o_row, o_inv, o_kc = 4 + cu_pad, 4 + cu_pad + R, 4 + cu_pad + 2 * R
    assert m[0] == T and m[1] == kc_pos.size and m[2] == 32 * kc_pos.size
    assert np.array_equal(m[4:4 + B + 1], np.concatenate([[0], np.cumsum(mask.sum(1))]))
    assert np.array_equal(m[o_row:o_row + T], row_of) and np.array_equal(m[o_inv:o_inv + R], packed_of)
    assert np.array_equal(m[o_kc:o_kc + kc_pos.size], kc_pos)
    if B > 16:
        return
    Cc = 72
    src = torch.randn(R, Cc, generator=torch.Generator().manual_seed(B)).bfloat16()
    src[T:] = 99.0                              # rows that do not exist: must reach nothing
    x = src.to(DEV)
    zero_end = min(R, max(64, (32 * kc_pos.size + 63) // 64 * 64))
    for compact in (True, False):
        y = torch.full((Cc, R), 55.0, dtype=torch.bfloat16, device=DEV)
        kc_n = dmap.data_ptr() + 4 if compact else None
        kc_p = dmap.data_ptr() + 4 * o_kc if compact else None
        L.check(lib.hs_transpose_bf16_tokens(x.data_ptr(), y.data_ptr(), R, Cc, Cc, R, dmap.data_ptr() + 4 * o_inv, kc_n, kc_p, rt.stream()),
                "hs_transpose_bf16_tokens")
        pos = np.arange(R)                      # padded position of each result column (R: none)
        if compact:
            live = pos < 32 * kc_pos.size
            pos = np.full(R, R)
            pos[live] = kc_pos[np.flatnonzero(live) // 32] * 32 + np.flatnonzero(live) % 32
        srow = np.where(pos < R, packed_of[np.minimum(pos, R - 1)], -1)
        want = torch.zeros(Cc, R, dtype=torch.bfloat16)
        have = torch.from_numpy(srow >= 0)
        want[:, have] = src[torch.from_numpy(srow[srow >= 0]).long()].T
        if compact:
            want[:, zero_end:] = 55.0
        assert torch.equal(y.cpu(), want), f"compact={compact}"


# ---- live tiles over all XCDs ---------------------------------------------------------------------------------------------------
def _lengths_for(T, B, L_):
    out = []
    for _ in range(B):
        out.append(min(L_, T))
        T -= out[-1]
    return out


@pytest.mark.parametrize("T", [1, 64, 65, 128, 129, 256, 257, 2048])
def test_xcd_spread_changes_no_result(T):
    """the narrow shape n-a (hidden 256, B = 16, L = 128) with T on both sides of every tile height the tower's GEMMs use (64,
    128, 256), one token, and every token: hidden states and all gradients equal with the spread on and off"""
    cfg, B, L_, _ = SHAPES["n-a"]
    p, _ = _model(cfg)
    ids, mask, cot = _inputs(B, L_, _lengths_for(T, B, L_), cfg["hidden_size"], cfg["vocab_size"], 31 + T)
    assert int(mask.sum()) == T
    on = _product(p, ids, mask, cot, True)
    L.lib().hs_set_pack_xcd_spread(0)
    off = _product(p, ids, mask, cot, True)
    L.lib().hs_set_pack_xcd_spread(1)
    _same(f"T = {T}: spread on / off", on, off, mask.bool())
    _same(f"T = {T}: packed / padded", on, _product(p, ids, mask, cot, False), mask.bool())


def test_xcd_spread_on_the_phase_pipelined_body():
    """BERT-base widths at B = 22 (the smallest batch at which the FFN up-projection takes the 256 x 256 phase-pipelined body, see
    tests/test_bert_packed_gpu.py test 3), T = 1707"""
    B, L_ = 22, 128
    p, _ = _model(WIDE)
    lengths = [128, 109, 117, 119, 43, 26, 17, 1, 127, 64, 65, 100, 90, 33, 77, 128, 5, 111, 96, 71, 120, 60]
    ids, mask, cot = _inputs(B, L_, lengths, 768, WIDE["vocab_size"], 13)
    on, ran = _logged(lambda: _product(p, ids, mask, cot, True))
    assert (0, 7) in ran, f"no launch of the 256x256 phase-pipelined body: {sorted(ran)}"
    L.lib().hs_set_pack_xcd_spread(0)
    off = _product(p, ids, mask, cot, True)
    L.lib().hs_set_pack_xcd_spread(1)
    _same("spread on / off", on, off, mask.bool())
