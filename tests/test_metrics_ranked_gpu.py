"""hs_metrics_auroc_ranked (csrc/metrics.hip) against tests/metrics_ref.py::pair_counts (every pair compared; small n) and
tests/metrics_ranked_ref.py::pair_counts_sorted (sort + searchsorted, pinned on the former by test_metrics_ranked_cpu.py; large
n), integer for integer, and MulticlassMeter(auroc="ranked") against auroc="pairs" bit for bit.

Sizes the kernels can go wrong at: a wave is 64 rows, a block takes 256 keys per round and 2048 (TILE) per tile of the sort, a
block of the search 1024 (SEARCH) rows; so n runs around 64, 256, 1024, 2048 and 4096, and 70 001 rows make 35 blocks per
class."""
import numpy as np
import pytest
import torch

import metrics_ref as R
import metrics_ranked_ref as RR

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402,F401
from hamspine import _lib as L  # noqa: E402
from hamspine import metrics as M  # noqa: E402
from hamspine import rt  # noqa: E402

DEV = "cuda"
TILE, SEARCH = 2048, 1024
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, SEARCH + 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE,
         4097)
SMALL = 5000                                                   # up to here the n^2 form is the reference


def _ranked(scores, labels, C, capacity=None, ws_bytes=None, garbage=False):
    """scores (n, C) f32 and labels (n,) -> (C, 4) int64 counts of the ranked entry"""
    n = len(labels)
    cap = n if capacity is None else capacity
    s = torch.full((C, max(cap, 1)), 0.5 if garbage else 0.0, dtype=torch.float32, device=DEV)
    y = torch.full((max(cap, 1),), 0 if garbage else -1, dtype=torch.int32, device=DEV)
    s[:, :n] = torch.from_numpy(np.ascontiguousarray(scores.T)).to(DEV)
    y[:n] = torch.from_numpy(labels.astype(np.int32)).to(DEV)
    counts = torch.full((C, 4), -7, dtype=torch.int64, device=DEV)
    ws = None if ws_bytes is None else torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    M.metrics_auroc_ranked(s, y, n, counts, ws)
    return counts.cpu().numpy()


def _check(scores, labels, C, **kw):
    ref = R.pair_counts if len(labels) <= SMALL else RR.pair_counts_sorted
    want, got = ref(scores, labels, C), _ranked(scores, labels, C, **kw)
    assert np.array_equal(got, want), f"n={len(labels)} C={C}: rows {np.flatnonzero((got != want).any(1))[:5]} differ"
    return want


def _random(n, C, seed, ties=True):
    rng = np.random.default_rng(seed)
    scores = rng.random((n, C), dtype=np.float32)
    if ties:
        scores = np.round(scores * 64) / np.float32(64)       # scores tie
    return scores.astype(np.float32), rng.integers(0, C, n)


@pytest.mark.parametrize("C", [2, 7, 64])
def test_sizes_around_the_wave_round_tile_and_search_block(C):
    for n in SIZES:
        _check(*_random(n, C, 1000 * C + n, ties=n % 2 == 0), C)


def test_many_blocks():
    scores, labels = _random(70001, 3, 11, ties=False)
    scores[::7] = np.round(scores[::7] * 256) / np.float32(256)
    want = _check(scores, labels, 3)
    assert want[:, 1].min() > 0 and want[:, 0].min() > 2 ** 28


def test_every_digit_pass_and_the_sign_handling():
    vals = RR.bit_pattern_scores()
    rng = np.random.default_rng(12)
    scores = np.stack([rng.permutation(np.concatenate([vals, vals])) for _ in range(3)], axis=1)
    want = _check(scores, rng.integers(0, 3, len(scores)), 3)
    assert want[:, 1].min() > 0
    z = np.array([[0.0], [-0.0], [1e-45], [-1e-45]], dtype=np.float32).repeat(2, axis=1)
    assert np.array_equal(_check(z, np.array([0, 1, 0, 1]), 2), [[3, 1, 2, 2], [0, 1, 2, 2]])


def test_equal_and_two_valued_scores():
    rng = np.random.default_rng(13)
    labels = rng.integers(0, 7, 2500)
    want = _check(np.full((2500, 7), 0.25, dtype=np.float32), labels, 7)
    assert (want[:, 0] == 0).all() and np.array_equal(want[:, 1], want[:, 2] * want[:, 3])
    _check(rng.choice(np.array([0.25, 0.75], dtype=np.float32), size=(2500, 7)), labels, 7)


@pytest.mark.parametrize("where", ["pos", "neg", "both"])
def test_nan_scores_count_in_p_or_nn_and_take_part_in_no_pair(where):
    scores, labels = _random(2300, 3, 14)
    clean = R.pair_counts(scores, labels, 3)
    for c in range(3):
        pos, neg = np.flatnonzero(labels == c), np.flatnonzero(labels != c)
        if where in ("pos", "both"):
            scores[pos[::3], c] = np.nan
        if where in ("neg", "both"):
            scores[neg[::4], c] = -np.nan
    got = _check(scores, labels, 3)
    assert np.array_equal(got[:, 2:], clean[:, 2:]) and (got[:, 0] < clean[:, 0]).all()


def test_unlabelled_rows_empty_sides_and_rows_beyond_n():
    scores, labels = _random(2300, 7, 15)
    labels[::5] = -1
    _check(scores, labels, 7)
    labels = np.where(labels == 4, 2, labels)                 # class 4 has no positives
    assert _check(scores, labels, 7)[4, 2] == 0
    only = np.where(labels >= 0, 1, -1)                       # class 1 has no negatives, the others no positives
    want = _check(scores, only, 7)
    assert want[1, 3] == 0 and (want[:, :2] == 0).all()
    # n < capacity: the rows beyond n hold ordinary-looking scores and labels that must not be counted
    scores, labels = _random(300, 7, 16)
    _check(scores, labels, 7, capacity=777, garbage=True)
    _check(scores[:0], labels[:0], 7, capacity=8, garbage=True)   # n = 0: zeros


def test_a_workspace_for_some_of_the_classes_gives_the_same_integers():
    scores, labels = _random(2300, 7, 17)
    full = M.auroc_ranked_ws_bytes(2300, 7)
    assert full % 7 == 0 and full < 7 * (2300 * 8 + 2 * 1024 + 64)
    want = _check(scores, labels, 7, ws_bytes=full)
    for classes in (1, 2, 3, 6):                              # 7, 4, 3 and 2 rounds
        assert np.array_equal(_ranked(scores, labels, 7, ws_bytes=full // 7 * classes + 16), want)
    assert M.auroc_ranked_ws_bytes(0, 7) == 0 and L.lib().hs_metrics_auroc_ranked_ws_bytes(10, 65) == -1
    assert L.lib().hs_metrics_auroc_ranked_ws_bytes(2 ** 31, 7) == -1


def test_refusals_write_nothing():
    C, n = 7, 300
    scores, labels = _random(n, C, 18)
    s = torch.from_numpy(np.ascontiguousarray(scores.T)).to(DEV)
    y = torch.from_numpy(labels.astype(np.int32)).to(DEV)
    one = M.auroc_ranked_ws_bytes(n, C) // C
    ws = torch.full((one * C,), 0x5a, dtype=torch.uint8, device=DEV)
    counts = torch.full((64 + C * 4 + 64,), -7, dtype=torch.int64, device=DEV)
    out = counts[64:64 + C * 4]
    lib = L.lib()

    def call(s_ptr=rt.p(s), y_ptr=rt.p(y), n=n, cap=n, C=C, ws_ptr=rt.p(ws), ws_bytes=one * C, out_ptr=rt.p(out)):
        return lib.hs_metrics_auroc_ranked(s_ptr, y_ptr, n, cap, C, ws_ptr, ws_bytes, out_ptr, rt.stream())

    for what, kw in (("a workspace too small for one class", dict(ws_bytes=one - 4)), ("no workspace", dict(ws_ptr=None)),
                     ("an unaligned workspace", dict(ws_ptr=rt.p(ws[4:]), ws_bytes=one * C - 4)),
                     ("C = 1", dict(C=1)), ("C = 65", dict(C=65)), ("null scores", dict(s_ptr=None)),
                     ("null labels", dict(y_ptr=None)), ("null counts", dict(out_ptr=None)), ("n > capacity", dict(n=n + 1)),
                     ("n < 0", dict(n=-1)), ("capacity = 2^31", dict(cap=2 ** 31))):
        status = call(**kw)
        torch.cuda.synchronize()
        assert status != 0, f"{what}: accepted"
        with pytest.raises(L.HamspineError):
            L.check(status, what)
        assert bool((counts == -7).all()) and bool((ws == 0x5a).all()), f"{what}: refused, but something was written"
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.view(C, 4).cpu().numpy(), R.pair_counts(scores, labels, C))
    assert bool((counts[:64] == -7).all()) and bool((counts[-64:] == -7).all())


# ------------------------------------------------------------------------------------------------------------ the meter
BATCHES = (1, 63, 64, 65, 200)


_inputs = RR.meter_inputs


def _bits(v):
    return np.atleast_1d(np.asarray(v)).view(np.uint8)


def _meter(C, dtype, logits, labels, auroc, reverse=False):
    meter = M.MulticlassMeter(C, capacity=64, device=DEV, auroc=auroc)
    bounds = np.cumsum((0,) + BATCHES)
    chunks = list(zip(bounds[:-1], bounds[1:]))
    for lo, hi in (chunks[::-1] if reverse else chunks):
        meter.update(torch.from_numpy(logits[lo:hi]).to(DEV, dtype), torch.from_numpy(labels[lo:hi]).to(DEV))
    return meter


@pytest.mark.parametrize("C,dtype", [(2, torch.float32), (7, torch.float32), (7, torch.bfloat16), (64, torch.float32),
                                     (64, torch.bfloat16)], ids=lambda p: str(p).split(".")[-1])
def test_meter_ranked_equals_pairs_bit_for_bit(C, dtype):
    logits, labels = _inputs(sum(BATCHES), C, 17 * C)
    pairs = _meter(C, dtype, logits, labels, "pairs")
    want, want_counts = pairs.compute(), pairs.auroc_counts()
    assert want_counts[:, 1].sum() > 0 and not np.isnan(want["auroc_macro"])
    for reverse in (False, True):
        ranked = _meter(C, dtype, logits, labels, "ranked", reverse)
        assert ranked.capacity == 512 and ranked._ws is None
        got = ranked.compute()
        assert ranked._ws is not None and ranked._ws.numel() == M.auroc_ranked_ws_bytes(512, C)
        ws = ranked._ws
        assert np.array_equal(ranked.auroc_counts(), want_counts)
        assert set(got) == set(want)
        for k, v in want.items():
            assert np.array_equal(_bits(got[k]), _bits(v)), k
        ranked.compute()
        assert ranked._ws is ws, "the workspace is not reused"
    auto = _meter(C, dtype, logits, labels, "auto")
    auto.compute()
    assert np.array_equal(auto.auroc_counts(), want_counts)
    if M.AUTO_RANKED_ROWS is None or auto.n < M.AUTO_RANKED_ROWS:
        assert auto._ws is None, "auto took the ranked route below its threshold"
    with pytest.raises(ValueError):
        M.MulticlassMeter(C, auroc="sorted")


def test_auto_changes_route_at_its_threshold_and_not_the_integers():
    T = M.AUTO_RANKED_ROWS
    assert isinstance(T, int) and T > 1, "no measured threshold: auto never takes the ranked route"
    C = 3
    logits, labels = _inputs(T, C, 20)
    t, y = torch.from_numpy(logits).to(DEV), torch.from_numpy(labels).to(DEV)
    below, at = (M.MulticlassMeter(C, capacity=T, device=DEV) for _ in range(2))      # auroc="auto" is the default
    below.update(t[:T - 1], y[:T - 1])
    at.update(t, y)
    res = at.compute()
    below.compute()
    assert at._ws is not None and below._ws is None, "the route does not change between T - 1 and T rows"
    probs, stored = at.scores[:, :T].t().cpu().numpy(), at.labels[:T].cpu().numpy()
    assert np.array_equal(at.auroc_counts(), RR.pair_counts_sorted(probs, stored, C))
    assert np.array_equal(below.auroc_counts(), RR.pair_counts_sorted(probs[:T - 1], stored[:T - 1], C))
    pairs = M.MulticlassMeter(C, capacity=T, device=DEV, auroc="pairs")
    pairs.update(t, y)
    for k, v in pairs.compute().items():
        assert np.array_equal(_bits(res[k]), _bits(v)), k


def _sync_warnings(fn):
    """the number of synchronising calls torch reports while fn runs"""
    import warnings
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    return sum("synchroniz" in str(w.message) for w in seen)


def test_ranked_route_does_not_synchronise_before_the_one_copy():
    C = 7
    logits, labels = _inputs(sum(BATCHES), C, 19)
    t, y = torch.from_numpy(logits).to(DEV), torch.from_numpy(labels).to(DEV)
    warm = M.MulticlassMeter(C, capacity=64, device=DEV, auroc="ranked")
    warm.update(t, y)
    want = warm.compute()                                     # library loaded, allocator pools warm
    counts = torch.zeros((C, 4), dtype=torch.int64, device=DEV)
    probe = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            probe.cpu()
        except RuntimeError:
            raised = True
        assert raised, "torch.cuda.set_sync_debug_mode('error') does not raise for .cpu() in this build: the test cannot see a sync"
        # everything compute() does in front of its copy, on a meter that still has to grow and to make its workspace
        m = M.MulticlassMeter(C, capacity=64, device=DEV, auroc="ranked")
        m.update(t, y)
        M.metrics_auroc_ranked(m.scores, m.labels, m.n, counts, m._workspace(m.n))
        L.check(L.lib().hs_metrics_finalize(rt.p(m.cm), rt.p(counts), C, rt.p(m._out), rt.stream()), "hs_metrics_finalize")
        M.metrics_auroc_ranked(m.scores, m.labels, m.n, counts)                  # workspace=None: allocated, no sync either
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert np.array_equal(counts.cpu().numpy(), warm.auroc_counts())
    # compute() itself: as many synchronising calls as the pair route's, whose one copy is the only one
    pairs = M.MulticlassMeter(C, capacity=512, device=DEV, auroc="pairs")
    pairs.update(t, y)
    res = {}
    n_pairs = _sync_warnings(lambda: res.update(pairs=pairs.compute()))
    n_ranked = _sync_warnings(lambda: res.update(ranked=m.compute()))
    assert n_pairs >= 1, "no warning for the copy of compute(): the test cannot see a sync"
    assert n_ranked == n_pairs, f"{n_ranked} synchronising calls on the ranked route, {n_pairs} on the pair route"
    for k, v in want.items():
        assert np.array_equal(res["ranked"][k], v, equal_nan=True) and np.array_equal(res["pairs"][k], v, equal_nan=True), k
