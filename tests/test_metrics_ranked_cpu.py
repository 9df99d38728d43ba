"""tests/metrics_ranked_ref.py::pair_counts_sorted (sort + searchsorted, the restatement of hs_metrics_auroc_ranked) pinned on
tests/metrics_ref.py::pair_counts (every pair compared), integer for integer, without a GPU; the declarations of the ranked
entry points; hamspine.metrics.shard_indices."""
import numpy as np
import pytest

import metrics_ref as R
import metrics_ranked_ref as RR


def _same(scores, labels, C):
    want, got = R.pair_counts(scores, labels, C), RR.pair_counts_sorted(scores, labels, C)
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    return want


@pytest.mark.parametrize("C", [2, 7])
@pytest.mark.parametrize("n", [1, 2, 3, 50, 300])
def test_random_scores(n, C):
    rng = np.random.default_rng(100 * n + C)
    _same(rng.random((n, C), dtype=np.float32), rng.integers(0, C, n), C)


@pytest.mark.parametrize("values", [(0.25, 0.75), (0.0, 0.5, 1.0)], ids=["two_valued", "three_valued"])
def test_heavy_ties(values):
    rng = np.random.default_rng(len(values))
    scores = rng.choice(np.array(values, dtype=np.float32), size=(300, 7))
    want = _same(scores, rng.integers(0, 7, 300), 7)
    assert (want[:, 1] > want[:, 0] / 4).all(), "ties do not dominate"


def test_all_scores_equal():
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 3, 50)
    want = _same(np.full((50, 3), 0.5, dtype=np.float32), labels, 3)
    assert (want[:, 0] == 0).all() and np.array_equal(want[:, 1], want[:, 2] * want[:, 3])


def test_signed_zeros_denormals_bit_patterns_and_nan():
    vals = RR.bit_pattern_scores()
    rng = np.random.default_rng(6)
    n = 2 * len(vals)
    scores = np.stack([rng.permutation(np.concatenate([vals, vals])) for _ in range(3)], axis=1)
    labels = rng.integers(0, 3, n)
    want = _same(scores, labels, 3)
    assert want[:, 1].min() > 0
    # -0.0 == +0.0, the smallest denormal is above both and its negative below: positives (0.0, 1e-45) against negatives
    # (-0.0, -1e-45) give three pairs below and one tie; the other way round only the tie
    z = np.array([[0.0], [-0.0], [1e-45], [-1e-45]], dtype=np.float32).repeat(2, axis=1)
    assert np.array_equal(_same(z, np.array([0, 1, 0, 1]), 2), [[3, 1, 2, 2], [0, 1, 2, 2]])
    # NaN among the positives only, the negatives only, and both
    for where in ("pos", "neg", "both"):
        s, y = scores.copy(), labels
        for c in range(3):
            pos, neg = np.flatnonzero(y == c), np.flatnonzero(y != c)
            if where in ("pos", "both"):
                s[pos[::3], c] = np.nan
            if where in ("neg", "both"):
                s[neg[::4], c] = np.nan
        got = _same(s, y, 3)
        assert np.array_equal(got[:, 2:], want[:, 2:]) and (got[:, 0] < want[:, 0]).all()


def test_unlabelled_rows_and_empty_sides():
    rng = np.random.default_rng(7)
    scores = np.round(rng.random((300, 7), dtype=np.float32) * 16) / 16
    labels = rng.integers(0, 7, 300)
    labels[::5] = -1
    want = _same(scores, labels, 7)
    assert (want[:, 2] + want[:, 3] == (labels >= 0).sum()).all()
    labels = np.where(labels == 4, 2, labels)                 # class 4 has no positives
    want = _same(scores, labels, 7)
    assert want[4, 2] == 0 and want[4, 0] == want[4, 1] == 0
    only = np.where(labels >= 0, 1, -1)                       # class 1 has no negatives, every other class no positives
    want = _same(scores, only, 7)
    assert want[1, 3] == 0 and (want[:, :2] == 0).all()


def test_declarations_of_the_ranked_entry_points():
    import hamspine._lib as L
    protos = L.parse_header(open(L.HEADER_PATH).read()).prototypes
    assert len(protos["hs_metrics_auroc_ranked"][1]) == 9 and len(protos["hs_metrics_auroc_ranked_ws_bytes"][1]) == 2
    assert len(protos["hs_metrics_auroc"][1]) == 7            # the pair kernel's entry is as it was


def test_shard_indices_cover_every_row_once_without_padding():
    from hamspine import metrics as M
    for n, world in ((101, 2), (7, 3), (2, 4), (0, 2)):
        shards = [list(M.shard_indices(n, r, world)) for r in range(world)]
        assert sorted(i for s in shards for i in s) == list(range(n))
        assert max(map(len, shards)) - min(map(len, shards)) <= 1
    assert list(M.shard_indices(5, 1, 2)) == [1, 3]
    with pytest.raises(ValueError):
        M.shard_indices(5, 2, 2)


def test_meter_arguments_are_checked_without_a_device():
    from hamspine import metrics as M
    assert M.AUTO_RANKED_ROWS is None or (isinstance(M.AUTO_RANKED_ROWS, int) and M.AUTO_RANKED_ROWS > 0)
    import inspect
    sig = inspect.signature(M.MulticlassMeter.__init__).parameters
    assert sig["auroc"].default == "auto" and sig["group"].default is None
    assert inspect.signature(M.MulticlassMeter.compute).parameters["group"].default is None
