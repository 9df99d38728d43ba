"""csrc/metrics.hip against tests/metrics_ref.py (itself pinned on scikit-learn by tests/test_metrics_cpu.py) and scikit-learn.

Integer results (confusion matrix, arg-max, AUROC pair counts) are compared exactly; the stored probabilities against an f64
softmax at the project's f32 gate, 1e-4 of the maximum; compute() against scikit-learn at 1e-12 on the probabilities read back
from the device (both sides then divide the same integers in f64).

Batches of 1, 63, 64, 65 and 200 rows go into a meter of capacity 64: it grows three times (128, 256, 512) and the rows cross
the boundaries of the update kernel (4 rows per wave, 16 rows per block) and the 256-row j tiles of the pair count; its 512-row
i tiles are crossed by the 1100-row case below."""
import numpy as np
import pytest
import sklearn.metrics as sk
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from hamspine import metrics as M  # noqa: E402
from hamspine._lib import HamspineError  # noqa: E402

DEV = "cuda"
BATCHES = (1, 63, 64, 65, 200)
TOL = 1e-12


def _inputs(N, C, seed):
    """quantised logits (quarters within +-4: exact in bf16 too) with tied rows and repeated rows, every class among the labels"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, N)
    labels[:C] = np.arange(C)
    logits = rng.normal(size=(N, C))
    logits[np.arange(N), labels] += 0.8
    logits = np.clip(np.round(logits * 4) / 4, -4, 4)
    k = max(N // 8, 2)
    logits[N // 2:N // 2 + k] = logits[:k]
    return logits.astype(np.float32), labels.astype(np.int64)


def _feed(meter, logits, labels, dtype, sizes, order=None):
    chunks, at = [], 0
    for b in sizes:
        chunks.append((at, at + b))
        at += b
    assert at == len(labels)
    for i in (range(len(chunks)) if order is None else order):
        lo, hi = chunks[i]
        meter.update(torch.from_numpy(logits[lo:hi]).to(DEV, dtype), torch.from_numpy(labels[lo:hi]).to(DEV))
    return [c for i in (range(len(chunks)) if order is None else order) for c in range(*chunks[i])]


def _stored(meter):
    return meter.scores[:, :meter.n].t().cpu().numpy(), meter.labels[:meter.n].cpu().numpy().astype(np.int64)


@pytest.fixture(scope="module", params=[(2, torch.float32), (7, torch.float32), (7, torch.bfloat16), (64, torch.float32),
                                        (64, torch.bfloat16)], ids=lambda p: f"C{p[0]}_{str(p[1]).split('.')[-1]}")
def run(request):
    C, dtype = request.param
    N = sum(BATCHES)
    logits, labels = _inputs(N, C, 17 * C)
    meter = M.MulticlassMeter(C, capacity=64, device=DEV)
    _feed(meter, logits, labels, dtype, BATCHES)
    assert meter.n == N and meter.capacity == 512
    probs, stored = _stored(meter)
    res = meter.compute()
    return dict(C=C, dtype=dtype, logits=logits, labels=labels, probs=probs, stored=stored, res=res,
                counts=meter.auroc_counts(), scores=meter.scores[:, :N].clone(), cm=meter.cm.clone())


def test_confusion_matrix_and_stored_rows(run):
    C, logits, labels = run["C"], run["logits"], run["labels"]
    cm, _ = R.confusion(labels, R.argmax_rows(logits), C)
    assert np.array_equal(run["res"]["confusion_matrix"], cm)
    assert np.array_equal(run["stored"], labels)
    want = R.softmax64(logits)
    err = np.abs(run["probs"] - want).max() / want.max()
    print("softmax rel err", err)
    assert err <= 1e-4
    assert run["probs"].dtype == np.float32


def test_pair_counts_equal_the_restatement_on_the_read_back_probabilities(run):
    want = R.pair_counts(run["probs"], run["stored"], run["C"])
    assert want[:, 1].sum() > 0, "no tied scores"
    assert np.array_equal(run["counts"], want)


def test_compute_agrees_with_sklearn(run):
    C, labels, res, probs = run["C"], run["labels"], run["res"], run["probs"].astype(np.float64)
    preds = R.argmax_rows(run["logits"])
    p, r, f, s = sk.precision_recall_fscore_support(labels, preds, average=None, labels=list(range(C)), zero_division=0)
    for key, want in (("precision", p), ("recall", r), ("f1", f), ("accuracy_per_class", r)):
        assert np.abs(res[key] - want).max() <= TOL, key
    assert np.array_equal(res["support"], s) and res["support"].dtype == np.int64
    assert abs(res["accuracy"] - sk.accuracy_score(labels, preds)) <= TOL
    for avg in ("macro", "weighted"):
        p, r, f, _ = sk.precision_recall_fscore_support(labels, preds, average=avg, labels=list(range(C)), zero_division=0)
        for key, want in ((f"precision_{avg}", p), (f"recall_{avg}", r), (f"f1_{avg}", f)):
            assert abs(res[key] - want) <= TOL, key
    auc = np.array([sk.roc_auc_score((labels == c).astype(int), probs[:, c]) for c in range(C)])
    print("auroc diff", np.abs(res["auroc"] - auc).max())
    assert np.abs(res["auroc"] - auc).max() <= TOL
    assert abs(res["auroc_macro"] - auc.mean()) <= TOL
    if C > 2:
        want = sk.roc_auc_score(labels, probs, multi_class="ovr", average="macro", labels=list(range(C)))
        assert abs(res["auroc_macro"] - want) <= TOL
    ref = R.finalize(res["confusion_matrix"], run["counts"])
    for k, v in ref.items():
        assert np.allclose(res[k], v, rtol=0, atol=TOL, equal_nan=True), k


def test_reverse_order_gives_the_same_integers_and_two_runs_the_same_bits(run):
    C, dtype, logits, labels = run["C"], run["dtype"], run["logits"], run["labels"]
    again = M.MulticlassMeter(C, capacity=64, device=DEV)
    _feed(again, logits, labels, dtype, BATCHES)
    res = again.compute()
    assert torch.equal(again.scores[:, :again.n], run["scores"]) and torch.equal(again.cm, run["cm"])
    assert np.array_equal(again.auroc_counts(), run["counts"])
    for k, v in run["res"].items():
        assert np.array_equal(res[k], v, equal_nan=True), k
    rev = M.MulticlassMeter(C, capacity=64, device=DEV)
    rows = _feed(rev, logits, labels, dtype, BATCHES, order=range(len(BATCHES) - 1, -1, -1))
    assert rev.capacity == 512
    assert np.array_equal(_stored(rev)[0], run["probs"][rows])
    res = rev.compute()
    assert np.array_equal(rev.auroc_counts(), run["counts"])
    assert np.array_equal(res["confusion_matrix"], run["res"]["confusion_matrix"])
    for k, v in run["res"].items():
        assert np.array_equal(res[k], v, equal_nan=True), k


@pytest.mark.parametrize("C", [2, 7, 64])
def test_arg_max_per_row_with_heavy_ties(C):
    """one row per label: row i of the matrix is then the one-hot of row i's arg-max"""
    rng = np.random.default_rng(C)
    meter = M.MulticlassMeter(C, capacity=C, device=DEV, keep_scores=False)
    labels = torch.arange(C, device=DEV)
    for dtype in (torch.float32, torch.bfloat16):
        for _ in range(3):
            logits = (rng.integers(-1, 2, (C, C)) / 4).astype(np.float32)
            logits[0, :] = 0.0                                # every class ties: class 0
            logits[1, :] = -0.0
            logits[1, C - 1] = 0.0                            # -0 == +0: still class 0
            meter.reset()
            meter.update(torch.from_numpy(logits).to(DEV, dtype), labels)
            cm = meter.compute()["confusion_matrix"]
            assert np.array_equal(cm.sum(1), np.ones(C)) and np.array_equal(cm.argmax(1), np.argmax(logits, 1))


@pytest.mark.parametrize("N,C", [(1100, 3), (2600, 64), (4500, 64)])
def test_crosses_the_i_tile_and_takes_plain_scores(N, C):
    """several 512-row i tiles, and each way the pair count cuts the j range over the grid: 1100 x 3 one 256-row tile per span,
    2600 x 64 two spans of six tiles (the second ragged), 4500 x 64 one span; from_logits=False stores the values as given"""
    logits, labels = _inputs(N, C, 5)
    meter = M.MulticlassMeter(C, capacity=8192, device=DEV)
    meter.update(torch.from_numpy(logits).to(DEV), torch.from_numpy(labels).to(DEV), from_logits=False)
    probs, stored = _stored(meter)
    assert np.array_equal(probs, logits) and np.array_equal(stored, labels)
    res = meter.compute()
    assert np.array_equal(meter.auroc_counts(), R.pair_counts(logits, labels, C))
    auc = [sk.roc_auc_score((labels == c).astype(int), logits[:, c].astype(np.float64)) for c in range(C)]
    assert np.abs(res["auroc"] - auc).max() <= TOL


def test_one_row_single_positive_and_one_class():
    meter = M.MulticlassMeter(4, capacity=8, device=DEV)
    meter.update(torch.tensor([[0.0, 2.0, 1.0, 2.0]], device=DEV), torch.tensor([1], device=DEV))
    res = meter.compute()                                     # n = 1
    assert res["accuracy"] == 1.0 and res["confusion_matrix"][1, 1] == 1 and res["confusion_matrix"].sum() == 1
    assert np.isnan(res["auroc"]).all() and np.isnan(res["auroc_macro"])
    assert res["f1_macro"] == 1.0 and res["recall_weighted"] == 1.0
    # a single positive among 40 rows
    meter.reset()
    logits, labels = _inputs(40, 4, 3)
    labels = np.where(labels == 2, 0, labels)
    labels[11] = 2
    meter.update(torch.from_numpy(logits).to(DEV), torch.from_numpy(labels).to(DEV))
    probs, stored = _stored(meter)
    res = meter.compute()
    counts = meter.auroc_counts()
    assert counts[2, 2] == 1 and counts[2, 3] == 39 and np.array_equal(counts, R.pair_counts(probs, stored, 4))
    assert abs(res["auroc"][2] - sk.roc_auc_score((labels == 2).astype(int), probs[:, 2].astype(np.float64))) <= TOL
    # every row in one class: no class has positives and negatives
    meter.reset()
    meter.update(torch.from_numpy(logits).to(DEV), torch.ones(40, dtype=torch.int64, device=DEV))
    res = meter.compute()
    assert np.isnan(res["auroc"]).all() and np.isnan(res["auroc_macro"]) and res["support"][1] == 40
    assert np.array_equal(meter.auroc_counts()[:, 2:], [[0, 40], [40, 0], [0, 40], [0, 40]])


def test_bad_labels_and_non_finite_logits_touch_nothing_else():
    """ordinary data with labels outside [0, C) and NaN / inf logits, on state tensors with guard regions either side"""
    C, B, n0, cap, G = 7, 90, 5, 128, 64
    logits, labels = _inputs(B, C, 23)
    bad_rows, weird_rows = [3, 40, 77, 89], [10, 41, 60, 61]
    dirty, dirty_labels = logits.copy(), labels.copy()
    dirty_labels[bad_rows] = (C, -1, 2 ** 40, -2 ** 40)
    dirty[10, 2] = np.nan
    dirty[41, 5] = np.inf
    dirty[60, :] = -np.inf
    dirty[61, 1], dirty[61, 4] = np.inf, -np.nan
    dirty[3, :] = np.nan                                       # a bad label on a non-finite row

    def state():
        ints = torch.full((G + C * C + 1 + G,), -7, dtype=torch.int64, device=DEV)
        ints[G:G + C * C + 1] = 0
        scores = torch.full((G + C * cap + G,), 12345.0, dtype=torch.float32, device=DEV)
        stored = torch.full((G + cap + G,), -99, dtype=torch.int32, device=DEV)
        return ints, scores, stored

    def go(lg, lb):
        ints, scores, stored = state()
        before = [t.clone() for t in (ints, scores, stored)]
        M.metrics_update(torch.from_numpy(lg).to(DEV), torch.from_numpy(lb).to(DEV), n0, ints[G:G + C * C].view(C, C),
                         ints[G + C * C:G + C * C + 1], scores[G:G + C * cap].view(C, cap), stored[G:G + cap])
        torch.cuda.synchronize()
        for t, b in zip((ints, scores, stored), before):       # guards either side unchanged
            assert torch.equal(t[:G], b[:G]) and torch.equal(t[-G:], b[-G:])
        sc, st = scores[G:G + C * cap].view(C, cap), stored[G:G + cap]
        assert (sc[:, :n0] == 12345.0).all() and (sc[:, n0 + B:] == 12345.0).all()      # columns of other rows unchanged
        assert (st[:n0] == -99).all() and (st[n0 + B:] == -99).all()
        return (ints[G:G + C * C].view(C, C).cpu().numpy(), int(ints[G + C * C]), sc[:, n0:n0 + B].t().cpu().numpy(),
                st[n0:n0 + B].cpu().numpy())

    cm0, inv0, sc0, st0 = go(logits, labels)
    cm1, inv1, sc1, st1 = go(dirty, dirty_labels)
    assert inv0 == 0 and inv1 == len(bad_rows)
    good = np.setdiff1d(np.arange(B), bad_rows + weird_rows)
    assert np.array_equal(sc1[good], sc0[good]) and np.array_equal(st1[good], st0[good])
    assert (st1[bad_rows] == -1).all() and np.isnan(sc1[bad_rows]).all()
    valid = np.setdiff1d(np.arange(B), bad_rows)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(cm1, R.confusion(dirty_labels[valid], np.argmax(dirty[valid], 1), C)[0])
    assert np.isnan(sc1[10]).all() and np.isnan(sc1[60]).all()
    # the meter reports the bad labels
    meter = M.MulticlassMeter(C, capacity=128, device=DEV)
    meter.update(torch.from_numpy(dirty).to(DEV), torch.from_numpy(dirty_labels).to(DEV))
    with pytest.raises(HamspineError, match="4 rows"):
        meter.compute()
    with pytest.raises(HamspineError):
        meter.update(torch.from_numpy(logits), torch.from_numpy(labels))         # host tensors: no CPU fallback


def test_update_preds_merge_and_reset():
    C, N = 6, 300
    logits, labels = _inputs(N, C, 31)
    preds = R.argmax_rows(logits)
    a = M.MulticlassMeter(C, capacity=16, device=DEV)
    a.update_preds(torch.from_numpy(preds).to(DEV), torch.from_numpy(labels).to(DEV))
    res = a.compute()
    assert np.array_equal(res["confusion_matrix"], R.confusion(labels, preds, C)[0]) and a.n == 0
    assert np.isnan(res["auroc"]).all()
    ref = R.finalize(res["confusion_matrix"])
    for k in ("accuracy", "precision_macro", "recall_macro", "f1_macro", "f1_weighted"):
        assert abs(res[k] - ref[k]) <= TOL
    # two shards merged equal one meter fed everything
    whole, left, right = (M.MulticlassMeter(C, capacity=16, device=DEV) for _ in range(3))
    t, y = torch.from_numpy(logits).to(DEV), torch.from_numpy(labels).to(DEV)
    whole.update(t, y)
    left.update(t[:113], y[:113])
    right.update(t[113:], y[113:])
    left.merge(right)
    assert left.n == N and torch.equal(left.scores[:, :N], whole.scores[:, :N]) and torch.equal(left.labels[:N], whole.labels[:N])
    rw, rl = whole.compute(), left.compute()
    for k, v in rw.items():
        assert np.array_equal(rl[k], v, equal_nan=True), k
    assert np.array_equal(left.auroc_counts(), whole.auroc_counts())
    # a bad prediction is reported like a bad label
    a.update_preds(torch.tensor([C], device=DEV), torch.tensor([0], device=DEV))
    with pytest.raises(HamspineError):
        a.compute()
    a.reset()
    assert a.n == 0 and int(a.cm.sum()) == 0 and int(a.invalid) == 0
    assert a.compute()["accuracy"] == 0.0
    left.reset()
    left.update(t[:10], y[:10])
    assert left.n == 10 and int(left.cm.sum()) == 10
    # keep_scores=False: the matrix alone
    lean = M.MulticlassMeter(C, device=DEV, keep_scores=False)
    lean.update(t, y)
    res = lean.compute()
    assert lean.scores is None and np.array_equal(res["confusion_matrix"], rw["confusion_matrix"]) and np.isnan(res["auroc_macro"])
