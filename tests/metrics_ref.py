"""numpy restatement of csrc/metrics.hip: integer confusion matrix and AUROC pair counts, every division in f64.

tests/test_metrics_cpu.py pins this file on scikit-learn (1.7.2); the GPU tests hold the kernels against it."""
import numpy as np


def argmax_rows(logits):
    """lowest index among the largest values; NaN counts as the largest (numpy.argmax, torch.argmax)"""
    return np.argmax(np.asarray(logits), axis=1)


def softmax64(logits):
    z = np.asarray(logits, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)


def confusion(labels, preds, C):
    """(C, C) int64, row = label, column = prediction; rows with a label outside [0, C) are left out and counted"""
    labels, preds = np.asarray(labels, dtype=np.int64), np.asarray(preds, dtype=np.int64)
    ok = (labels >= 0) & (labels < C)
    cm = np.zeros((C, C), dtype=np.int64)
    np.add.at(cm, (labels[ok], preds[ok]), 1)
    return cm, int((~ok).sum())


def pair_counts(scores, labels, C):
    """(C, 4) int64 of (less, eq, P, Nn): scores (n, C), labels (n,) with -1 = neither positive nor negative.  Comparisons are
    made on the values as given (f32 stays f32); a NaN score compares false both ways."""
    scores, labels = np.asarray(scores), np.asarray(labels)
    out = np.zeros((C, 4), dtype=np.int64)
    for c in range(C):
        pos, neg = scores[labels == c, c], scores[(labels >= 0) & (labels != c), c]
        with np.errstate(invalid="ignore"):
            less = int((neg[None, :] < pos[:, None]).sum())
            eq = int((neg[None, :] == pos[:, None]).sum())
        out[c] = (less, eq, len(pos), len(neg))
    return out


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape, dtype=np.float64), where=den != 0)


def finalize(cm, counts=None):
    """the dict of MulticlassMeter.compute() from the integer counts"""
    cm = np.asarray(cm, dtype=np.int64)
    C = cm.shape[0]
    tp, support = np.diag(cm), cm.sum(1)
    fp, fn = cm.sum(0) - tp, support - tp
    prec, rec, f1 = _ratio(tp, tp + fp), _ratio(tp, tp + fn), _ratio(2 * tp, 2 * tp + fp + fn)
    seen = (tp + fp + fn) > 0
    total = float(support.sum())
    auroc = np.full(C, np.nan)
    if counts is not None:
        counts = np.asarray(counts, dtype=np.int64)
        for c in range(C):
            less, eq, P, Nn = (int(v) for v in counts[c])
            if P > 0 and Nn > 0:
                auroc[c] = float(2 * less + eq) / (2.0 * float(P) * float(Nn))
    defined = ~np.isnan(auroc)

    def macro(v):
        return float(_ratio(sum(float(x) for x in v[seen]), float(seen.sum())))

    def weighted(v):
        return float(_ratio(sum(float(s) * float(x) for s, x in zip(support, v)), total))

    return {"accuracy": float(_ratio(float(tp.sum()), total)),
            "precision_macro": macro(prec), "recall_macro": macro(rec), "f1_macro": macro(f1),
            "precision_weighted": weighted(prec), "recall_weighted": weighted(rec), "f1_weighted": weighted(f1),
            "auroc_macro": float(sum(float(x) for x in auroc[defined]) / defined.sum()) if defined.any() else float("nan"),
            "precision": prec, "recall": rec, "f1": f1, "accuracy_per_class": rec.copy(), "auroc": auroc,
            "support": support.astype(np.int64), "confusion_matrix": cm}


def metrics(logits, labels, C):
    """everything from logits (n, C) and labels (n,): arg-max, f64 softmax scores, counts, finalize"""
    labels = np.asarray(labels, dtype=np.int64)
    cm, invalid = confusion(labels, argmax_rows(logits), C)
    stored = np.where((labels >= 0) & (labels < C), labels, -1)
    res = finalize(cm, pair_counts(softmax64(logits), stored, C))
    res["invalid"] = invalid
    return res
