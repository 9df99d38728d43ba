"""Multiclass validation metrics accumulated on the device (csrc/metrics.hip, DESIGN.md "Device-side validation metrics").

Every validation loop of the reference pulls predictions to the host once per batch (`.cpu()` / `.item()` in scripts/train.py:
102-129, mibf_net/train_resnet.py:44-61, ConNexT/models/test.py:84-130, mibf_net/predict_resnet_ham_image.py:103-110) and hands
them to scikit-learn or torchmetrics.  `MulticlassMeter.update` is one kernel launch per batch with no synchronisation;
`compute()` reads the device back once.  All state is integer counts plus the stored f32 scores, so the result does not depend
on the order of the batches and two runs give the same bits.

Definitions (pinned on scikit-learn by tests/test_metrics_cpu.py through tests/metrics_ref.py):
  * per class, from the confusion matrix: precision tp/(tp+fp), recall tp/(tp+fn), F1 2tp/(2tp+fp+fn), 0 where the denominator
    is 0; per-class accuracy is recall (cm.diagonal() / cm.sum(1) of ConNexT/models/test.py:128-130, torchmetrics' multiclass
    Accuracy(average=None));
  * accuracy trace/total; macro averages over the classes with tp+fp+fn > 0 (torchmetrics' rule, scikit-learn's labels=None
    with zero_division=0); support-weighted averages as ConNexT/models/test.py:119-121;
  * AUROC one-vs-rest per class as (2 less + eq) / (2 P Nn) from exact pair counts; macro over the classes where it is defined.
    Departure from torchmetrics: a class without positives (or without negatives) is NaN and left out of the mean, where
    torchmetrics scores it 0 with a warning.

There is no CPU fallback and no collective: `merge` is for callers that shard validation inside one process.
"""
import numpy as np
import torch

from . import _lib as L
from . import rt

MAX_CLASSES, N_SCALARS, N_PER_CLASS = ABI_CONSTANTS = tuple(L._const("METRICS_MAX_CLASSES", "METRICS_SCALARS", "METRICS_PER_CLASS"))
SCALAR_KEYS = ("accuracy", "precision_macro", "recall_macro", "f1_macro", "precision_weighted", "recall_weighted", "f1_weighted",
               "auroc_macro")
PER_CLASS_KEYS = ("precision", "recall", "f1", "auroc", "support")
assert len(SCALAR_KEYS) == N_SCALARS and len(PER_CLASS_KEYS) == N_PER_CLASS


def _classes(C):
    if not 2 <= C <= MAX_CLASSES:
        raise L.HamspineError(f"metrics: {C} classes, supported 2..{MAX_CLASSES}")


def _labels(t, what):
    if t.dtype != torch.int64 or t.dim() != 1:
        raise TypeError(f"metrics: {what} is a 1-d int64 tensor, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def metrics_update(logits, labels, n, cm, invalid, scores=None, stored_labels=None, from_logits=True):
    """hs_metrics_update on caller-owned state: rows n .. n + B - 1 of `scores` (C, capacity) f32 / `stored_labels` (capacity,)
    int32, `cm` (C, C) int64, `invalid` one int64.  One launch on the current stream, no synchronisation."""
    rt.need_gpu(logits, labels, cm, invalid, scores, stored_labels)
    if logits.dim() != 2 or logits.shape[0] != labels.shape[0]:
        raise ValueError(f"metrics: logits (B, C) and labels (B,), got {tuple(logits.shape)} and {tuple(labels.shape)}")
    B, C = logits.shape
    _classes(C)
    if cm.dtype != torch.int64 or tuple(cm.shape) != (C, C) or not cm.is_contiguous() or invalid.dtype != torch.int64:
        raise TypeError("metrics: cm is a contiguous (C, C) int64 tensor and invalid an int64")
    capacity = 0
    if scores is not None:
        capacity = scores.shape[1]
        if (scores.dtype != torch.float32 or scores.shape[0] != C or not scores.is_contiguous() or stored_labels is None
                or stored_labels.dtype != torch.int32 or tuple(stored_labels.shape) != (capacity,)):
            raise TypeError("metrics: scores is a contiguous (C, capacity) f32 tensor with (capacity,) int32 labels")
    logits, labels = logits.contiguous(), _labels(labels, "labels")
    L.check(L.lib().hs_metrics_update(rt.hs_dtype(logits), rt.p(logits), rt.p(labels), B, C,
                                      int(n), capacity, rt.p(cm), rt.p(invalid), rt.p(scores), rt.p(stored_labels),
                                      int(bool(from_logits)), rt.stream()), "hs_metrics_update")


def metrics_auroc(scores, stored_labels, n, counts):
    """hs_metrics_auroc: counts (C, 4) int64 <- (less, eq, P, Nn) per class over the first n stored rows"""
    rt.need_gpu(scores, stored_labels, counts)
    C, capacity = scores.shape
    if (scores.dtype != torch.float32 or not scores.is_contiguous() or stored_labels.dtype != torch.int32
            or tuple(stored_labels.shape) != (capacity,)):
        raise TypeError("metrics: scores is a contiguous (C, capacity) f32 tensor with (capacity,) int32 labels")
    if counts.dtype != torch.int64 or tuple(counts.shape) != (C, 4) or not counts.is_contiguous():
        raise TypeError("metrics: counts is a contiguous (C, 4) int64 tensor")
    L.check(L.lib().hs_metrics_auroc(rt.p(scores), rt.p(stored_labels), int(n), capacity, C, rt.p(counts), rt.stream()),
            "hs_metrics_auroc")


class MulticlassMeter:
    """Confusion matrix, precision / recall / F1 / accuracy and one-vs-rest AUROC of a validation pass, kept on the device.

    update(logits, labels)            one launch per batch: arg-max, softmax, scores and label stored, one count added
    update_preds(pred_labels, labels) the confusion matrix alone (MetricCollection.update(pred_labels, labels))
    compute()                         AUROC pair counts + finalize, ONE device-to-host copy; raises on out-of-range labels
    reset() / merge(other)

    `capacity` rows of scores are preallocated and doubled when they run out (the host knows the row count, so growing needs
    no read-back either); keep_scores=False drops the scores and with them AUROC, which is then NaN."""

    def __init__(self, num_classes, capacity=4096, device="cuda", keep_scores=True):
        C = int(num_classes)
        _classes(C)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.HamspineError(f"MulticlassMeter runs on the HIP device only (got {self.device}); there is no CPU fallback")
        if capacity < 1:
            raise ValueError("MulticlassMeter: capacity is at least 1")
        self.num_classes, self.capacity, self.keep_scores, self.n = C, int(capacity), bool(keep_scores), 0
        # one tensor of 8-byte words, so that compute() is one copy: the f64 result vector | cm | invalid | AUROC counts
        self._n_out = N_SCALARS + N_PER_CLASS * C
        self._words = torch.zeros(self._n_out + C * C + 1 + 4 * C, dtype=torch.int64, device=self.device)
        w, o = self._words, self._n_out
        self._out = w[:o].view(torch.float64)
        self.cm = w[o:o + C * C].view(C, C)
        self.invalid = w[o + C * C:o + C * C + 1]
        self._counts = w[o + C * C + 1:].view(C, 4)
        self.scores = self.labels = None
        if self.keep_scores:
            self.scores = torch.empty((C, self.capacity), dtype=torch.float32, device=self.device)
            self.labels = torch.empty((self.capacity,), dtype=torch.int32, device=self.device)

    def _reserve(self, rows):
        """room for `rows` more stored rows: double the capacity as often as needed and copy, on the current stream"""
        if not self.keep_scores or self.n + rows <= self.capacity:
            return
        cap = self.capacity
        while self.n + rows > cap:
            cap *= 2
        scores = torch.empty((self.num_classes, cap), dtype=torch.float32, device=self.device)
        labels = torch.empty((cap,), dtype=torch.int32, device=self.device)
        scores[:, :self.n].copy_(self.scores[:, :self.n])
        labels[:self.n].copy_(self.labels[:self.n])
        self.scores, self.labels, self.capacity = scores, labels, cap

    def update(self, logits, labels, from_logits=True):
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"MulticlassMeter.update: logits are (B, {self.num_classes}), got {tuple(logits.shape)}")
        B = logits.shape[0]
        self._reserve(B)
        metrics_update(logits.detach(), labels, self.n, self.cm, self.invalid, self.scores, self.labels, from_logits)
        if self.keep_scores:
            self.n += B

    def update_preds(self, pred_labels, labels):
        rt.need_gpu(pred_labels, labels)
        if pred_labels.shape != labels.shape:
            raise ValueError("MulticlassMeter.update_preds: predictions and labels have one shape")
        pred_labels, labels = _labels(pred_labels, "pred_labels"), _labels(labels, "labels")
        L.check(L.lib().hs_metrics_update_preds(rt.p(pred_labels), rt.p(labels),
                                                labels.shape[0], self.num_classes, rt.p(self.cm), rt.p(self.invalid),
                                                rt.stream()), "hs_metrics_update_preds")

    def compute(self):
        C, o = self.num_classes, self._n_out
        if self.keep_scores:
            metrics_auroc(self.scores, self.labels, self.n, self._counts)
        L.check(L.lib().hs_metrics_finalize(rt.p(self.cm), rt.p(self._counts) if self.keep_scores else None, C,
                                            rt.p(self._out), rt.stream()), "hs_metrics_finalize")
        host = self._words.cpu().numpy()                      # the one device-to-host copy (and synchronisation)
        out, cm, invalid = host[:o].view(np.float64), host[o:o + C * C].reshape(C, C), int(host[o + C * C])
        if invalid > 0:
            raise L.HamspineError(f"MulticlassMeter: {invalid} rows had a label (or prediction) outside [0, {C})")
        res = {k: float(out[i]) for i, k in enumerate(SCALAR_KEYS)}
        for i, k in enumerate(PER_CLASS_KEYS):
            res[k] = out[N_SCALARS + i * C:N_SCALARS + (i + 1) * C].copy()
        res["accuracy_per_class"] = res["recall"].copy()
        res["support"] = res["support"].astype(np.int64)
        res["confusion_matrix"] = cm.copy()
        return res

    def auroc_counts(self):
        """(C, 4) int64 host array of (less, eq, P, Nn) per class, as the last compute() left them"""
        return self._counts.cpu().numpy()

    def reset(self):
        self._words.zero_()
        self.n = 0

    def merge(self, other):
        """add another meter's confusion matrix and append its stored rows (sharded validation inside one process)"""
        if other.num_classes != self.num_classes or other.keep_scores != self.keep_scores:
            raise ValueError("MulticlassMeter.merge: meters differ in num_classes or keep_scores")
        self.cm += other.cm.to(self.device)
        self.invalid += other.invalid.to(self.device)
        if self.keep_scores and other.n:
            self._reserve(other.n)
            self.scores[:, self.n:self.n + other.n].copy_(other.scores[:, :other.n])
            self.labels[self.n:self.n + other.n].copy_(other.labels[:other.n])
            self.n += other.n
        return self
