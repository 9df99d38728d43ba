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

The pair counts come from one of two kernels with the same integers: `auroc="pairs"` compares every (positive, negative) pair,
O(C n^2); `auroc="ranked"` sorts each class's negatives and looks every positive up, O(C n log n).  `"auto"` takes the pair
kernel below AUTO_RANKED_ROWS rows and the ranked route from there on.

Across ranks (DESIGN.md "Rank-based AUROC and metrics over all ranks"): `compute(group=...)` returns, on every rank, the metrics
of the union of all ranks' rows -- the confusion matrices are summed as integers, the stored rows gathered in rank order, and
every rank divides the same integers.  Shard the validation set with `shard_indices`, not with a padding sampler.  `merge` is
for callers that shard validation inside one process.  There is no CPU fallback.
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


def _auroc_args(scores, stored_labels, counts):
    rt.need_gpu(scores, stored_labels, counts)
    C, capacity = scores.shape
    if (scores.dtype != torch.float32 or not scores.is_contiguous() or stored_labels.dtype != torch.int32
            or tuple(stored_labels.shape) != (capacity,)):
        raise TypeError("metrics: scores is a contiguous (C, capacity) f32 tensor with (capacity,) int32 labels")
    if counts.dtype != torch.int64 or tuple(counts.shape) != (C, 4) or not counts.is_contiguous():
        raise TypeError("metrics: counts is a contiguous (C, 4) int64 tensor")
    return C, capacity


def metrics_auroc(scores, stored_labels, n, counts):
    """hs_metrics_auroc: counts (C, 4) int64 <- (less, eq, P, Nn) per class over the first n stored rows"""
    C, capacity = _auroc_args(scores, stored_labels, counts)
    L.check(L.lib().hs_metrics_auroc(rt.p(scores), rt.p(stored_labels), int(n), capacity, C, rt.p(counts), rt.stream()),
            "hs_metrics_auroc")


def auroc_ranked_ws_bytes(n, C):
    """bytes of workspace with which hs_metrics_auroc_ranked sorts all C classes of n rows side by side"""
    need = L.lib().hs_metrics_auroc_ranked_ws_bytes(int(n), int(C))
    if need < 0:
        raise L.HamspineError(f"metrics: {n} rows of {C} classes are outside the limits of hs_metrics_auroc_ranked")
    return need


def metrics_auroc_ranked(scores, stored_labels, n, counts, workspace=None):
    """hs_metrics_auroc_ranked: the counts of metrics_auroc, integer for integer, by sorting.  `workspace` is a contiguous
    uint8 device tensor (None: one of auroc_ranked_ws_bytes(n, C) is allocated); a smaller one that still holds one class makes
    the kernels take the classes in several rounds.  No synchronisation."""
    C, capacity = _auroc_args(scores, stored_labels, counts)
    if workspace is None:
        workspace = torch.empty(auroc_ranked_ws_bytes(n, C), dtype=torch.uint8, device=scores.device)
    rt.need_gpu(workspace)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise TypeError("metrics: workspace is a contiguous uint8 tensor")
    L.check(L.lib().hs_metrics_auroc_ranked(rt.p(scores), rt.p(stored_labels), int(n), capacity, C,
                                            rt.p(workspace) if workspace.numel() else None, workspace.numel(), rt.p(counts),
                                            rt.stream()), "hs_metrics_auroc_ranked")


def shard_indices(n, rank, world):
    """The rows of rank `rank` when `world` ranks share a validation set of n rows: range(rank, n, world), unpadded.  Every row
    belongs to exactly one rank, and the shards may differ in length by one.  torch.utils.data.DistributedSampler instead pads
    the shards to one length by repeating samples; `compute(group=...)` would count those rows twice.  Use it as
    `Subset(dataset, shard_indices(len(dataset), rank, world))` with a plain sequential loader."""
    n, rank, world = int(n), int(rank), int(world)
    if world < 1 or not 0 <= rank < world or n < 0:
        raise ValueError(f"shard_indices: rank {rank} of {world} over {n} rows")
    return range(rank, n, world)


# "auto" takes the ranked route from this many rows on (None: never): the smallest measured row count at which compute() was
# faster that way by more than the spread of repeated runs (profiles/metrics_ranked.txt)
AUTO_RANKED_ROWS = 10000


def _resolve_group(group):
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise L.HamspineError("MulticlassMeter(group=...): torch.distributed is not initialised")
    return dist.group.WORLD if isinstance(group, str) and group == "world" else group


def _gather(t, pg, world, nccl):
    """(world,) + t.shape: the equally shaped t of every rank in rank order, on t's device for nccl, else on the host"""
    import torch.distributed as dist
    if nccl:
        out = torch.empty((world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        dist.all_gather_into_tensor(out, t.contiguous(), group=pg)
        return out
    out = torch.empty((world,) + tuple(t.shape), dtype=t.dtype)
    dist.all_gather(list(out.unbind(0)), t.cpu().contiguous(), group=pg)
    return out


class MulticlassMeter:
    """Confusion matrix, precision / recall / F1 / accuracy and one-vs-rest AUROC of a validation pass, kept on the device.

    update(logits, labels)            one launch per batch: arg-max, softmax, scores and label stored, one count added
    update_preds(pred_labels, labels) the confusion matrix alone (MetricCollection.update(pred_labels, labels))
    compute(group=None)               AUROC pair counts + finalize, ONE device-to-host copy; raises on out-of-range labels
    reset() / merge(other)

    `capacity` rows of scores are preallocated and doubled when they run out (the host knows the row count, so growing needs
    no read-back either); keep_scores=False drops the scores and with them AUROC, which is then NaN.

    auroc   "pairs" (hs_metrics_auroc), "ranked" (hs_metrics_auroc_ranked; its workspace belongs to the meter, is reused between
            calls and grows with the score buffer) or "auto" (by AUTO_RANKED_ROWS); the integers are the same either way
    group   a torch.distributed process group or "world": compute() then returns the metrics of ALL ranks' rows on every rank.
            Every rank of the group must call it.  The ranks may hold different numbers of rows, none included.  Local state is
            left as it was.  On this route compute() synchronises with the host more than once (the row counts travel first)."""

    def __init__(self, num_classes, capacity=4096, device="cuda", keep_scores=True, auroc="auto", group=None):
        C = int(num_classes)
        _classes(C)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.HamspineError(f"MulticlassMeter runs on the HIP device only (got {self.device}); there is no CPU fallback")
        if capacity < 1:
            raise ValueError("MulticlassMeter: capacity is at least 1")
        if auroc not in ("pairs", "ranked", "auto"):
            raise ValueError(f"MulticlassMeter: auroc is 'pairs', 'ranked' or 'auto', got {auroc!r}")
        self.num_classes, self.capacity, self.keep_scores, self.n = C, int(capacity), bool(keep_scores), 0
        self.auroc, self.group = auroc, group
        # one tensor of 8-byte words, so that compute() is one copy: the f64 result vector | cm | invalid | AUROC counts
        self._n_out = N_SCALARS + N_PER_CLASS * C
        self._words = torch.zeros(self._n_out + C * C + 1 + 4 * C, dtype=torch.int64, device=self.device)
        self._out, self.cm, self.invalid, self._counts = self._views(self._words)
        self._last_counts = self._counts
        self._ws, self._ws_rows = None, 0
        self.scores = self.labels = None
        if self.keep_scores:
            self.scores = torch.empty((C, self.capacity), dtype=torch.float32, device=self.device)
            self.labels = torch.empty((self.capacity,), dtype=torch.int32, device=self.device)

    def _views(self, w):
        C, o = self.num_classes, self._n_out
        return w[:o].view(torch.float64), w[o:o + C * C].view(C, C), w[o + C * C:o + C * C + 1], w[o + C * C + 1:].view(C, 4)

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

    def _workspace(self, rows):
        """the ranked route's workspace for `rows` rows: kept, and sized for the score buffer so that it grows when that does"""
        if self._ws is None or self._ws_rows < rows:
            self._ws_rows = max(rows, self.capacity)
            self._ws = torch.empty(auroc_ranked_ws_bytes(self._ws_rows, self.num_classes), dtype=torch.uint8, device=self.device)
        return self._ws

    def _finish(self, words, scores, labels, n):
        """pair counts of the n rows + finalize into `words` (whose cm and invalid are set), the ONE device-to-host copy
        (and synchronisation), the result dict"""
        C, o = self.num_classes, self._n_out
        out, cm, _, counts = self._views(words)
        if self.keep_scores:
            ranked = self.auroc == "ranked" or (self.auroc == "auto" and AUTO_RANKED_ROWS is not None and n >= AUTO_RANKED_ROWS)
            if ranked:
                metrics_auroc_ranked(scores, labels, n, counts, self._workspace(n))
            else:
                metrics_auroc(scores, labels, n, counts)
        L.check(L.lib().hs_metrics_finalize(rt.p(cm), rt.p(counts) if self.keep_scores else None, C,
                                            rt.p(out), rt.stream()), "hs_metrics_finalize")
        self._last_counts = counts
        host = words.cpu().numpy()
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

    def compute(self, group=None):
        group = self.group if group is None else group
        if group is not None:
            return self._compute_group(_resolve_group(group))
        return self._finish(self._words, self.scores, self.labels, self.n)

    def _compute_group(self, pg):
        """Every rank counts the union.  The collectives, the same on every rank and in this order: (1) all-gather of
        (num_classes, keep_scores, n); (2) all-reduce SUM of cm and invalid, int64; (3) all-gather of the stored labels and (4)
        of the stored scores, each padded to the longest shard -- (3) and (4) only with keep_scores and at least one row
        somewhere.  A mismatch raises on every rank after (1), a bad label anywhere on every rank at the end: (2) has summed
        `invalid`.  No floating-point value is reduced."""
        import torch.distributed as dist
        C, o = self.num_classes, self._n_out
        world, nccl = dist.get_world_size(pg), dist.get_backend(pg) == "nccl"
        wire = self.device if nccl else torch.device("cpu")
        heads = _gather(torch.tensor([C, int(self.keep_scores), self.n], dtype=torch.int64, device=wire), pg, world, nccl)
        heads = [tuple(h) for h in heads.cpu().tolist()]
        if any(h[:2] != heads[0][:2] for h in heads):
            raise L.HamspineError("MulticlassMeter.compute(group=...): the ranks differ in (num_classes, keep_scores): "
                                  f"{[h[:2] for h in heads]}")
        ns = [h[2] for h in heads]
        N, longest = sum(ns), max(ns)
        if N >= 2 ** 31:
            raise L.HamspineError(f"MulticlassMeter.compute(group=...): {N} rows over all ranks, supported below 2^31")
        ints = self._words[o:o + C * C + 1].to(wire, copy=True)
        dist.all_reduce(ints, op=dist.ReduceOp.SUM, group=pg)
        words = torch.zeros_like(self._words)
        words[o:o + C * C + 1].copy_(ints)
        scores = labels = None
        if self.keep_scores and N > 0:
            mine_l = torch.empty((longest,), dtype=torch.int32, device=self.device)
            mine_s = torch.empty((C, longest), dtype=torch.float32, device=self.device)
            mine_l[:self.n].copy_(self.labels[:self.n])
            mine_s[:, :self.n].copy_(self.scores[:, :self.n])
            all_l, all_s = _gather(mine_l, pg, world, nccl), _gather(mine_s, pg, world, nccl)
            labels = torch.empty((N,), dtype=torch.int32, device=self.device)
            scores = torch.empty((C, N), dtype=torch.float32, device=self.device)
            at = 0
            for r, k in enumerate(ns):                                # rank order; the padding stays behind
                labels[at:at + k].copy_(all_l[r, :k])
                scores[:, at:at + k].copy_(all_s[r, :, :k])
                at += k
        elif self.keep_scores:
            scores = torch.empty((C, 1), dtype=torch.float32, device=self.device)
            labels = torch.empty((1,), dtype=torch.int32, device=self.device)
        return self._finish(words, scores, labels, N)

    def auroc_counts(self):
        """(C, 4) int64 host array of (less, eq, P, Nn) per class, as the last compute() left them"""
        return self._last_counts.cpu().numpy()

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
