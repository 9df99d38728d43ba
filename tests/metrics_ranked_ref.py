"""numpy restatement of the ranked route of csrc/metrics.hip (hs_metrics_auroc_ranked): per class the negatives' scores sorted,
every positive looked up with searchsorted.  tests/test_metrics_ranked_cpu.py pins it on metrics_ref.pair_counts (the n^2
form); it is the reference at sizes whose n^2 comparison matrix does not fit in memory.

A NaN score is set aside before the sort: such a row counts in P or Nn and takes part in no pair.  -0.0 and +0.0 compare equal
and denormals compare by value, as numpy's comparisons have it, so no key map is needed here."""
import numpy as np


def pair_counts_sorted(scores, labels, C):
    """(C, 4) int64 of (less, eq, P, Nn): scores (n, C), labels (n,) with -1 = neither positive nor negative"""
    scores, labels = np.asarray(scores), np.asarray(labels)
    out = np.zeros((C, 4), dtype=np.int64)
    for c in range(C):
        pos, neg = scores[labels == c, c], scores[(labels >= 0) & (labels != c), c]
        P, Nn = len(pos), len(neg)
        pos, neg = pos[~np.isnan(pos)], np.sort(neg[~np.isnan(neg)])
        lower, upper = np.searchsorted(neg, pos, side="left"), np.searchsorted(neg, pos, side="right")
        out[c] = (int(lower.sum()), int((upper - lower).sum()), P, Nn)
    return out


def bit_pattern_scores():
    """f32 scores whose keys exercise every digit of a 4 x 8-bit radix sort and the sign handling: k << 0, 8, 16, 24 for k in
    0..255 kept below the infinity pattern, the same with the sign bit set, +-0.0, denormals, +-inf"""
    k = np.arange(256, dtype=np.uint32)
    mags = np.concatenate([k << s for s in (0, 8, 16, 24)])
    mags = mags[mags < 0x7f800000]
    bits = np.concatenate([mags, mags | 0x80000000,
                           np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000,
                                     0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff], dtype=np.uint32)]).astype(np.uint32)
    vals = bits.view(np.float32)
    assert not np.isnan(vals).any()
    return vals


def meter_inputs(N, C, seed):
    """the logits and labels tests/test_metrics_gpu.py feeds its meters: quarters within +-4 (exact in bf16 too) with tied rows
    and repeated rows, every class among the labels"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, N)
    labels[:C] = np.arange(C)
    logits = rng.normal(size=(N, C))
    logits[np.arange(N), labels] += 0.8
    logits = np.clip(np.round(logits * 4) / 4, -4, 4)
    k = max(N // 8, 2)
    logits[N // 2:N // 2 + k] = logits[:k]
    return logits.astype(np.float32), labels.astype(np.int64)
