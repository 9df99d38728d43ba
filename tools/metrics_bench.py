#!/usr/bin/env python
"""Cost of the validation metrics: hamspine.metrics.MulticlassMeter (csrc/metrics.hip) against what the validation loops do
without it -- per batch `argmax(...).cpu()` and `softmax(...).cpu()` of the logits, scikit-learn on the collected arrays at the
end (reference scripts/train.py:102-129, ConNexT/models/test.py:84-130).

    python tools/metrics_bench.py --out profiles/metrics.txt

Per (rows, classes): a validation pass in batches of 64 over logits that are already on the device.  Both ways run in one
process, alternating, `--rounds` times after a warm-up round; every figure is the median with the minimum and maximum.
  update    host clock from the first `update` to a device synchronise after the last, over the number of batches: what one
            batch costs the loop (launch overhead included); and device events around the same loop, over the batches
  compute   host clock around compute() (it ends in the one device-to-host copy); device events around the pair-count launch
            and around finalize
  baseline  host clock per batch of the two `.cpu()` copies, and around the scikit-learn calls at the end
The last line is the forward pass of one validation batch of the flagship model (bench.py's C2, batch 32, no_grad) in the same
process, the yardstick for the pair count.

    python tools/metrics_bench.py --ranked 2003x7,10000x7,50000x7,200000x7,1000000x7 --out profiles/metrics_ranked.txt

times compute() of two meters holding the same rows, auroc="pairs" and auroc="ranked", alternating, and names the smallest
measured row count from which the ranked route is faster by more than the spread (max - min over the rounds) of either route:
the value for hamspine.metrics.AUTO_RANKED_ROWS.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

BATCH = 64


def _fmt(v, unit="us", scale=1e3):
    return f"{statistics.median(v) * scale:10.1f} {unit}  (min {min(v) * scale:.1f}, max {max(v) * scale:.1f})"


def device_pass(meter, batches):
    """-> ms: (host per batch of update, device per batch of update, host compute, device auroc, device finalize)"""
    from hamspine import _lib as L
    from hamspine import metrics as M
    from hamspine import rt
    meter.reset()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev[0].record()
    for lg, lb in batches:
        meter.update(lg, lb)
    ev[1].record()
    torch.cuda.synchronize()
    upd_host = (time.perf_counter() - t0) * 1e3 / len(batches)
    upd_dev = ev[0].elapsed_time(ev[1]) / len(batches)
    # the two launches of compute(), with device events between them
    ev[2].record()
    M.metrics_auroc(meter.scores, meter.labels, meter.n, meter._counts)
    ev[3].record()
    L.check(L.lib().hs_metrics_finalize(rt.p(meter.cm), rt.p(meter._counts), meter.num_classes, rt.p(meter._out), rt.stream()),
            "hs_metrics_finalize")
    ev[4].record()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = meter.compute()
    comp_host = (time.perf_counter() - t0) * 1e3
    return (upd_host, upd_dev, comp_host, ev[2].elapsed_time(ev[3]), ev[3].elapsed_time(ev[4])), res


def host_pass(batches, C):
    """-> ms: (host per batch of the .cpu() copies, host of the scikit-learn calls), results"""
    import sklearn.metrics as sk
    preds, probs, labels = [], [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for lg, lb in batches:
        preds.append(lg.argmax(1).cpu())
        probs.append(torch.softmax(lg.float(), 1).cpu())
        labels.append(lb.cpu())
    per_batch = (time.perf_counter() - t0) * 1e3 / len(batches)
    t0 = time.perf_counter()
    y, p, s = torch.cat(labels).numpy(), torch.cat(preds).numpy(), torch.cat(probs).numpy().astype(np.float64)
    res = {"accuracy": sk.accuracy_score(y, p), "confusion_matrix": sk.confusion_matrix(y, p, labels=list(range(C)))}
    res["precision_macro"], res["recall_macro"], res["f1_macro"], _ = sk.precision_recall_fscore_support(
        y, p, average="macro", zero_division=0)
    pc = sk.precision_recall_fscore_support(y, p, average=None, labels=list(range(C)), zero_division=0)
    res["precision"], res["recall"], res["f1"] = pc[:3]
    res["auroc_macro"] = sk.roc_auc_score(y, s, multi_class="ovr", average="macro", labels=list(range(C)))
    end = (time.perf_counter() - t0) * 1e3
    return (per_batch, end), res


def c2_forward_ms(iters, warmup):
    import bench
    net, fwd_loss, _ = bench.build_workload("c2", torch.device("cuda:0"), 0)
    net.eval()
    with torch.no_grad():
        for _ in range(warmup):
            fwd_loss()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fwd_loss()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def ranked_lines(shapes, rounds):
    """compute() with auroc="pairs" against auroc="ranked" on the same stored rows"""
    from hamspine import metrics as M
    lines = [f"metrics_bench --ranked: MulticlassMeter.compute() on stored rows, auroc=\"pairs\" (hs_metrics_auroc) against "
             f"auroc=\"ranked\" (hs_metrics_auroc_ranked), one process, alternating; median of {rounds} rounds after one warm-up "
             "round (min, max); host clock around compute(), device events around the count launches alone",
             f"{'rows':>9} {'C':>3}  {'pairs compute()':>44}  {'ranked compute()':>44}  {'pairs count, device':>20}  "
             f"{'ranked count, device':>20}  ranked workspace"]
    threshold = None
    for shape in shapes.split(","):
        N, C = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(N + C)
        labels = torch.randint(0, C, (N,), generator=g)
        logits = torch.randn(N, C, generator=g)
        logits[torch.arange(N), labels] += 1.0
        logits, labels = logits.cuda(), labels.cuda()
        cap = 4096
        while cap < N:
            cap *= 2
        meters = {k: M.MulticlassMeter(C, capacity=cap, auroc=k) for k in ("pairs", "ranked")}
        for m in meters.values():
            for at in range(0, N, 65536):
                m.update(logits[at:at + 65536], labels[at:at + 65536])
        host, dev, res = {k: [] for k in meters}, {k: [] for k in meters}, {}
        scratch = torch.zeros((C, 4), dtype=torch.int64, device="cuda")
        for r in range(rounds + 1):
            for k, m in meters.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[k] = m.compute()
                dt = time.perf_counter() - t0
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                if k == "pairs":
                    M.metrics_auroc(m.scores, m.labels, m.n, scratch)
                else:
                    M.metrics_auroc_ranked(m.scores, m.labels, m.n, scratch, m._workspace(m.n))
                ev[1].record()
                torch.cuda.synchronize()
                if r:
                    host[k].append(dt * 1e3)
                    dev[k].append(ev[0].elapsed_time(ev[1]))
        assert np.array_equal(meters["pairs"].auroc_counts(), meters["ranked"].auroc_counts()), "the two routes count differently"
        for k, v in res["pairs"].items():
            assert np.array_equal(res["ranked"][k], v, equal_nan=True), k
        med = {k: statistics.median(v) for k, v in host.items()}
        spread = max(max(v) - min(v) for v in host.values())
        faster = med["pairs"] - med["ranked"] > spread
        if faster and threshold is None:
            threshold = N
        if not faster:
            threshold = None                                  # the ranked route has to stay ahead from the threshold on
        lines.append(f"{N:>9} {C:>3}  {_fmt(host['pairs']):>44}  {_fmt(host['ranked']):>44}  "
                     f"{statistics.median(dev['pairs']) * 1e3:>17.1f} us  {statistics.median(dev['ranked']) * 1e3:>17.1f} us  "
                     f"{M.auroc_ranked_ws_bytes(cap, C) / 2 ** 20:.2f} MiB   spread {spread * 1e3:.1f} us, ranked "
                     f"{'faster by more' if faster else 'not faster by more'}")
    lines.append(f"AUTO_RANKED_ROWS = {threshold}: the smallest measured row count from which the ranked route is faster by more than "
                 "the spread of either route (None: at no measured size)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranked", default=None, metavar="SHAPES", help="time auroc='pairs' against auroc='ranked' at these "
                    "rows x classes instead of the validation pass, e.g. 2003x7,50000x7")
    ap.add_argument("--shapes", default="2003x7,50000x7")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--forward-iters", type=int, default=30, help="C2 forward passes timed (0 skips that leg)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import hamspine
    from hamspine.metrics import MulticlassMeter
    hamspine.require_device()
    hamspine.set_compute_dtype("bf16")
    if args.ranked:
        lines = ranked_lines(args.ranked, args.rounds)
        args.shapes, args.forward_iters = "", 0
    else:
        lines = [f"metrics_bench: validation pass in batches of {BATCH}, f32 logits on the device; median of {args.rounds} alternating "
                 "rounds after one warm-up round (min, max)"]
    for shape in filter(None, args.shapes.split(",")):
        N, C = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(N + C)
        labels = torch.randint(0, C, (N,), generator=g)
        logits = torch.randn(N, C, generator=g)
        logits[torch.arange(N), labels] += 1.0
        logits, labels = logits.cuda(), labels.cuda()
        batches = [(logits[i:i + BATCH], labels[i:i + BATCH]) for i in range(0, N, BATCH)]
        cap = 4096
        while cap < N:
            cap *= 2
        meter = MulticlassMeter(C, capacity=cap)              # sized for the pass: no growth inside the timed loop
        dev, host = [], []
        for r in range(args.rounds + 1):
            d, res_d = device_pass(meter, batches)
            h, res_h = host_pass(batches, C)
            if r:
                dev.append(d)
                host.append(h)
        # same data both ways: the results agree (f32 softmax on both sides; the device counts pairs exactly)
        assert np.array_equal(res_d["confusion_matrix"], res_h["confusion_matrix"])
        for k in ("accuracy", "precision_macro", "recall_macro", "f1_macro"):
            assert abs(res_d[k] - res_h[k]) <= 1e-12, k
        auc_diff = abs(res_d["auroc_macro"] - res_h["auroc_macro"])
        dev, host = list(zip(*dev)), list(zip(*host))
        nb = len(batches)
        lines += [f"N = {N}, C = {C}: {nb} batches, {N * N * C / 1e9:.3f} G score pairs compared by the pair count",
                  f"  MulticlassMeter.update, per batch, host clock   {_fmt(dev[0])}",
                  f"  MulticlassMeter.update, per batch, device time  {_fmt(dev[1])}",
                  f"  MulticlassMeter.compute(), host clock           {_fmt(dev[2])}",
                  f"    hs_metrics_auroc, device time                 {_fmt(dev[3])}",
                  f"    hs_metrics_finalize, device time              {_fmt(dev[4])}",
                  f"  whole pass, device-side meter                   {(statistics.median(dev[0]) * nb + statistics.median(dev[2])):10.3f} ms",
                  f"  argmax().cpu() + softmax().cpu() + labels.cpu(), per batch, host clock  {_fmt(host[0])}",
                  f"  scikit-learn at the end (accuracy, confusion matrix, P/R/F1 macro and per class, ovr AUROC)  {_fmt(host[1], 'ms', 1.0)}",
                  f"  whole pass, host-side metrics                   {(statistics.median(host[0]) * nb + statistics.median(host[1])):10.3f} ms",
                  f"  |macro AUROC device - scikit-learn| = {auc_diff:.1e}"]
    if args.forward_iters > 0:
        lines.append(f"forward pass of one validation batch, C2 (ResNet-50 + BERT-base, batch 32, bf16, no_grad), same process, "
                     f"{args.forward_iters} passes after 5 warm-up: {c2_forward_ms(args.forward_iters, 5):.3f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
