#!/usr/bin/env python
"""What global gradient-norm clipping costs per training step of C2 (bench.py's flagship: ResNet50 + BERT-base(L=128) + fusion
+ MLP head, 224x224, batch 32, bf16 mode), on three routes that alternate in ONE process on the same model:

    a   FusedAdamW, no clipping
    b   torch.nn.utils.clip_grad_norm_(parameters, 1.0) + FusedAdamW.step()      (the only route without csrc/gradclip.hip)
    c   FusedAdamW(max_grad_norm=1.0)                                            (sum-of-squares + finish + _clip step kernels)

One step = zero_grad -> forward -> loss -> backward -> [clip] -> step, as bench.py runs it.  Per step two device-event
intervals are taken: the whole step, and the optimizer section alone (everything after backward).  Every route keeps its own
optimizer state; after warm-up the routes run `--steps` steps each per round, `--rounds` rounds.  Reported per route: the median
over all timed steps, and the spread (min, max and standard deviation of the per-round medians).  The costs of b and c are their
medians minus a's; the spread of a is the noise a difference has to exceed.

    python tools/clip_bench.py --dry-run                      # tensors, elements, bytes per pass, launches; needs no device
    python tools/clip_bench.py --steps 20 --rounds 5
    python tools/clip_bench.py --steps 20 --rounds 5 --max-norm 0.02      # a coefficient below 1 in every step
    rocprofv3 --kernel-trace --stats -d DIR -o clip -- python tools/clip_bench.py --only c --steps 10 --rounds 1
    python tools/clip_bench.py --trace DIR --trace-steps 13   # bytes over time of the sum-of-squares kernels in that trace
"""
import argparse
import csv
import glob
import json
import os
import sqlite3
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_ACHIEVABLE_TBS = 6.3          # MI355X: achievable HBM bandwidth
MAX_NORM = 1.0


def shape_counts(params):
    """from the shapes alone: what each route reads and writes on top of the unclipped step"""
    from hamspine import _lib as L
    n = sum(p.numel() for p in params)
    t = len(params)
    return dict(tensors=t, elements=n, grad_bytes=4 * n,
                fused_extra_bytes=4 * n,                       # one more read of every gradient; nothing extra written
                torch_extra_bytes=3 * 4 * n,                   # norm read, scale read + write
                sumsq_launches=-(-t // L.GRADCLIP_MAX), adam_launches=-(-t // L.ADAM_MAX))


def trace_rows(path):
    """(kernel name, duration ns) of every kernel in a rocprofv3 output directory (rocpd database or csv)"""
    rows = []
    for db in glob.glob(os.path.join(path, "**", "*_results.db"), recursive=True):
        con = sqlite3.connect(db)
        try:
            rows += con.execute("select name, end - start from kernels").fetchall()
        finally:
            con.close()
    if not rows:
        for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                rows.append((r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    return rows


def trace_report(path, steps, grad_bytes):
    rows = trace_rows(path)
    if not rows:
        raise SystemExit(f"no kernel trace under {path}")
    out = {}
    for key in ("grad_sumsq_kernel", "grad_norm_finish_kernel", "adam_multi_kernel"):
        sel = [d for n, d in rows if key in n]
        out[key] = dict(calls=len(sel), total_us=sum(sel) / 1e3, us_per_step=sum(sel) / 1e3 / steps if steps else None)
    ss = out["grad_sumsq_kernel"]
    if ss["calls"] and steps:
        tbs = grad_bytes / (ss["total_us"] / steps * 1e-6) / 1e12
        out["sumsq_bytes_per_step"] = grad_bytes
        out["sumsq_tb_per_s"] = tbs
        out["sumsq_share_of_achievable_hbm"] = tbs / HBM_ACHIEVABLE_TBS
        out["hbm_achievable_tb_per_s"] = HBM_ACHIEVABLE_TBS
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", choices=("", "a", "b", "c"), help="one route only (a profiler run)")
    ap.add_argument("--max-norm", type=float, default=MAX_NORM, help="below the batch's gradient norm the coefficient is < 1")
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--trace", default="", help="a rocprofv3 output directory of an `--only c` run: report the kernels' bytes over time")
    ap.add_argument("--trace-steps", type=int, default=0, help="steps in that trace (warm-up + timed)")
    a = ap.parse_args()

    import torch
    import bench
    import hamspine
    from hamspine.optim import FusedAdamW

    if a.dry_run or a.trace:
        # shapes only: the model on the meta device
        import model as product_model
        import tempfile
        os.environ["HAMSPINE_BERT_RANDOM_INIT"] = "1"
        with tempfile.TemporaryDirectory() as tmp, torch.device("meta"):
            net = product_model.MultimodalBaselineModel(
                num_classes=7, hidden_dim=256, dropout=0.2, pretrained_image=False, image_weights_path=None,
                text_model_name=bench.bert_base_dir(tmp), num_heads=8, image_backbone="resnet50", classifier_type="mlp",
                fusion_type="basic")
        counts = shape_counts([p for p in net.parameters() if p.requires_grad])
        if a.trace:
            return trace_report(a.trace, a.trace_steps, counts["grad_bytes"])
        print(json.dumps(dict(dry_run=True, **counts, ms_per_step="not measured")))
        return

    hamspine.require_device()
    hamspine.set_compute_dtype("bf16")
    net, fwd_loss, _ = bench.build_workload("c2", "cuda", 0)
    params = [p for p in net.parameters() if p.requires_grad]
    kw = dict(lr=1e-4, weight_decay=0.01)
    routes = {"a": (FusedAdamW(params, **kw), False), "b": (FusedAdamW(params, **kw), True),
              "c": (FusedAdamW(params, max_grad_norm=a.max_norm, **kw), False)}
    names = [a.only] if a.only else ["a", "b", "c"]

    def step(name, timed):
        opt, torch_clip = routes[name]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timed else None
        if timed:
            ev[0].record()
        opt.zero_grad(set_to_none=True)
        fwd_loss().backward()
        if timed:
            ev[1].record()
        if torch_clip:
            torch.nn.utils.clip_grad_norm_(params, a.max_norm)
        opt.step()
        if timed:
            ev[2].record()
        return ev

    for name in names:
        for _ in range(a.warmup):
            step(name, False)
    torch.cuda.synchronize()
    whole = {n: [] for n in names}
    section = {n: [] for n in names}
    for _ in range(a.rounds):
        for name in names:                               # alternating in the same process
            evs = [step(name, True) for _ in range(a.steps)]
            torch.cuda.synchronize()
            whole[name].append([e[0].elapsed_time(e[2]) for e in evs])
            section[name].append([e[1].elapsed_time(e[2]) for e in evs])

    def summary(rounds):
        meds = [statistics.median(r) for r in rounds]
        return dict(median=statistics.median([v for r in rounds for v in r]), round_medians=[round(m, 4) for m in meds],
                    min=min(meds), max=max(meds), stdev=statistics.pstdev(meds))

    out = dict(workload=bench.WORKLOADS["c2"][3], mode="bf16", steps=a.steps, rounds=a.rounds, warmup=a.warmup, max_norm=a.max_norm,
               **shape_counts(params))
    for name in names:
        out[f"{name}_step_ms"] = summary(whole[name])
        out[f"{name}_optimizer_section_ms"] = summary(section[name])
    if not a.only:
        for key in ("step_ms", "optimizer_section_ms"):
            base = out[f"a_{key}"]
            out[f"cost_{key}"] = dict(b_minus_a=out[f"b_{key}"]["median"] - base["median"],
                                      c_minus_a=out[f"c_{key}"]["median"] - base["median"],
                                      spread_of_a=base["max"] - base["min"], stdev_of_a=base["stdev"])
        d = out["cost_optimizer_section_ms"]
        out["fused_cheaper_by_more_than_the_spread"] = bool(d["b_minus_a"] - d["c_minus_a"] > d["spread_of_a"])
    oc = routes["c"][0]
    out["last_grad_norm"] = None if oc.grad_norm is None else float(oc.grad_norm)
    out["last_clip_coef"] = None if oc.grad_clip_coef is None else float(oc.grad_clip_coef)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
