#!/usr/bin/env python
"""optimizer.step() of the Muon training config (reference configs/ham/ham_optimizer_muon_v1.yml, scripts/train.py:262-307):
hamspine.optim.MuonWithAuxAdam against the plain-torch restatement of tests/muon_ref.py running its Newton-Schulz iteration
in bf16 on GPU tensors (what a user of the published `muon` package gets).

The model of that config (ResNet18 + BERT-base + fusion_type "basic" + residual head + tabular branch) is built with
procedural weights, every parameter gets a seeded gradient, and step() is timed with device events after warm-up.  The two
optimizers alternate in the same process, `--steps` timed steps each per round, `--rounds` rounds to show the spread.
Prints one JSON line: ms/step of both, the FLOPs and bytes per step computed from the shapes, achieved TFLOP/s.

    python tools/muon_bench.py --dry-run          # shapes, groups, FLOPs, workspace bytes; needs no device
    python tools/muon_bench.py --steps 20 --rounds 3
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

NS_STEPS = 5
MUON_KW = dict(lr=0.02, weight_decay=0.01)                                   # muon_lr, muon_weight_decay of the config
AUX_KW = dict(lr=3e-4, betas=(0.9, 0.95), weight_decay=0.01)                # muon_aux_*


def build_model(device):
    import bench
    import model as product_model
    os.environ["HAMSPINE_BERT_RANDOM_INIT"] = "1"
    torch.manual_seed(1234)
    with tempfile.TemporaryDirectory() as tmp:
        net = product_model.MultimodalBaselineModel(
            num_classes=7, hidden_dim=256, dropout=0.3, pretrained_image=False, image_weights_path=None,
            text_model_name=bench.bert_base_dir(tmp), image_backbone="resnet18", classifier_type="residual", fusion_type="basic",
            tabular_enabled=True, tabular_input_dim=19, tabular_hidden_dim=128, tabular_dropout=0.1)
    return net.to(device).train()


def split(params):
    """scripts/train.py:289-306"""
    muon, aux = [p for p in params if p.ndim >= 2], [p for p in params if p.ndim < 2]
    return [dict(params=muon, use_muon=True, **MUON_KW), dict(params=aux, use_muon=False, **AUX_KW)]


def shape_groups(params):
    g = {}
    for p in params:
        if p.ndim >= 2:
            key = (p.shape[0], p.numel() // p.shape[0])
            g[key] = g.get(key, 0) + 1
    return g


def counts(groups, aux_elems, esz):
    """FLOPs (1 MAC = 2) of the Newton-Schulz products and bytes of every pass, each operand moved once, from the shapes"""
    flops = bytes_ = 0.0
    for (r, c), cnt in groups.items():
        n, k = min(r, c), max(r, c)
        flops += cnt * NS_STEPS * (4.0 * n * n * k + 2.0 * n ** 3)
        gemm = NS_STEPS * esz * ((n * k + n * n) + (2 * n * n) + (n * n + 2 * n * k))     # X->S ; S(+S)->B ; B,X->X'
        passes = 4.0 * (2 * 2 * n * k + n * k) + esz * n * k + esz * n * k + 4.0 * 2 * n * k   # momentum, pack, apply
        bytes_ += cnt * (gemm + passes)
    bytes_ += 28.0 * aux_elems            # Adam: 16 B read + 12 B written per element
    return flops, bytes_


def dry_run():
    net = build_model("cpu")
    params = [p for p in net.parameters() if p.requires_grad]
    groups = shape_groups(params)
    aux = sum(p.numel() for p in params if p.ndim < 2)
    try:
        from hamspine import _lib as L
        lib = L.lib()
    except Exception:
        lib = None
    print(f"{'rows':>6} {'cols':>6} {'count':>5} {'GFLOP/step':>11} {'ws MiB (bf16)':>14}")
    ws_max = 0
    for (r, c), cnt in sorted(groups.items(), key=lambda kv: -kv[1] * kv[0][0] * kv[0][1]):
        f, _ = counts({(r, c): cnt}, 0, 2)
        ws = int(lib.hs_muon_ws_bytes(L.HS_BF16, cnt, r, c)) if lib else -1
        ws_max = max(ws_max, ws)
        print(f"{r:6d} {c:6d} {cnt:5d} {f / 1e9:11.2f} {ws / 2 ** 20:14.1f}")
    flops, nbytes = counts(groups, aux, 2)
    c8 = lambda v: (v + 7) // 8 * 8
    packed = sum(cnt * c8(r) * c8(c) * 2 for (r, c), cnt in groups.items())
    print(json.dumps(dict(dry_run=True, muon_tensors=sum(groups.values()), shape_groups=len(groups), aux_tensors=sum(1 for p in params if p.ndim < 2),
                          muon_elements=sum(cnt * r * c for (r, c), cnt in groups.items()), aux_elements=aux,
                          tflop_per_step=flops / 1e12, gbytes_per_step_bf16=nbytes / 1e9, workspace_bytes_bf16=ws_max,
                          packed_bytes_bf16=packed, ms_per_step="not measured")))


def timed_steps(opt, steps):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in evs:
        a.record()
        opt.step()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--only", default="", choices=("", "ours", "ref"), help="one optimizer only (a profiler run)")
    a = ap.parse_args()
    if a.dry_run:
        return dry_run()
    if a.steps < 20 and not a.only:
        ap.error("--steps must be at least 20")
    import hamspine
    import muon_ref
    from hamspine.optim import MuonWithAuxAdam
    hamspine.require_device()
    hamspine.set_compute_dtype("bf16")
    net = build_model("cuda")
    params = [p for p in net.parameters() if p.requires_grad]
    gen = torch.Generator(device="cuda").manual_seed(77)
    for p in params:                              # seeded gradients in the parameter's own memory layout
        p.grad = torch.empty_like(p, memory_format=torch.preserve_format).normal_(generator=gen)
    clones = [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in params]
    for c, p in zip(clones, params):
        c.grad = p.grad
    ours = MuonWithAuxAdam(split(params))
    ref = muon_ref.RefMuonWithAuxAdam(split(clones), ns_dtype=torch.bfloat16)
    groups = shape_groups(params)
    flops, nbytes = counts(groups, sum(p.numel() for p in params if p.ndim < 2), 2)
    which = [("ours", ours), ("ref", ref)] if not a.only else [(a.only, ours if a.only == "ours" else ref)]
    for _, opt in which:
        for _ in range(a.warmup):
            opt.step()
    torch.cuda.synchronize()
    rounds = {name: [] for name, _ in which}
    for _ in range(a.rounds):
        for name, opt in which:                   # alternating in the same process
            rounds[name].append(statistics.median(timed_steps(opt, a.steps)))
    out = dict(workload="muon_v1: ResNet18 + BERT-base + basic fusion + residual head + tabular", mode="bf16", steps=a.steps,
               rounds=a.rounds, muon_tensors=sum(groups.values()), shape_groups=len(groups), tflop_per_step=flops / 1e12,
               gbytes_per_step=nbytes / 1e9)
    for name, _ in which:
        ms = rounds[name]
        out[f"{name}_ms_per_step"] = statistics.median(ms)
        out[f"{name}_ms_per_step_rounds"] = [round(v, 4) for v in ms]
        out[f"{name}_tflops"] = flops / 1e9 / statistics.median(ms)
    if not a.only:
        out["speedup_vs_ref"] = out["ref_ms_per_step"] / out["ours_ms_per_step"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
