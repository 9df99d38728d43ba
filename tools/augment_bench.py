#!/usr/bin/env python
"""Device time of the augmentation passes (hamspine.augment, csrc/augment.hip) for one training batch of the baseline
trainer's transform, per entry point and in total, next to the C2 step time of the same process.

    python tools/augment_bench.py --out profiles/augment.txt

Batch 32 of 450 x 600 sources -> (32, 3, 224, 224): RandomResizedCrop(scale 0.2..1), both flips, RandomRotation(45),
ColorJitter(0.2, 0.2, 0.2, 0.1), ImageNet Normalize.  Times are device events around each call, median over `--iters`
batches with fresh parameters, after a warm-up; the host columns are the wall time of drawing the parameters and of packing.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def c2_step_ms(steps, warmup):
    import bench
    net, fwd_loss, make_opt = bench.build_workload("c2", torch.device("cuda:0"), 0)
    opt = make_opt()

    def step():
        opt.zero_grad(set_to_none=True)
        fwd_loss().backward()
        opt.step()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=450)
    ap.add_argument("--width", type=int, default=600)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30, help="C2 steps timed (0 skips the step-time leg)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import hamspine
    from hamspine import _lib as L
    from hamspine import augment as A
    from hamspine import rt
    hamspine.require_device()
    hamspine.set_compute_dtype("bf16")
    lib = L.lib()
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (args.height, args.width, 3), dtype=np.uint8) for _ in range(args.batch)]
    t0 = time.perf_counter()
    host = A.pack_images(images)
    pack_ms = (time.perf_counter() - t0) * 1e3
    pack = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in host.items()}
    t = A.TrainTransform.baseline(size=args.size, generator=torch.Generator().manual_seed(0))
    h, w, off = A._pack_tables(pack)
    N, S = args.batch, args.size
    mean, std = (C.c_float * 3)(*t.mean), (C.c_float * 3)(*t.std)
    out = torch.empty((N, 3, S, S), dtype=torch.float32, device="cuda")
    names = ["plan", "resize", "stats", "finish"]
    times = {n: [] for n in names + ["total"]}
    sample_ms = []
    for it in range(args.warmup + args.iters):
        t0 = time.perf_counter()
        p = t.sample(pack)
        sample_ms.append((time.perf_counter() - t0) * 1e3)
        ip, fp = np.ascontiguousarray(p["iparams"]), np.ascontiguousarray(p["fparams"])
        ws_bytes = lib.hs_augment_ws_bytes(A._ptr(ip), N, S)
        ws = rt.workspace(ws_bytes, out.device)
        st = rt.stream()
        calls = [lambda: lib.hs_augment_plan(A._ptr(h), A._ptr(w), A._ptr(off), len(h), pack["arena"].numel(), A._ptr(ip), A._ptr(fp),
                                             N, S, rt.p(ws), ws_bytes, st),
                 lambda: lib.hs_augment_resize(rt.p(pack["arena"]), rt.p(ws), N, S, st),
                 lambda: lib.hs_augment_stats(rt.p(ws), N, S, st),
                 lambda: lib.hs_augment_finish(rt.p(ws), rt.p(out), N, S, mean, std, st)]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
        ev[0].record()
        for i, call in enumerate(calls):
            L.check(call(), names[i])
            ev[i + 1].record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            for i, n in enumerate(names):
                times[n].append(ev[i].elapsed_time(ev[i + 1]))
            times["total"].append(ev[0].elapsed_time(ev[-1]))
    med = {n: statistics.median(v) for n, v in times.items()}
    # the whole transform as a caller runs it, host work included, timed with a host clock around a synchronise
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        t(pack)
    torch.cuda.synchronize()
    call_ms = (time.perf_counter() - t0) / args.iters * 1e3
    step_ms = c2_step_ms(args.steps, 5) if args.steps > 0 else None
    lines = [f"augment_bench: batch {N} of {args.height}x{args.width} uint8 sources -> ({N}, 3, {S}, {S}) f32, baseline trainer's transform",
             f"device events around each entry point, median of {args.iters} batches (fresh parameters each), {args.warmup} warm-up:"]
    launches = {"plan": f"{(N + 15) // 16} launches", "resize": "2 launches", "stats": "1 launch", "finish": "1 launch"}
    for n in names:
        lines.append(f"  {n:7s} {med[n] * 1e3:9.1f} us   ({launches[n]}; min {min(times[n]) * 1e3:.1f}, max {max(times[n]) * 1e3:.1f})")
    lines.append(f"  total   {med['total'] * 1e3:9.1f} us   first event to last")
    lines.append(f"TrainTransform.__call__ (draw + plan + kernels, host clock around a synchronise): {call_ms:.3f} ms per batch")
    lines.append(f"host: drawing {N} parameter sets {statistics.median(sample_ms[args.warmup:]):.3f} ms; pack_images (pinned arena, "
                 f"{host['arena'].numel() / 1e6:.1f} MB) {pack_ms:.3f} ms on first use")
    if step_ms is not None:
        lines.append(f"C2 training step, same process, bf16, batch 32, {args.steps} steps after 5 warm-up: {step_ms:.3f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
