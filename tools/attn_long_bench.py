"""Attention forward + backward through hamspine.convnext_ops.attention_core at BERT-base shapes beyond 128 keys, fused
kernels against the GEMM + softmax fallback (HAMSPINE_FUSED_ATTENTION=0).

The switch is read once per process, so each path runs in a fresh child process.  Prints one table row per case:
median milliseconds of forward + backward over --iters timed iterations (after --warmup), each iteration timed with
CUDA events around both directions.

    python tools/attn_long_bench.py [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd")

# (name, B, H, L, ragged): B*H = 32*12 at the MIBF loader's 256 tokens, 64*12 at BERT's 512, and one ragged key mask
CASES = [
    ("L256 B32", 32, 12, 256, False),
    ("L512 B64", 64, 12, 512, False),
    ("L512 B64 ragged", 64, 12, 512, True),
]


def child(iters, warmup):
    sys.path.insert(0, PKG)
    import torch

    import hamspine
    from hamspine import convnext_ops as X
    hamspine.set_compute_dtype("bf16")
    res = {}
    for name, B, H, L, ragged in CASES:
        g = torch.Generator().manual_seed(L)
        q, k, v, do = (torch.randn(B, L, H * 64, generator=g).bfloat16().to("cuda") for _ in range(4))
        mask = None
        if ragged:
            lens = torch.randint(L // 4, L + 1, (B,), generator=g)
            mask = (torch.arange(L)[None, :] < lens[:, None]).long().to("cuda")
        q, k, v = (t.requires_grad_(True) for t in (q, k, v))
        times = []
        for it in range(warmup + iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = X.attention_core(q, k, v, heads=H, scale=0.125, key_mask=mask)
            out.backward(do)
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times.append(e0.elapsed_time(e1))
            q.grad = k.grad = v.grad = None
        times.sort()
        res[name] = times[len(times) // 2]
        del q, k, v, do, out
        torch.cuda.empty_cache()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.iters, a.warmup)
        return
    out = {}
    for label, flag in (("fused", "1"), ("fallback", "0")):
        env = dict(os.environ, HAMSPINE_FUSED_ATTENTION=flag)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--warmup",
                            str(a.warmup)], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"{label} child exited with {r.returncode}")
        out[label] = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"{'case (fwd+bwd, hd 64)':<24} {'fused ms':>10} {'fallback ms':>12} {'speed-up':>9}")
    for name, *_ in CASES:
        f, u = out["fused"][name], out["fallback"][name]
        print(f"{name:<24} {f:>10.3f} {u:>12.3f} {u / f:>8.2f}x")


if __name__ == "__main__":
    main()
