#!/usr/bin/env python
"""SupCon loss + gradient: the single-workgroup entry (hs_supcon_loss, B <= 256) against the tiled MFMA entry (hs_supcon_tiled),
alternating in ONE process on the same seeded features, at B = 32, 64, 128, 256 with D = 128, 512; then the tiled entry alone at
B = 512 ... 8192 (the single-workgroup entry refuses those).

One timed window = back-to-back calls of one entry between two device events (the calls are asynchronous; the window ends
in a synchronise), as many as fill about `--window-ms` and `--iters` at least, reported as microseconds per call.  Every
(entry, shape) is warmed up first; the entries then alternate, one window each per round, `--rounds` rounds; reported: the
median window, the fastest and the slowest.  The f32 operations the algorithm needs are computed from the shapes (the
N x N x D products: S once for the statistics, S again and C x Fn for the gradient = 6 N^2 D flop), so the rate is an
end-to-end rate of the call's four to six launches, not a kernel's share of peak.
Before timing, both entries' outputs at the shared shapes are compared (largest difference relative to the largest value).

    python tools/supcon_bench.py --dry-run                    # shapes, workspace bytes, flop; needs no device
    python tools/supcon_bench.py --out profiles/supcon_global.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHARED = [(B, D) for D in (128, 512) for B in (32, 64, 128, 256)]
TILED_ONLY = [(B, D) for D in (128, 512) for B in (512, 1024, 2048, 4096, 8192)]
T = 0.07


def flop(N, D):
    return 6.0 * N * N * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="calls per window at least")
    ap.add_argument("--window-ms", type=float, default=40.0, help="a window holds as many calls as fill about this long")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from hamspine import _lib as L
    lib = L.lib()
    if a.dry_run:
        for B, D in SHARED + TILED_ONLY:
            old = lib.hs_supcon_ws_bytes(B, D) if B <= 256 else None
            say(f"B={B:5d} D={D:4d}  flop {flop(B, D):.3e}  ws single {old}  ws tiled {lib.hs_supcon_tiled_ws_bytes(B, D)}  us/call not measured")
        return

    import torch
    import hamspine
    from hamspine import rt
    hamspine.require_device()
    say(f"# tools/supcon_bench.py --iters {a.iters} --window-ms {a.window_ms:g} --rounds {a.rounds}   device: {torch.cuda.get_device_name(0)}")
    say("# loss + d/d features, f32, temperature 0.07, labels uniform in 7 classes; us per call = one window of calls between")
    say("# device events / its calls; median [fastest .. slowest] over the rounds; the entries alternate inside a round")
    say("# single = hs_supcon_loss (one 256-thread workgroup), tiled = hs_supcon_tiled (normalise, statistics [merge], finish, gradient [project])")

    def make(B, D):
        g = torch.Generator().manual_seed(1000 + B + D)
        f = torch.randn(B, D, generator=g).cuda()
        y = torch.randint(0, 7, (B,), generator=g).cuda()
        loss = torch.empty(1, device="cuda")
        df = torch.empty(B, D, device="cuda")
        ws_old = torch.empty(max(lib.hs_supcon_ws_bytes(B, D), 16) // 4, device="cuda") if B <= 256 else None
        ws_new = torch.empty(lib.hs_supcon_tiled_ws_bytes(B, D) // 4, device="cuda")

        def single():
            L.check(lib.hs_supcon_loss(rt.p(f), rt.p(y), B, D, T, rt.p(loss), rt.p(df), rt.p(ws_old), rt.stream()), "hs_supcon_loss")

        def tiled():
            L.check(lib.hs_supcon_tiled(rt.p(f), rt.p(y), B, D, 0, B, T, 1.0, rt.p(loss), rt.p(df), rt.p(ws_new), rt.stream()),
                    "hs_supcon_tiled")

        return {"single": single, "tiled": tiled}, loss, df

    def window(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    def fmt(v):
        return f"{statistics.median(v):10.1f} [{min(v):9.1f} .. {max(v):9.1f}]"

    for shapes, entries in ((SHARED, ("single", "tiled")), (TILED_ONLY, ("tiled",))):
        say("")
        say(f"{'B':>6} {'D':>5}  " + "  ".join(f"{e + ' us/call':>36}" for e in entries) + "   tiled Gflop/s" +
            ("   single/tiled   max rel diff (loss, dfeat)" if len(entries) == 2 else ""))
        for B, D in shapes:
            fns, loss, df = make(B, D)
            got, iters = {}, {}
            for e in entries:                                              # warm-up, and the outputs for the comparison
                fns[e]()
                torch.cuda.synchronize()
                got[e] = (loss.clone(), df.clone())
                est = window(fns[e], 3)
                iters[e] = max(a.iters, min(5000, int(a.window_ms * 1e3 / est)))      # a window of about window_ms
            times = {e: [] for e in entries}
            for _ in range(a.rounds):
                for e in entries:
                    times[e].append(window(fns[e], iters[e]))
            med = statistics.median(times["tiled"])
            row = f"{B:6d} {D:5d}  " + "  ".join(f"{fmt(times[e]):>36}" for e in entries) + f"   {flop(B, D) / med / 1e3:13.1f}"
            if len(entries) == 2:
                dl = ((got["single"][0] - got["tiled"][0]).abs().max() / got["single"][0].abs().max()).item()
                dg = ((got["single"][1] - got["tiled"][1]).abs().max() / got["single"][1].abs().max()).item()
                row += f"   {statistics.median(times['single']) / med:12.2f}   {dl:.2e}, {dg:.2e}"
            say(row)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
