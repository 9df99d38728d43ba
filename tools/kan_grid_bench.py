#!/usr/bin/env python
"""KAN grid update: the host route (KANLinear._update_grid_host: device -> host copies, the (batch, in, out) tensor, torch.sort
and a batched LAPACK lstsq on the CPU, copies back) against the device route (hamspine.kan.kan_update_grid: csrc/kan_grid.hip),
alternating in ONE process on the same modules, for

    experts    KAN1([1536, 512, 128, 32, 7]) at 64 rows: forward(update_grid=True), i.e. four updates and four forwards
    attention  one KANLinear(768, 768) at 3328 rows (64 samples x the 52 tokens of the KAN attention): one update

One call = the parameters restored to their saved state (untimed), then the update(s), timed with a host clock around work that
ends in a device synchronise -- the host route's time is mostly host time, so device events alone would miss it.  After one
warm-up call per route the routes alternate, `--reps` calls each per round, `--rounds` rounds.  Reported per route: the median
over all timed calls, the per-round medians and their spread, and the growth of torch.cuda.max_memory_allocated() over the
call (on either route that is the forward's packed weight matrix) and, from an untimed call, over one layer's update alone.
The host route's host memory is computed from the shapes (the (batch, in, out) tensor and the copies lstsq makes of it);
a case whose estimate exceeds the free host memory is reported as "not run", never shortened.

    python tools/kan_grid_bench.py --dry-run                 # shapes, bytes and launches per case; needs no device
    python tools/kan_grid_bench.py --reps 5 --rounds 3
    python tools/kan_grid_bench.py --case experts --only device --reps 20 --rounds 1      # a profiler run
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = {"experts": dict(widths=[1536, 512, 128, 32, 7], rows=64), "attention": dict(widths=[768, 768], rows=3328)}
GRID_SIZE, ORDER = 5, 3


def shape_counts(widths, rows):
    """from the shapes alone, summed over the layers: what each route allocates and launches"""
    nb, nk = GRID_SIZE + ORDER, GRID_SIZE + 2 * ORDER + 1
    chunks = -(-rows // 256)
    pairs = list(zip(widths, widths[1:]))
    return dict(
        layers=len(pairs), rows=rows,
        host_materialised_bytes_largest_layer=max(rows * i * o * 4 for i, o in pairs),
        # y, its transposed copy handed to lstsq, and the solver's own working copy of the right-hand sides
        host_route_host_bytes_estimate=3 * max(rows * i * o * 4 for i, o in pairs),
        host_route_copy_bytes=sum((rows * i + i * nk + o * i * nb) * 4 * 2 for i, o in pairs),
        device_workspace_bytes_largest_layer=max(chunks * i * nb * 2 * nb * 8 for i, o in pairs),
        device_new_grid_bytes_largest_layer=max(i * nk * 4 for i, o in pairs),
        device_launches_per_update=4,                     # knots, accumulate, solve, grid copy
        device_f64_fma_per_update=sum(rows * i * 2 * nb * nb + i * o * nb * nb for i, o in pairs))


def free_host_bytes():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    except OSError:
        pass
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="", choices=("", *CASES))
    ap.add_argument("--only", default="", choices=("", "host", "device"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    cases = [a.case] if a.case else list(CASES)
    if a.dry_run:
        print(json.dumps({c: dict(shape_counts(**CASES[c]), ms_per_call="not measured") for c in cases}))
        return

    import torch
    import hamspine
    from ConNexT.models.block import kan1

    hamspine.require_device()
    out = dict(reps=a.reps, rounds=a.rounds, grid_size=GRID_SIZE, spline_order=ORDER, device=torch.cuda.get_device_name(0))
    for case in cases:
        widths, rows = CASES[case]["widths"], CASES[case]["rows"]
        torch.manual_seed(0)
        net = kan1.KAN1(widths, grid_size=GRID_SIZE, spline_order=ORDER).cuda()
        x0 = (torch.randn(rows, widths[0]) * 0.9).cuda()
        saved = {k: v.detach().clone() for k, v in net.state_dict().items()}
        counts = shape_counts(widths, rows)
        res = dict(counts)

        def call(route):
            with torch.no_grad():
                x = x0
                for n, layer in enumerate(net.layers):
                    (layer._update_grid_host if route == "host" else layer.update_grid)(x)
                    if n + 1 < len(net.layers):
                        x = layer(x)

        def timed(route):
            net.load_state_dict(saved)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            call(route)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() - base

        def update_peak(route):
            """largest growth of the device allocation over one layer's update alone (untimed; the whole call's peak is the
            forward's packed weight matrix on either route)"""
            net.load_state_dict(saved)
            worst = 0
            with torch.no_grad():
                x = x0
                for n, layer in enumerate(net.layers):
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    (layer._update_grid_host if route == "host" else layer.update_grid)(x)
                    torch.cuda.synchronize()
                    worst = max(worst, torch.cuda.max_memory_allocated() - base)
                    if n + 1 < len(net.layers):
                        x = layer(x)
            return worst

        routes = [a.only] if a.only else ["host", "device"]
        free = free_host_bytes()
        if "host" in routes and free is not None and counts["host_route_host_bytes_estimate"] > 0.5 * free:
            routes.remove("host")
            res["host"] = f"not run: needs about {counts['host_route_host_bytes_estimate']} bytes of host memory, {free} free"
        for r in routes:
            timed(r)                                          # warm-up: code objects, allocator pools, LAPACK threads
        times = {r: [] for r in routes}
        peaks = {r: 0 for r in routes}
        for _ in range(a.rounds):
            for r in routes:                                  # alternating in the same process
                got = [timed(r) for _ in range(a.reps)]
                times[r].append([t for t, _ in got])
                peaks[r] = max(peaks[r], max(p for _, p in got))
        for r in routes:
            meds = [statistics.median(v) for v in times[r]]
            res[r] = dict(median_ms=statistics.median([t for v in times[r] for t in v]), round_medians_ms=[round(m, 3) for m in meds],
                          min_ms=min(meds), max_ms=max(meds), peak_device_bytes=peaks[r], update_peak_device_bytes=update_peak(r))
        if len(routes) == 2:
            res["host_over_device"] = res["host"]["median_ms"] / res["device"]["median_ms"]
        out[case] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
