"""Microseconds per launch of the Mamba kernels (csrc/ssm.hip) and of the whole SSMFusionModule, at the shape of the
reference's configs/ham/ham_fusion_ssm_v1.yml: B 64, L 49 image tokens, hidden 256 (d_inner 512, dt_rank 16).

Each C entry point is timed on its own with device events around --launches back-to-back launches, after --warmup
launches, --repeats times; the table gives the median and the spread.  "bytes" counts every operand once in and every
result once out (workspaces and recomputation not counted); "HBM %" is bytes / time over the 8.0 TB/s peak.  The module
rows time forward, and forward + backward, of SSMFusionModule(768, 256) with 32 text tokens (d_state 16 only).

--d-state N times the kernels at another state size (16, 32, 64, 128, 256); --batch 16 --tokens 52 --d-state 128 is the shape
of the multimodal Mamba blocks (reference ConNexT/models/block/len4mamba.py).  --len4mamba adds forward + backward of
MultimodalMambaWithKANAttention with the reference's defaults (768 / 640 / 3584 / 256, 4 heads, 49 image tokens) at --batch, and
the number of kernel launches of one such step as the profiler counts them.

    python tools/ssm_bench.py [--dtype bf16|f32] [--d-state 16] [--len4mamba] [--launches 200] [--warmup 20] [--repeats 5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd"))

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "f32"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=49)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--d-state", type=int, default=16)
    ap.add_argument("--len4mamba", action="store_true")
    a = ap.parse_args()

    import torch

    import hamspine
    from hamspine import _lib as L
    from hamspine import rt
    hamspine.require_device()
    hamspine.set_compute_dtype(a.dtype)
    lib = L.lib()
    T = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    hdt = rt.hs_dtype(T)
    esz = 2 if a.dtype == "bf16" else 4
    B, Lt, H = a.batch, a.tokens, a.hidden
    d, N = 2 * H, a.d_state
    rows = B * Lt
    dev = "cuda"
    g = torch.Generator().manual_seed(0)

    def rnd(*shape, scale=1.0):
        return (scale * torch.randn(*shape, generator=g)).to(dev, T)
    from hamspine.nn import Mamba
    blk = Mamba(H, d_state=N).to(dev)
    xz, u, dt, bc, dout = rnd(B, Lt, 2 * d), rnd(B, Lt, d), rnd(B, Lt, d, scale=0.5), rnd(B, Lt, 2 * N), rnd(B, Lt, d)
    cw, cb = blk.conv1d.weight.detach(), blk.conv1d.bias.detach()
    A_log, D, dtb = blk.A_log.detach(), blk.D.detach(), blk.dt_proj.bias.detach()
    y = torch.empty(B, Lt, d, device=dev, dtype=T)
    out = torch.empty_like(y)
    nck = (Lt - 1) // lib.hs_selective_scan_chunk_len_n(N)
    hck = torch.empty(B, max(nck, 1), d, N, device=dev)
    du, ddt, dz, dxs = (torch.empty_like(y) for _ in range(4))
    dbc = torch.empty(B, Lt, 2 * N, device=dev, dtype=T)
    dA, dD, ddtb, dcw, dcb = (torch.empty_like(t) for t in (A_log, D, dtb, cw, cb))
    ws = torch.empty(max(lib.hs_selective_scan_ws_bytes_n(B, Lt, d, N), lib.hs_causal_conv1d_ws_bytes(B, d)), dtype=torch.uint8,
                     device=dev)
    p, st = rt.p, rt.stream()
    z_off = d * esz

    def conv_fwd():
        L.check(lib.hs_causal_conv1d_fwd(hdt, p(xz), 2 * d, p(cw), p(cb), p(y), d, B, Lt, d, 4, st), "conv fwd")

    def conv_bwd():
        L.check(lib.hs_causal_conv1d_bwd(hdt, p(dout), d, p(xz), 2 * d, p(cw), p(cb), p(dxs), d, p(dcw), p(dcb), p(ws), ws.numel(),
                                         B, Lt, d, 4, st), "conv bwd")

    def scan_fwd():
        L.check(lib.hs_selective_scan_fwd(hdt, p(u), d, p(dt), d, p(dtb), p(A_log), p(bc), p(bc, N * esz), 2 * N, p(D),
                                          p(xz, z_off), 2 * d, p(out), d, p(hck), B, Lt, d, N, st), "scan fwd")

    def scan_bwd():
        L.check(lib.hs_selective_scan_bwd(hdt, p(dout), d, p(u), d, p(dt), d, p(dtb), p(A_log), p(bc), p(bc, N * esz), 2 * N,
                                          p(D), p(xz, z_off), 2 * d, p(hck), p(du), d, p(ddt), d, p(dbc), p(dbc, N * esz), 2 * N,
                                          p(dz), d, p(dA), p(dD), p(ddtb), p(ws), ws.numel(), B, Lt, d, N, st), "scan bwd")

    act = rows * d * esz                 # one (B, L, d) activation
    small = rows * 2 * N * esz           # Bm | Cm
    par = (d * N + 2 * d) * 4
    cases = [
        ("hs_causal_conv1d_fwd", conv_fwd, 2 * act + 5 * d * 4),
        ("hs_causal_conv1d_bwd (2 launches)", conv_bwd, 3 * act + 10 * d * 4),
        ("hs_selective_scan_fwd", scan_fwd, 4 * act + small + par + B * nck * d * N * 4),
        ("hs_selective_scan_bwd (2 launches)", scan_bwd, 7 * act + 2 * small + 2 * par + B * nck * d * N * 4),
    ]

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        res = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        res.sort()
        return res[len(res) // 2], res[0], res[-1]

    print(f"shape B {B} L {Lt} hidden {H} (d_inner {d}, d_state {N}), {a.dtype}; {a.launches} launches x {a.repeats} repeats "
          f"after {a.warmup} warm-up")
    print(f"{'entry point':<36} {'us/call':>9} {'min':>8} {'max':>8} {'bytes':>12} {'GB/s':>8} {'HBM %':>6}")
    for name, fn, nbytes in cases:
        med, lo, hi = timed(fn)
        bw = nbytes / (med * 1e-6)
        print(f"{name:<36} {med:>9.2f} {lo:>8.2f} {hi:>8.2f} {nbytes:>12d} {bw / 1e9:>8.1f} {100 * bw / HBM_PEAK:>6.2f}")

    def module_rows(title, m, leaves, grad_out):
        def fwd():
            with torch.no_grad():
                m(*leaves)

        def fwd_bwd():
            m(*leaves).backward(grad_out)
            for q in m.parameters():
                q.grad = None
            for t in leaves:
                t.grad = None
        for name, fn in ((title + " forward (no_grad)", fwd), (title + " forward + backward", fwd_bwd)):
            med, lo, hi = timed(fn)
            print(f"{name:<36} {med:>9.2f} {lo:>8.2f} {hi:>8.2f}")
        return fwd_bwd

    if N == 16:
        from modules.fusion_blocks import SSMFusionModule
        torch.manual_seed(0)
        m = SSMFusionModule(768, H).to(dev).train()
        module_rows("SSMFusionModule", m, [rnd(B, Lt, H).requires_grad_(True), rnd(B, 32, 768).requires_grad_(True)],
                    torch.randn(B, H, generator=g).to(dev))

    if a.len4mamba:
        from torch.profiler import ProfilerActivity, profile

        from ConNexT.models.block.len4mamba import MultimodalMambaWithKANAttention
        torch.manual_seed(0)
        m = MultimodalMambaWithKANAttention().to(dev).train()
        leaves = [torch.randn(*shape, generator=g).to(dev).requires_grad_(True)
                  for shape in ((B, 768), (B, 640, 49), (B, 3584), (B, 3584))]
        step = module_rows("MultimodalMambaWithKANAttention", m, leaves, torch.randn(B, 52, 256, generator=g).to(dev))
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        print(f"MultimodalMambaWithKANAttention forward + backward at B {B}: {len(kernels)} device launches "
              f"(kernels and copies), {sum(e.device_time for e in kernels):.1f} us of device time")


if __name__ == "__main__":
    main()
