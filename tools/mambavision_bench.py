"""Microseconds per call of the MambaVision kernels (csrc/ssm.hip: centred conv1d + SiLU, the 8-state gate-less scan) and of the
hybrid stage (ConNexT/models/block/mamba_vision.py: MambaVisionLayer) at the MambaVision-T sizes, batch 32:

    stage 3: dim 320, 14 x 14 map, window 14, depth 8 (blocks 4-7 attention, 8 heads)  ->  32 windows of 196 tokens, d = 160
    stage 4: dim 640,  7 x  7 map, window  7, depth 4 (blocks 2-3 attention, 16 heads) ->  32 windows of  49 tokens, d = 320

Each row is timed with device events around --launches back-to-back calls (--steps for the stage) after --warmup calls,
--repeats times; the table gives the median and the spread (min - max).  "fwd+bwd" runs the forward and the backward entry
points one after the other; the backward of the conv and of the scan is two launches (kernel + ordered reduce).

The one comparison that means something for the scan is the path this kernel replaces: the existing 16-lane gated kernel
(d_state 16) on the same (B, L, d), with the upper 8 states' Bm / Cm zero and z = 1.2785 (silu(z) = 1, an inert gate).  The two
are timed alternately inside each repeat.

    python tools/mambavision_bench.py [--dtype both|bf16|f32] [--batch 32] [--launches 200] [--steps 30] [--warmup 20] [--repeats 5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd"))

STAGES = (dict(dim=320, side=14, window=14, depth=8, heads=8), dict(dim=640, side=7, window=7, depth=4, heads=16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="both", choices=("both", "bf16", "f32"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()

    import torch

    import hamspine
    from hamspine import _lib as L
    from hamspine import rt
    hamspine.require_device()
    lib = L.lib()
    dev = "cuda"

    def timed_many(fns, count):
        """the functions alternate inside each repeat -> [(median, min, max)] in microseconds per call"""
        for fn in fns:
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        res = [[] for _ in fns]
        for _ in range(a.repeats):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(count):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                res[i].append(e0.elapsed_time(e1) * 1e3 / count)
        return [(sorted(r)[len(r) // 2], min(r), max(r)) for r in res]

    def row(name, t):
        print(f"{name:<58} {t[0]:>9.2f}  ({t[1]:.2f} - {t[2]:.2f})")

    def kernels(mode, B, Lt, d):
        from ConNexT.models.block.mamba_vision import MambaVisionMixer
        from hamspine.nn import Mamba
        T = torch.bfloat16 if mode == "bf16" else torch.float32
        hdt, esz = rt.hs_dtype(T), (2 if mode == "bf16" else 4)
        g = torch.Generator().manual_seed(0)

        def rnd(*shape, scale=1.0):
            return (scale * torch.randn(*shape, generator=g)).to(dev, T)
        torch.manual_seed(0)
        mix = MambaVisionMixer(2 * d, d_state=8, d_conv=3, expand=1).to(dev)
        wide = Mamba(d // 2, d_state=16).to(dev)                      # d_inner = d: its A_log (d, 16)
        xz, u, dt, dout = rnd(B, Lt, 2 * d), rnd(B, Lt, d), rnd(B, Lt, d, scale=0.5), rnd(B, Lt, 2 * d)
        bc8 = rnd(B, Lt, 16)
        bc16 = torch.zeros(B, Lt, 32, device=dev, dtype=T)
        bc16[..., :8], bc16[..., 16:24] = bc8[..., :8], bc8[..., 8:]
        z = torch.full((B, Lt, d), 1.2785, device=dev, dtype=T)
        cw = mix.conv1d_x.weight.detach()
        A8, D, dtb, A16 = mix.A_log.detach(), mix.D.detach(), mix.dt_proj.bias.detach(), wide.A_log.detach()
        yz = torch.empty(B, Lt, 2 * d, device=dev, dtype=T)
        nck = (Lt - 1) // 16
        hck8 = torch.empty(B, max(nck, 1), d, 8, device=dev)
        hck16 = torch.empty(B, max(nck, 1), d, 16, device=dev)
        du, ddt, dz, dxs = (torch.empty(B, Lt, d, device=dev, dtype=T) for _ in range(4))
        dbc = torch.empty(B, Lt, 32, device=dev, dtype=T)
        dA8, dA16, dD, ddtb, dcw = (torch.empty_like(t) for t in (A8, A16, D, dtb, cw))
        ws = torch.empty(max(lib.hs_selective_scan_ws_bytes_nogate(B, Lt, d, 8), lib.hs_selective_scan_ws_bytes_n(B, Lt, d, 16),
                             lib.hs_conv1d_same_silu_ws_bytes(B, d)), dtype=torch.uint8, device=dev)
        p, st = rt.p, rt.stream()

        # as in the mixer: the z half of the in_proj output is read in place, the result lands in the right half of yz
        def conv_fwd():
            L.check(lib.hs_conv1d_same_silu_fwd(hdt, p(xz, d * esz), 2 * d, p(cw), None, p(yz, d * esz), 2 * d, B, Lt, d, 3, st), "conv")

        def conv_bwd():
            L.check(lib.hs_conv1d_same_silu_bwd(hdt, p(dout, d * esz), 2 * d, p(xz, d * esz), 2 * d, p(cw), None, p(dxs), d, p(dcw),
                                                None, p(ws), ws.numel(), B, Lt, d, 3, st), "conv bwd")

        def scan8_fwd():
            L.check(lib.hs_selective_scan_fwd(hdt, p(u), d, p(dt), d, p(dtb), p(A8), p(bc8), p(bc8, 8 * esz), 16, p(D), None, 0, p(yz),
                                              2 * d, p(hck8), B, Lt, d, 8, st), "scan 8")

        def scan8_bwd():
            L.check(lib.hs_selective_scan_bwd(hdt, p(dout), 2 * d, p(u), d, p(dt), d, p(dtb), p(A8), p(bc8), p(bc8, 8 * esz), 16, p(D),
                                              None, 0, p(hck8), p(du), d, p(ddt), d, p(dbc), p(dbc, 8 * esz), 16, None, 0, p(dA8), p(dD),
                                              p(ddtb), p(ws), ws.numel(), B, Lt, d, 8, st), "scan 8 bwd")

        def scan16_fwd():
            L.check(lib.hs_selective_scan_fwd(hdt, p(u), d, p(dt), d, p(dtb), p(A16), p(bc16), p(bc16, 16 * esz), 32, p(D), p(z), d,
                                              p(yz), 2 * d, p(hck16), B, Lt, d, 16, st), "scan 16")

        def scan16_bwd():
            L.check(lib.hs_selective_scan_bwd(hdt, p(dout), 2 * d, p(u), d, p(dt), d, p(dtb), p(A16), p(bc16), p(bc16, 16 * esz), 32,
                                              p(D), p(z), d, p(hck16), p(du), d, p(ddt), d, p(dbc), p(dbc, 16 * esz), 32, p(dz), d,
                                              p(dA16), p(dD), p(ddtb), p(ws), ws.numel(), B, Lt, d, 16, st), "scan 16 bwd")

        def both(f, b):
            def fn():
                f()
                b()
            return fn
        print(f"-- kernels, {mode}, B {B} L {Lt} d {d}: us per call, median (min - max)")
        t = timed_many([conv_fwd, both(conv_fwd, conv_bwd)], a.launches)
        row("hs_conv1d_same_silu fwd", t[0])
        row("hs_conv1d_same_silu fwd+bwd", t[1])
        t = timed_many([scan8_fwd, scan16_fwd, both(scan8_fwd, scan8_bwd), both(scan16_fwd, scan16_bwd)], a.launches)
        row("hs_selective_scan N 8 gate-less fwd", t[0])
        row("hs_selective_scan N 16 gated, 8 states zero, fwd", t[1])
        row("hs_selective_scan N 8 gate-less fwd+bwd", t[2])
        row("hs_selective_scan N 16 gated, 8 states zero, fwd+bwd", t[3])

    def stage(mode, B, cfg):
        from ConNexT.models.block.mamba_vision import MambaVisionLayer
        hamspine.set_compute_dtype(mode)
        torch.manual_seed(0)
        depth = cfg["depth"]
        m = MambaVisionLayer(dim=cfg["dim"], depth=depth, num_heads=cfg["heads"], window_size=cfg["window"], conv=False,
                             downsample=False, transformer_blocks=list(range(depth // 2, depth)), layer_scale=1e-5).to(dev).train()
        g = torch.Generator().manual_seed(1)
        x = torch.randn(B, cfg["dim"], cfg["side"], cfg["side"], generator=g).to(dev).requires_grad_(True)
        go = torch.randn(B, cfg["dim"], cfg["side"], cfg["side"], generator=g).to(dev)

        def fwd():
            with torch.no_grad():
                m(x)

        def fwd_bwd():
            m(x).backward(go)
            for q in m.parameters():
                q.grad = None
            x.grad = None
        t = timed_many([fwd, fwd_bwd], a.steps)
        name = f"MambaVisionLayer({cfg['dim']}, depth {depth}, window {cfg['window']}) {mode} B {B}"
        row(name + " fwd", t[0])
        row(name + " fwd+bwd", t[1])

    modes = ("bf16", "f32") if a.dtype == "both" else (a.dtype,)
    print(f"{a.launches} launches ({a.steps} stage steps) x {a.repeats} repeats after {a.warmup} warm-up calls")
    for mode in modes:
        for cfg in STAGES:
            kernels(mode, a.batch, cfg["window"] ** 2, cfg["dim"] // 2)
    print("-- stage: us per step, median (min - max)")
    for mode in modes:
        for cfg in STAGES:
            stage(mode, a.batch, cfg)
    hamspine.set_compute_dtype("bf16")


if __name__ == "__main__":
    main()
