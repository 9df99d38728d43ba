"""Time per step of mamba_vision_T and mamba_vision_S (ConNexT/models/block/mamba_vision.py), forward + backward at batch 32,
224 pixels, bf16, and microseconds per call of the 3x3 convolution body of csrc/mvconv.hip (hs_conv3x3_fwd / hs_conv3x3_dgrad)
at the conv-stage shapes of the two variants:

    T: PatchEmbed 3 -> 32 -> 80 (stride 2 each), ConvBlocks at 80 x 56 x 56 and 160 x 28 x 28, Downsample 80 -> 160 -> 320
    S: PatchEmbed 3 -> 64 -> 96,                 ConvBlocks at 96 x 56 x 56 and 192 x 28 x 28, Downsample 96 -> 192 -> 384

The one comparison that means something for the body is the core it stands in for: at C = Kout = 128, 56 x 56, batch 32 both
hs_gemm's implicit-GEMM convolution and the 3x3 body accept the shape (the dispatch rule keeps hs_gemm there); the two are timed
alternately inside each repeat, forward and data gradient, stride 1 and 2.

Each row is timed with device events around --launches back-to-back calls (--steps for the models) after --warmup calls,
--repeats times; the table gives the median and the spread (min - max).

    python tools/mambavision_model_bench.py [--batch 32] [--launches 50] [--steps 10] [--warmup 5] [--repeats 5] [--skip-models]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd"))

# (name, C, Kout, H = W of the input, stride)
SHAPES = (("T PatchEmbed 3->32", 3, 32, 224, 2), ("T PatchEmbed 32->80", 32, 80, 112, 2), ("T ConvBlock 80", 80, 80, 56, 1),
          ("T Downsample 80->160", 80, 160, 56, 2), ("T ConvBlock 160", 160, 160, 28, 1), ("T Downsample 160->320", 160, 320, 28, 2),
          ("S PatchEmbed 3->64", 3, 64, 224, 2), ("S PatchEmbed 64->96", 64, 96, 112, 2), ("S ConvBlock 96", 96, 96, 56, 1),
          ("S Downsample 96->192", 96, 192, 56, 2), ("S ConvBlock 192", 192, 192, 28, 1), ("S Downsample 192->384", 192, 384, 28, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-models", action="store_true")
    a = ap.parse_args()

    import torch

    import hamspine
    from hamspine import _lib as L
    from hamspine import mambavision_conv_ops as cops
    from hamspine import raw, rt
    hamspine.require_device()
    hamspine.set_compute_dtype("bf16")
    lib = L.lib()
    dev, T = "cuda", torch.bfloat16

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

    def row(name, t, flops=None):
        rate = f"  {flops / t[0] * 1e-6:7.1f} TFLOP/s" if flops else ""
        print(f"{name:<58} {t[0]:>9.2f}  ({t[1]:.2f} - {t[2]:.2f}){rate}")

    def conv_fns(B, C, K, H, stride):
        """(new fwd, new dgrad, core fwd or None, core dgrad or None, flops)"""
        g = torch.Generator().manual_seed(0)
        Cp, Kp = cops.ceil8(C), cops.ceil8(K)
        P = (H - 1) // stride + 1
        x = torch.zeros(B, H, H, Cp, dtype=T, device=dev)
        x[..., :C] = torch.randn(B, H, H, C, generator=g).to(dev, T)
        dy = torch.zeros(B, P, P, Kp, dtype=T, device=dev)
        dy[..., :K] = torch.randn(B, P, P, K, generator=g).to(dev, T)
        w = (torch.randn(K, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(dev)
        wf, wt = torch.empty(K, 9 * Cp, dtype=T, device=dev), torch.empty(C, 9 * Kp, dtype=T, device=dev)
        L.check(lib.hs_conv3x3_pack_filter(rt.hs_dtype(T), rt.p(w), rt.p(wf), rt.p(wt), K, C, Cp, Kp, rt.stream()), "pack")
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        hdt, p, st = rt.hs_dtype(T), rt.p, rt.stream()

        def new_fwd():
            L.check(lib.hs_conv3x3_fwd(hdt, p(x), p(wf), None, p(y), B, H, H, C, Cp, K, Kp, stride, st), "hs_conv3x3_fwd")

        def new_dgrad():
            L.check(lib.hs_conv3x3_dgrad(hdt, p(dy), p(wt), p(dx), B, H, H, C, Cp, K, Kp, stride, st), "hs_conv3x3_dgrad")
        core_fwd = core_dgrad = None
        if cops.uses_gemm_core(C, K):
            geom = raw.conv_geom(B, H, H, C, K, 3, 3, stride, 1)

            def core_fwd():
                raw.gemm(x, wf, y, B * P * P, K, 9 * C, a_kind=L.A_CONV, b_kind=L.B_KC, ldb=9 * C, ldd=K, geom=geom)

            def core_dgrad():
                raw.gemm(dy, wf, dx, B * H * H, C, 9 * K, a_kind=L.A_DGRAD, b_kind=L.B_WDGRAD, ldd=C, geom=geom)
        return new_fwd, new_dgrad, core_fwd, core_dgrad, 2.0 * B * P * P * K * 9 * C

    print(f"{a.launches} launches ({a.steps} model steps) x {a.repeats} repeats after {a.warmup} warm-up calls; bf16, batch {a.batch}")
    print("-- 3x3 body (csrc/mvconv.hip): us per call, median (min - max), algorithmic rate")
    for name, C, K, H, stride in SHAPES:
        f, d, _, _, fl = conv_fns(a.batch, C, K, H, stride)
        t = timed_many([f, d], a.launches)
        row(f"{name} {H}x{H} s{stride} fwd", t[0], fl)
        row(f"{name} {H}x{H} s{stride} dgrad", t[1], fl)
    print("-- 3x3 body against hs_gemm's core at C = Kout = 128, 56 x 56: us per call")
    for stride in (1, 2):
        f, d, cf, cd, fl = conv_fns(a.batch, 128, 128, 56, stride)
        t = timed_many([f, cf, d, cd], a.launches)
        row(f"128->128 s{stride} fwd   3x3 body", t[0], fl)
        row(f"128->128 s{stride} fwd   hs_gemm core", t[1], fl)
        row(f"128->128 s{stride} dgrad 3x3 body", t[2], fl)
        row(f"128->128 s{stride} dgrad hs_gemm core", t[3], fl)
    if a.skip_models:
        return
    import ConNexT.models.block.mamba_vision as mv
    print("-- models: us per step, median (min - max)")
    for name in ("mamba_vision_T", "mamba_vision_S"):
        torch.manual_seed(0)
        m = getattr(mv, name)().to(dev).train()
        x = torch.randn(a.batch, 3, 224, 224, device=dev)
        go = torch.randn(a.batch, 1000, device=dev)

        def fwd():
            with torch.no_grad():
                m(x)

        def fwd_bwd():
            m(x).backward(go)
            for q in m.parameters():
                q.grad = None
        t = timed_many([fwd, fwd_bwd], a.steps)
        row(f"{name} bf16 B {a.batch} 224 px fwd (train mode)", t[0])
        row(f"{name} bf16 B {a.batch} 224 px fwd+bwd", t[1])
        del m


if __name__ == "__main__":
    main()
