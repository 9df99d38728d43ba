"""The convolutional half of MambaVision and the whole model (reference ConNexT/models/block/mamba_vision.py) on the GPU: the 3x3
convolution body, the BatchNorm epilogues, the NHWC window partition / reverse and the drop-in modules against
tests/mambavision_model_ref.py in float64, and the small model against the fixture recorded from the reference.

Gates (those of tests/test_mambavision_gpu.py).  f32 mode: outputs <= 1e-4 * max|ref| and every gradient <= 1e-3 in relative L2
norm.  bf16 mode: the yardstick itself is run on the CPU with bfloat16 activations under the module's dtype policy; the GPU may
show at most twice its error against float64, with the f32 round-off floor F32_NOISE.  The window kernels are permutations and
are compared bitwise.

A bias in front of a train-mode BatchNorm (ConvBlock's conv1.bias and conv2.bias) has the gradient zero in exact arithmetic: the
reference holds round-off only, so a relative error says nothing there.  Those gradients are bounded against the gradient of
the same convolution's weight instead (ZERO_F32 / ZERO_BF16 below); the eval-mode ConvBlock tests, where the biases have a real
gradient, put them under the ordinary gates.  The same holds in the whole model for the last block's mlp.fc2.bias (LAST_BIAS):
it shifts every kept token of a channel alike, and the train-mode final BatchNorm removes that shift."""
import copy
import os

import numpy as np
import pytest
import torch

import mambavision_model_ref as mm
import mambavision_ref as mr

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from hamspine import mambavision_conv_ops as cops  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mambavision_model.npz")
F32_NOISE = 1e-6
# |d bias| / |d weight| of a convolution whose bias gradient cancels exactly.  The bias gradient is the sum over the M pixels of
# dy, the weight gradient sums dy * x with |x| = O(1): f32 leaves eps_f32 * sqrt(M) of the terms' norm, well inside 1e-3.  In
# bf16 dy is rounded to 2^-9 relative before the sum, so up to 2^-9 * sqrt(M) * |dy| / (|dy| * rms(x) * sqrt(M)) ~ 2^-9 / rms(x)
# remains; 2^-6 leaves a factor 8 for rms(x) < 1 after the GELU.
ZERO_F32, ZERO_BF16 = 1e-3, 2.0 ** -6
LAST_BIAS = "levels.3.blocks.1.mlp.fc2.bias"
SMALL_KW = dict(dim=8, in_dim=8, depths=[1, 2, 2, 2], num_heads=[1, 1, 2, 2], window_size=[8, 8, 4, 2], mlp_ratio=2,
                drop_path_rate=0., num_classes=5, layer_scale=0.5, layer_scale_conv=0.5)


@pytest.fixture
def f32_mode():
    hamspine.set_compute_dtype("f32")
    yield
    hamspine.set_compute_dtype("bf16")


def _rel(got, ref):
    ref = ref.double()
    return ((got.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def _maxrel(got, ref):
    ref = ref.double()
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _is_zero_grad(k, train):
    return train and (k.endswith(("conv1.bias", "conv2.bias")) or k == LAST_BIAS)


def _weight_of(k):
    return k[:-4] + "weight"


def _assert_f32(what, outs, g, ref_outs, ref_g, train=True):
    errs = {k: _maxrel(outs[k], ref_outs[k]) for k in ref_outs}
    print(f"{what} f32:", {k: f"{v:.2e}" for k, v in errs.items()},
          {k: f"{_rel(g[k], ref_g[k]):.2e}" if g.get(k) is not None else "missing" for k in ref_g})
    assert all(v <= 1e-4 for v in errs.values()), errs
    for k in ref_g:
        assert g.get(k) is not None, k
        if _is_zero_grad(k, train):
            assert g[k].double().norm().item() <= ZERO_F32 * ref_g[_weight_of(k)].norm().item(), k
        else:
            assert _rel(g[k], ref_g[k]) <= 1e-3, k


def _assert_bf16(what, outs, g, cpu_outs, cpu_g, ref_outs, ref_g, train=True):
    o = {k: (_maxrel(outs[k], ref_outs[k]), _maxrel(cpu_outs[k], ref_outs[k])) for k in ref_outs}
    rows = {k: (_rel(g[k], ref_g[k]) if g.get(k) is not None else None, _rel(cpu_g[k], ref_g[k])) for k in ref_g}
    print(f"{what} bf16 against float64 (GPU, CPU bf16 yardstick):", {k: f"{a:.2e} {b:.2e}" for k, (a, b) in o.items()},
          {k: f"{a:.2e} {b:.2e}" if a is not None else "missing" for k, (a, b) in rows.items()})
    for k, (a, b) in o.items():
        assert a <= max(2 * b, F32_NOISE), k
    for k, (a, b) in rows.items():
        assert a is not None, k
        if _is_zero_grad(k, train):
            assert g[k].double().norm().item() <= ZERO_BF16 * ref_g[_weight_of(k)].norm().item(), k
        else:
            assert a <= max(2 * b, F32_NOISE), k


def _ref_run(fn, params, x, w, bf16=False):
    """the yardstick on the CPU: float64 throughout, or (bf16) f32 leaves with bfloat16 activations.  fn(x, params) -> output or
    dict of outputs whose first entry takes the cotangent w"""
    keep = torch.float32 if bf16 else torch.float64
    leaves = {k: v.detach().cpu().to(keep).requires_grad_(True) if v.is_floating_point() and "running_" not in k
              else v.detach().cpu().to(keep) for k, v in params.items() if v.is_floating_point()}
    xin = x.detach().clone().to(keep).requires_grad_(True)
    outs = fn(xin.to(BF16) if bf16 else xin, leaves)
    outs = outs if isinstance(outs, dict) else {"out": outs}
    first = next(iter(outs.values()))
    (first.to(keep) * w.to(keep)).sum().backward()
    grads = {k: v.grad for k, v in leaves.items() if v.requires_grad}
    grads["x"] = xin.grad
    return {k: v.detach() for k, v in outs.items()}, grads


def _mode_dtype(mode):
    return torch.float32 if mode == "f32" else BF16


# ------------------------------------------------------------------------------------------------ the 3x3 convolution
CONV_CASES = [(1, 1, 1, 8, 8, 1), (2, 5, 6, 8, 16, 2), (2, 7, 7, 80, 80, 1), (3, 9, 9, 24, 40, 1), (2, 6, 5, 80, 160, 2),
              (2, 4, 4, 196, 392, 2)]
_conv_cache = {}


def _conv_case(case, bias):
    key = (case, bias)
    if key not in _conv_cache:
        N, H, W, C, K, stride = case
        g = torch.Generator().manual_seed(hash(case) % 1000 + bias)
        x = torch.randn(N, C, H, W, generator=g)
        params = {"weight": torch.randn(K, C, 3, 3, generator=g) / (3 * C ** 0.5)}
        if bias:
            params["bias"] = torch.randn(K, generator=g)
        w = torch.randn(N, K, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=g)
        fn = lambda t, p: mm.conv3x3_ref(t, p["weight"], p.get("bias"), stride)
        _conv_cache[key] = (x, params, w, _ref_run(fn, params, x, w), _ref_run(fn, params, x, w, bf16=True))
    return _conv_cache[key]


def _conv_gpu(x, params, w, stride, dtype, force_new=False):
    p = {k: v.to(DEV).requires_grad_(True) for k, v in params.items()}
    xin = x.to(DEV, dtype).requires_grad_(True)
    out = cops.conv3x3(xin, p["weight"], p.get("bias"), stride, force_new_body=force_new)
    assert out.dtype == dtype and tuple(out.shape) == tuple(w.shape)
    (out.float() * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in p.items()}
    grads["x"] = xin.grad
    return out.detach(), grads


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_conv3x3_forward_data_weight_and_bias_gradients(mode, case, bias):
    x, params, w, (ref, ref_g), (cpu, cpu_g) = _conv_case(case, bias)
    C, K = case[3], case[4]
    assert not cops.uses_gemm_core(C, K)
    out, g = _conv_gpu(x, params, w, case[5], _mode_dtype(mode))
    what = f"conv3x3 {case} bias {bias}"
    if mode == "f32":
        _assert_f32(what, {"out": out}, g, ref, ref_g)
    else:
        _assert_bf16(what, {"out": out}, g, cpu, cpu_g, ref, ref_g)
    for t, ch in ((out, K), (g["x"], C)):            # the pad lanes of what the kernels wrote are zero
        rows = cops._rows(t)
        assert rows.shape[-1] == cops.ceil8(ch) and not rows[..., ch:].any()
    assert tuple(g["weight"].shape) == (K, C, 3, 3) and g["weight"].dtype == torch.float32


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_padded_output_pitch_has_zero_pad_lanes(mode):
    """196 output channels are stored with pitch 200: lanes 196 .. 199 of every pixel are written as zeros, with a bias too"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 196, 4, 4, generator=g).to(DEV, _mode_dtype(mode))
    w, b = (torch.randn(196, 196, 3, 3, generator=g) / 42).to(DEV), torch.randn(196, generator=g).to(DEV)
    y = cops.conv3x3(x, w, b, 1)
    rows = cops._rows(y)
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (2, 4, 4, 200) and rows.data_ptr() == y.data_ptr() and not rows[..., 196:].any()
    ref = torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), b.double().cpu(), 1, 1)
    assert _maxrel(y, ref) <= (1e-4 if mode == "f32" else 2e-2)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_dispatch_keeps_the_gemm_core_where_it_fits_and_both_bodies_agree(mode, stride):
    case = (2, 6, 6, 128, 128, stride)
    assert cops.uses_gemm_core(128, 128)
    x, params, w, (ref, ref_g), (cpu, cpu_g) = _conv_case(case, True)
    for force_new in (False, True):
        out, g = _conv_gpu(x, params, w, stride, _mode_dtype(mode), force_new)
        what = f"conv3x3 {case} {'3x3 body' if force_new else 'hs_gemm core'}"
        if mode == "f32":
            _assert_f32(what, {"out": out}, g, ref, ref_g)
        else:
            _assert_bf16(what, {"out": out}, g, cpu, cpu_g, ref, ref_g)


# ------------------------------------------------------------------------------------------------ BatchNorm epilogues
def _bn_params(C, seed):
    g = torch.Generator().manual_seed(seed)
    return {"bn.weight": 1 + 0.3 * torch.randn(C, generator=g), "bn.bias": 0.3 * torch.randn(C, generator=g),
            "bn.running_mean": 0.2 * torch.randn(C, generator=g), "bn.running_var": 1 + 0.3 * torch.rand(C, generator=g)}


def _bn_holder(params, C, eps):
    bn = torch.nn.BatchNorm2d(C, eps=eps)
    bn.load_state_dict({k[3:]: v for k, v in params.items()}, strict=False)
    return bn.to(DEV)


BN_CASES = {"gelu_98x80": (0, (2, 80, 7, 7), False, False), "gelu_3x8": (0, (3, 8, 1, 1), False, False),
            "residual_196_ls_rowscale": (1, (2, 196, 3, 3), True, True), "residual_196_plain": (1, (2, 196, 3, 3), False, False),
            "residual_196_ls": (1, (2, 196, 3, 3), True, False), "residual_196_rowscale": (1, (2, 196, 3, 3), False, True)}


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("name", list(BN_CASES))
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_batchnorm_epilogues(mode, name, train):
    kind, shape, with_ls, with_rs = BN_CASES[name]
    B, C = shape[:2]
    g = torch.Generator().manual_seed(len(name))
    params = _bn_params(C, 7)
    x = torch.randn(shape, generator=g) * 1.5 + 0.3
    w = torch.randn(shape, generator=g)
    rowscale = torch.tensor([0.0, 2.0]) if with_rs else None        # one sample dropped, the other scaled by 1 / keep
    if kind == 1:
        params["res"] = torch.randn(shape, generator=g)
        if with_ls:
            params["ls"] = 0.5 + 0.2 * torch.randn(C, generator=g)

    def fn(t, p):
        stats = {}
        if kind == 0:
            y = mm.bn_gelu_tanh_ref(t, p, "bn", 1e-5, train, stats)
        else:
            y = mm.bn_scale_residual_ref(t, p, "bn", 1e-5, train, p["res"].to(t.dtype), p.get("ls"), rowscale, stats)
        return {"out": y, **{k[3:]: v for k, v in stats.items()}}
    ref, ref_g = _ref_run(fn, params, x, w)
    dtype = _mode_dtype(mode)
    bn = _bn_holder(params, C, 1e-5)
    xin = x.to(DEV, dtype).requires_grad_(True)
    if kind == 0:
        out = cops.batch_norm_gelu_tanh(xin, bn, train)
    else:
        res = params["res"].to(DEV, dtype).requires_grad_(True)
        ls = params["ls"].to(DEV).requires_grad_(True) if with_ls else None
        out = cops.batch_norm_scale_residual(xin, bn, train, res, ls, rowscale.to(DEV) if with_rs else None)
    (out.float() * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {"x": xin.grad, "bn.weight": bn.weight.grad, "bn.bias": bn.bias.grad}
    if kind == 1:
        grads["res"] = res.grad
        if with_ls:
            grads["ls"] = ls.grad
    outs = {"out": out.detach()}
    if train:
        outs.update(running_mean=bn.running_mean, running_var=bn.running_var)
    else:
        assert torch.equal(bn.running_mean.cpu(), params["bn.running_mean"]) and torch.equal(bn.running_var.cpu(), params["bn.running_var"])
    for t in (out, xin.grad):
        rows = cops._rows(t)
        assert not rows[..., C:].any()
    if mode == "f32":
        _assert_f32(f"bn {name} train {train}", outs, grads, ref, ref_g)
    else:
        cpu, cpu_g = _ref_run(fn, params, x, w, bf16=True)
        _assert_bf16(f"bn {name} train {train}", outs, grads, cpu, cpu_g, ref, ref_g)
    if with_rs:
        # the dropped sample leaves as its residual; in eval mode nothing flows back into it (in train mode it still moves the
        # batch statistics)
        assert torch.equal(out[0].float().cpu(), params["res"][0].to(dtype).float())
        assert train or not grads["x"][0].any()


# ------------------------------------------------------------------------------------------------ NHWC window partition / reverse
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("name,shape,ws", [("single", (2, 16, 4, 4), 4), ("2x2", (2, 24, 6, 6), 3), ("padded", (2, 12, 5, 7), 4),
                                           ("single_odd_channels", (1, 12, 3, 3), 3)])
def test_nhwc_window_partition_and_reverse_are_the_permutations(name, shape, ws, dtype):
    B, C, H, W = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(dtype)
    xg = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    tok = cops.window_partition_nhwc(xg, ws)
    want = mr.window_partition_ref(x, ws)
    assert tok.dtype == dtype and torch.equal(tok.cpu(), want)
    if name == "single":
        assert tok.data_ptr() == xg.data_ptr()                       # a view: no kernel ran
    back = cops.window_reverse_nhwc(tok, ws, H, W)
    assert tuple(back.shape) == shape and torch.equal(back.cpu(), x)             # the round trip is the identity
    assert not cops._rows(back)[..., C:].any()
    t2 = torch.randn(want.shape, generator=torch.Generator().manual_seed(4)).to(dtype)
    tg = t2.to(DEV).requires_grad_(True)
    m = cops.window_reverse_nhwc(tg, ws, H, W)
    assert torch.equal(m.cpu(), mr.window_reverse_ref(t2, ws, H, W))
    # each direction is the other's backward
    cot = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(dtype)
    m.backward(cot.to(DEV))
    assert torch.equal(tg.grad.cpu(), mr.window_partition_ref(cot, ws))
    tok.backward(t2.to(DEV))
    assert torch.equal(xg.grad.cpu(), mr.window_reverse_ref(t2, ws, H, W))


# ------------------------------------------------------------------------------------------------ modules
def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith(("bias", "gamma")) or "norm" in n or "conv_down.1." in n or "conv_down.4." in n:
                p.add_(0.2 * torch.randn(p.shape, generator=g))
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.add_(0.1 * torch.randn(b.shape, generator=g))
            elif n.endswith("running_var"):
                b.mul_(1 + 0.2 * torch.rand(b.shape, generator=g))
    return m


def _module_gpu(m, x, w, train, call=None):
    m = copy.deepcopy(m).to(DEV).train(train)
    xin = x.to(DEV).requires_grad_(True)
    out = (call or (lambda mod, t: mod(t)))(m, xin)
    outs = out if isinstance(out, dict) else {"out": out}
    first = next(iter(outs.values()))
    assert tuple(first.shape) == tuple(w.shape)
    (first.float() * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in m.named_parameters()}
    grads["x"] = xin.grad
    outs = {k: v.detach() for k, v in outs.items()}
    if train:
        outs.update({k: v for k, v in m.state_dict().items() if "running_" in k})
    return outs, grads, m


def _module_case(m, x, w, fn, train, mode, what):
    params = m.state_dict()

    def run(t, p):
        stats = {}
        out = fn(t, p, stats)
        return {"out": out, **stats} if not isinstance(out, dict) else {**out, **stats}
    ref, ref_g = _ref_run(run, params, x, w)
    outs, g, _ = _module_gpu(m, x, w, train)
    if mode == "f32":
        _assert_f32(what, outs, g, ref, ref_g, train)
    else:
        cpu, cpu_g = _ref_run(run, params, x, w, bf16=True)
        _assert_bf16(what, outs, g, cpu, cpu_g, ref, ref_g, train)


def _set_mode(mode):
    hamspine.set_compute_dtype(mode)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_patch_embed_conv_block_and_downsample(mode, train):
    from ConNexT.models.block.mamba_vision import ConvBlock, Downsample, PatchEmbed
    _set_mode(mode)
    try:
        g = torch.Generator().manual_seed(11)
        torch.manual_seed(12)
        pe = _perturb(PatchEmbed(3, 16, 24), 13)
        x = torch.randn(2, 3, 18, 14, generator=g)
        _module_case(pe, x, torch.randn(2, 24, 5, 4, generator=g), lambda t, p, s: mm.patch_embed_ref(t, p, train, s), train, mode,
                     f"PatchEmbed train {train}")
        for dim, ls in ((24, 0.5), (196, None)):
            cb = _perturb(ConvBlock(dim, layer_scale=ls), 14)
            x = torch.randn(2, dim, 5, 4, generator=g)
            _module_case(cb, x, torch.randn(2, dim, 5, 4, generator=g), lambda t, p, s: mm.conv_block_ref(t, p, train, None, s), train,
                         mode, f"ConvBlock({dim}, layer_scale={ls}) train {train}")
        ds = Downsample(24)
        x = torch.randn(2, 24, 5, 4, generator=g)
        _module_case(ds, x, torch.randn(2, 48, 3, 2, generator=g), lambda t, p, s: mm.downsample_ref(t, p), train, mode, "Downsample")
    finally:
        _set_mode("bf16")


def test_conv_block_drop_path_draws_once_per_sample(f32_mode):
    from ConNexT.models.block.mamba_vision import ConvBlock
    torch.manual_seed(21)
    cb = _perturb(ConvBlock(16, drop_path=0.5, layer_scale=0.5), 22).to(DEV).train()
    x = torch.randn(8, 16, 4, 4, device=DEV)
    keep = copy.deepcopy(cb)
    keep.drop_path_rate = 0.0
    full = keep(x) - x                                               # the branch without stochastic depth
    seen = set()
    for _ in range(6):
        d = (copy.deepcopy(cb)(x) - x).float()
        for b in range(8):
            ratio = (d[b].norm() / full[b].float().norm()).item()
            assert abs(ratio) <= 1e-4 or abs(ratio - 2.0) <= 1e-3, ratio        # dropped, or scaled by 1 / keep
            seen.add(round(ratio))
    assert seen == {0, 2}
    # eval mode draws nothing (a fresh copy without the rate: `keep` has taken a train step, its running statistics moved)
    plain = copy.deepcopy(cb)
    plain.drop_path_rate = 0.0
    assert torch.equal(cb.eval()(x), plain.eval()(x))


_model_cache = {}


def _golden_model():
    if "m" not in _model_cache:
        from ConNexT.models.block.mamba_vision import MambaVision
        z = np.load(GOLDEN)
        sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
        m = MambaVision(**SMALL_KW)
        m.load_state_dict(sd, strict=True)
        x, w = torch.from_numpy(z["x"]), torch.from_numpy(z["cotangent"])

        def run(t, p):
            stats = {}
            logits, fusion = mm.model_ref(t if t.dtype != BF16 else t.float(), p, SMALL_KW["num_heads"], SMALL_KW["window_size"],
                                          BF16 if t.dtype == BF16 else None, torch.float32 if t.dtype == BF16 else None, True, stats)
            return {"logits": logits, "fusion": fusion, **stats}
        _model_cache.update(m=m, z=z, x=x, w=w, run=run, ref=_ref_run(run, sd, x, w))
    return _model_cache


def _model_call(mod, t):
    fusion = mod.forward_features_mamba_fusion(t).detach()
    for k, v in _model_cache["before"].items():                      # the first pass updated the running statistics: put them back
        mod.state_dict()[k].copy_(v)                                 # (reading the state dict flushes the step counters first)
    return {"logits": mod(t), "fusion": fusion}


def test_small_model_f32_against_the_fixture_and_the_yardstick(f32_mode):
    c = _golden_model()
    z, (ref, ref_g) = c["z"], c["ref"]
    c["before"] = {k: v.clone().to(DEV) for k, v in c["m"].state_dict().items() if "running_" in k or "num_batches" in k}
    outs, g, m = _module_gpu(c["m"], c["x"], c["w"], True, _model_call)
    assert outs["logits"].dtype == torch.float32 and outs["fusion"].dtype == torch.float32 and outs["fusion"].is_contiguous()
    fixture = {"logits": z["logits"], "fusion": z["fusion"], "dx": z["dx"]}
    e = {k: _maxrel(outs[k], torch.from_numpy(fixture[k])) for k in ("logits", "fusion")}
    e["dx"] = _rel(g["x"], torch.from_numpy(z["dx"]))
    after = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("after.")}
    e["running"] = max(_maxrel(m.state_dict()[k], v) for k, v in after.items() if "running_" in k)
    assert all(int(m.state_dict()[k]) == int(v) for k, v in after.items() if "num_batches" in k)
    with torch.no_grad():
        e["eval_logits"] = _maxrel(m.eval()(c["x"].to(DEV)), torch.from_numpy(z["eval_logits"]))
    # the encoder's reshape reads the NCHW memory of the map
    e["encoder_reshape"] = _maxrel(outs["fusion"].reshape(2, 18, -1), torch.from_numpy(z["fusion"]).reshape(2, 18, -1))
    print("small MambaVision f32 against the fixture:", {k: f"{v:.2e}" for k, v in e.items()})
    assert all(v <= (1e-3 if k == "dx" else 1e-4) for k, v in e.items()), e
    _assert_f32("small MambaVision", outs, g, ref, ref_g)


def test_small_model_bf16_within_twice_the_cpu_bf16_error():
    c = _golden_model()
    ref, ref_g = c["ref"]
    c["before"] = {k: v.clone().to(DEV) for k, v in c["m"].state_dict().items() if "running_" in k or "num_batches" in k}
    cpu, cpu_g = _ref_run(c["run"], c["m"].state_dict(), c["x"], c["w"], bf16=True)
    outs, g, _ = _module_gpu(c["m"], c["x"], c["w"], True, _model_call)
    assert outs["logits"].dtype == torch.float32 and outs["fusion"].dtype == torch.float32
    _assert_bf16("small MambaVision", outs, g, cpu, cpu_g, ref, ref_g)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_tiny_variant_and_encoder_run_forward_and_backward_at_224(mode):
    from ConNexT.models.block.mamba_vision import MambaVisionEncoder, mamba_vision_T
    _set_mode(mode)
    try:
        torch.manual_seed(40)
        x = torch.randn(2, 3, 224, 224, device=DEV)
        model = mamba_vision_T().to(DEV).train()
        logits = model(x)
        assert tuple(logits.shape) == (2, 1000) and logits.dtype == torch.float32 and torch.isfinite(logits).all()
        logits.square().mean().backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
        enc = MambaVisionEncoder(pretrained=False, model_variant="T").to(DEV).train()
        tokens = enc(x)
        assert tuple(tokens.shape) == (2, 1568, 20) and tokens.dtype == torch.float32 and torch.isfinite(tokens).all()
        tokens.square().mean().backward()
        used = [p for n, p in enc.named_parameters() if not n.startswith(("projection", "mamba_vision.norm"))]
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in used)
        assert enc.projection.weight.grad is None
    finally:
        _set_mode("bf16")
