"""MambaVision mixer, Block and hybrid stage (reference ConNexT/models/block/mamba_vision.py) on the GPU: the centred conv1d, the
8-state gate-less scan, the window partition / reverse and the drop-in modules against tests/mambavision_ref.py in float64.

Gates, f32 mode: outputs <= 1e-4 * max|ref| and every gradient <= 1e-3 in relative L2 norm (the bounds the scan already has,
tests/test_mamba_general_gpu.py).  bf16 mode: the yardstick itself is run on the CPU with bfloat16 activations and an f32 state
under the module's dtype policy; the GPU may show at most twice its error against float64, with the f32 round-off floor
F32_NOISE.  The window kernels are permutations and are compared bitwise.  A_log and dt_proj.bias come from the real
initialiser, so dt and the decays are in their working range."""
import copy
import os

import numpy as np
import pytest
import torch

import mambavision_ref as mr

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from hamspine import _lib as L  # noqa: E402
from hamspine import mambavision_ops as ops  # noqa: E402
from hamspine import rt  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mambavision_layer.npz")
# relative errors below this are f32 round-off, not bf16 (tests/test_mamba_general_gpu.py explains the floor)
F32_NOISE = 1e-6


def _chunk():
    return int(L.lib().hs_selective_scan_chunk_len_nogate(8))


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
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _assert_f32(what, out, g, ref, ref_g):
    e = _maxrel(out, ref)
    print(f"{what} f32: out {e:.2e}", {k: f"{_rel(g[k], ref_g[k]):.2e}" if g.get(k) is not None else "missing" for k in ref_g})
    assert e <= 1e-4
    for k in ref_g:
        assert g.get(k) is not None, k
        assert _rel(g[k], ref_g[k]) <= 1e-3, k


def _assert_within_twice_the_cpu_bf16_error(what, out, g, cpu_out, cpu_g, ref, ref_g):
    e_gpu, e_cpu = _maxrel(out, ref), _maxrel(cpu_out, ref)
    rows = {k: (_rel(g[k], ref_g[k]) if g.get(k) is not None else None, _rel(cpu_g[k], ref_g[k])) for k in ref_g}
    print(f"{what} bf16 against float64 (GPU, CPU bf16 yardstick): out {e_gpu:.2e} {e_cpu:.2e}",
          {k: f"{a:.2e} {b:.2e}" if a is not None else "missing" for k, (a, b) in rows.items()})
    assert e_gpu <= max(2 * e_cpu, F32_NOISE)
    for k, (a, b) in rows.items():
        assert a is not None, k
        assert a <= max(2 * b, F32_NOISE), k


# ------------------------------------------------------------------------------------------------------ conv
def _conv_inputs(B, Lt, d, bias, seed):
    g = torch.Generator().manual_seed(seed)
    t = {"xz": torch.randn(B, Lt, 2 * d, generator=g), "weight": 0.6 * torch.randn(d, 1, 3, generator=g),
         "w": torch.randn(B, Lt, d, generator=g)}
    if bias:
        t["bias"] = 0.3 * torch.randn(d, generator=g)
    return {k: v.double() for k, v in t.items()}


def _conv_run(t, d, half, device=DEV, dtype=torch.float32):
    """the input is the left or right column half of xz (B, L, 2d); on the GPU the output goes to the other half of a (B, L, 2d)
    buffer, whose remaining half must stay as it was"""
    sl = slice(0, d) if half == "left" else slice(d, 2 * d)
    if device == "cpu" and dtype != BF16:
        leaf = {k: v.clone().requires_grad_(k != "w") for k, v in t.items()}
    else:
        leaf = {k: v.to(device, dtype if k in ("xz", "w") else torch.float32).requires_grad_(k != "w") for k, v in t.items()}
    x = leaf["xz"][..., sl]
    if device == "cpu":
        out = mr.conv_same_ref(x, leaf["weight"], leaf.get("bias"))
    else:
        buf = torch.full(tuple(leaf["xz"].shape), 7.0, device=DEV, dtype=dtype)
        so = slice(d, 2 * d) if half == "left" else slice(0, d)
        out = ops.conv1d_same_silu(x, leaf["weight"], leaf.get("bias"), out=buf[..., so])
        assert out.data_ptr() == buf[..., so].data_ptr() and torch.equal(buf[..., sl], torch.full_like(buf[..., sl], 7.0))
    wide = leaf["weight"].dtype
    (out.to(wide) * leaf["w"].to(wide)).sum().backward()
    return out.detach(), {k: leaf[k].grad for k in leaf if k != "w"}


@pytest.mark.parametrize("half", ["left", "right"])
@pytest.mark.parametrize("shape", [(1, 1, 8), (2, 2, 40), (2, 19, 40)], ids=["1x1x8", "2x2x40", "2x19x40"])
def test_conv1d_same_silu_f32_against_float64(shape, half, f32_mode):
    B, Lt, d = shape
    t = _conv_inputs(B, Lt, d, bias=half == "right", seed=2000 + Lt + d)
    ref, ref_g = _conv_run(t, d, half, device="cpu")
    out, g = _conv_run(t, d, half)
    torch.cuda.synchronize()
    other = slice(d, 2 * d) if half == "left" else slice(0, d)
    assert torch.count_nonzero(g["xz"][..., other]).item() == 0
    _assert_f32(f"conv {B}x{Lt}x{d} {half}", out, g, ref, ref_g)


def test_conv1d_same_silu_bf16_within_twice_the_cpu_bf16_error():
    B, Lt, d = 2, 19, 40
    t = _conv_inputs(B, Lt, d, bias=True, seed=2100)
    ref, ref_g = _conv_run(t, d, "right", device="cpu")
    cpu_out, cpu_g = _conv_run(t, d, "right", device="cpu", dtype=BF16)
    out, g = _conv_run(t, d, "right", dtype=BF16)
    torch.cuda.synchronize()
    assert out.dtype == BF16
    _assert_within_twice_the_cpu_bf16_error("conv 2x19x40", out, g, cpu_out, cpu_g, ref, ref_g)


# ------------------------------------------------------------------------------------------------------ scan
SCAN_GRADS = ("u", "dt", "bc", "A_log", "D", "dt_bias")


def _scan_inputs(B, Lt, d, seed):
    """float64 CPU leaves laid out as the mixer lays them out: u and dt contiguous, Bm / Cm the halves of the (B, L, 16) copy of
    the x_proj output's tail; the per-channel parameters come from the mixer's initialiser"""
    from ConNexT.models.block.mamba_vision import MambaVisionMixer
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    mix = MambaVisionMixer(2 * d, d_state=8, d_conv=3, expand=1)
    t = {
        "u": torch.randn(B, Lt, d, generator=g),
        "dt": 0.5 * torch.randn(B, Lt, d, generator=g),
        "bc": torch.randn(B, Lt, 16, generator=g),
        "A_log": mix.A_log.detach() + 0.1 * torch.randn(d, 8, generator=g),
        "D": mix.D.detach() + 0.3 * torch.randn(d, generator=g),
        "dt_bias": mix.dt_proj.bias.detach().clone(),
        "w": torch.randn(B, Lt, d, generator=g),
    }
    return {k: v.double() for k, v in t.items()}


def _scan_run(t, device=DEV, dtype=torch.float32):
    """forward + backward of the gate-less scan: the HIP kernels on the GPU in `dtype`, writing the left half of a (B, L, 2d)
    buffer as in the mixer; on the CPU the yardstick's loop in float64, or (bfloat16) with an f32 state"""
    acts = ("u", "dt", "bc", "w")
    if device == "cpu" and dtype != BF16:
        leaf = {k: v.clone().requires_grad_(k != "w") for k, v in t.items()}
    else:
        leaf = {k: v.to(device, dtype if k in acts else torch.float32).requires_grad_(k != "w") for k, v in t.items()}
    if device == "cpu":
        out = mr.scan_ref(leaf["u"], leaf["dt"], leaf["dt_bias"], leaf["A_log"], leaf["bc"][..., :8], leaf["bc"][..., 8:], leaf["D"],
                          torch.float32 if dtype == BF16 else None)
    else:
        B, Lt, d = leaf["u"].shape
        buf = torch.full((B, Lt, 2 * d), 7.0, device=DEV, dtype=dtype)
        out = ops.selective_scan_nogate(leaf["u"], leaf["dt"], leaf["dt_bias"], leaf["A_log"], leaf["bc"], leaf["D"], out=buf[..., :d])
        assert torch.equal(buf[..., d:], torch.full_like(buf[..., d:], 7.0))
    (out.to(leaf["D"].dtype) * leaf["w"].to(leaf["D"].dtype)).sum().backward()
    return out.detach().clone(), {k: leaf[k].grad for k in SCAN_GRADS}


def _scan_shape(which):
    lc = _chunk()
    return [(1, 1, 32), (2, lc + 1, 40), (1, 2 * lc + 3, 32)][which]


@pytest.mark.parametrize("which", range(3), ids=["1x1x32", "2x(Lc+1)x40", "1x(2Lc+3)x32"])
def test_gateless_scan_f32_against_float64(which, f32_mode):
    assert _chunk() == 16
    B, Lt, d = _scan_shape(which)
    t = _scan_inputs(B, Lt, d, 2200 + which)
    ref, ref_g = _scan_run(t, device="cpu")
    out, g = _scan_run(t)
    torch.cuda.synchronize()
    _assert_f32(f"scan N 8 {B}x{Lt}x{d}", out, g, ref, ref_g)


def test_gateless_scan_bf16_within_twice_the_cpu_bf16_error():
    B, Lt, d = _scan_shape(1)
    t = _scan_inputs(B, Lt, d, 2300)
    ref, ref_g = _scan_run(t, device="cpu")
    cpu_out, cpu_g = _scan_run(t, device="cpu", dtype=BF16)
    out, g = _scan_run(t, dtype=BF16)
    torch.cuda.synchronize()
    assert out.dtype == BF16
    _assert_within_twice_the_cpu_bf16_error(f"scan N 8 {B}x{Lt}x{d}", out, g, cpu_out, cpu_g, ref, ref_g)


def test_gateless_scan_repeats_bitwise(f32_mode):
    B, Lt, d = _scan_shape(1)
    t = _scan_inputs(B, Lt, d, 2400)
    out1, g1 = _scan_run(t)
    out2, g2 = _scan_run(t)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("t_cut", ["1", "Lc"])
def test_gateless_scan_is_causal(t_cut, f32_mode):
    lc = _chunk()
    cut = 1 if t_cut == "1" else lc
    B, Lt, d = 2, 2 * lc + 3, 32
    t = _scan_inputs(B, Lt, d, 2500)
    base, _ = _scan_run(t)
    g = torch.Generator().manual_seed(2501)
    t2 = dict(t)
    for k in ("u", "dt", "bc"):
        v = t[k].clone()
        v[:, cut:] = torch.randn(v[:, cut:].shape, generator=g).double()
        t2[k] = v
    other, _ = _scan_run(t2)
    torch.cuda.synchronize()
    assert torch.equal(base[:, :cut], other[:, :cut])
    assert not torch.equal(base[:, cut:], other[:, cut:])


# ---------------------------------------------------------------------------------------- window partition / reverse
_WINDOW_CASES = {"2x16x5x5-ws3-padded": ((2, 16, 5, 5), 3), "1x24x4x6-ws2": ((1, 24, 4, 6), 2), "2x16x3x3-ws3-one-window": ((2, 16, 3, 3), 3)}


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(_WINDOW_CASES))
def test_window_partition_and_reverse_are_the_permutations(name, dtype):
    shape, ws = _WINDOW_CASES[name]
    B, C, H, W = shape
    g = torch.Generator().manual_seed(2600 + H * W)
    x = torch.randn(shape, generator=g)
    ref_tok = mr.window_partition_ref(x, ws)                                 # f32 on the CPU
    xin = x.to(DEV).requires_grad_(True)
    tok = ops.window_partition(xin, ws, dtype)
    assert tok.dtype == dtype and tuple(tok.shape) == tuple(ref_tok.shape)
    assert torch.equal(tok.detach().cpu(), ref_tok.to(dtype))
    pad = mr.window_partition_ref(torch.ones(shape), ws) == 0                # the tokens of padded positions
    assert (H % ws == 0 and W % ws == 0) == (not pad.any().item())
    assert torch.count_nonzero(tok.detach().cpu()[pad]).item() == 0
    # reverse(partition(x)) is x (through a bf16 token buffer: x rounded)
    back = ops.window_reverse(tok, ws, H, W)
    assert back.dtype == torch.float32 and torch.equal(back.detach().cpu(), x.to(dtype).float())
    # the backward of the partition is the reverse of the cotangent ...
    ct = torch.randn(ref_tok.shape, generator=g).to(dtype)
    tok.backward(ct.to(DEV))
    assert xin.grad.dtype == torch.float32 and torch.equal(xin.grad.cpu(), mr.window_reverse_ref(ct.float(), ws, H, W))
    # ... and the backward of the reverse is the partition of the cotangent
    tin = ref_tok.to(dtype).to(DEV).requires_grad_(True)
    cm = torch.randn(shape, generator=g)
    out = ops.window_reverse(tin, ws, H, W)
    assert torch.equal(out.detach().cpu(), mr.window_reverse_ref(ref_tok.to(dtype).float(), ws, H, W))
    out.backward(cm.to(DEV))
    torch.cuda.synchronize()
    assert tin.grad.dtype == dtype and torch.equal(tin.grad.cpu(), mr.window_partition_ref(cm, ws).to(dtype))


def test_module_level_window_functions_follow_the_reference_signature(f32_mode):
    from ConNexT.models.block.mamba_vision import window_partition, window_reverse
    x = torch.randn(1, 24, 4, 6, generator=torch.Generator().manual_seed(2650))
    tok = window_partition(x.to(DEV), 2)
    assert torch.equal(tok.cpu(), mr.window_partition_ref(x, 2))
    assert torch.equal(window_reverse(tok, 2, 4, 6).cpu(), x)


# ------------------------------------------------------------------------------------------------ modules
def _leaves(sd, dtype):
    return {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}


def _perturb(m, seed):
    """generic values where the initialisers give constants (D, LayerNorm, layer scale, zero biases); A_log and dt_proj.bias
    stay as initialised"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "dt_proj" not in n and (n.endswith(("D", "bias", "gamma_1", "gamma_2")) or "norm" in n):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    return m


def _ref_run(fn, m, x, w, bf16=False):
    """the yardstick on the CPU: float64 throughout, or (bf16) f32 leaves with bfloat16 activations and an f32 state.  fn(x,
    params, bf16) -> output"""
    keep = torch.float32 if bf16 else torch.float64
    sd = _leaves(m.state_dict(), keep)
    xin = x.detach().clone().to(keep).requires_grad_(True)
    out = fn(xin, sd, bf16)
    (out.to(keep) * w.to(keep)).sum().backward()
    grads = {k: v.grad for k, v in sd.items()}
    grads["x"] = xin.grad
    return out.detach(), grads


def _gpu_run(m, x, w, dtype, train=True):
    m = copy.deepcopy(m).to(DEV).train(train)
    xin = x.to(DEV, dtype).requires_grad_(True)
    out = m(xin)
    assert out.dtype == dtype and tuple(out.shape) == tuple(x.shape)
    (out.float() * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in m.named_parameters()}
    grads["x"] = xin.grad
    return out.detach(), grads


def _mixer_fn(x, p, bf16):
    return mr.mixer_ref(x.to(BF16), p, torch.float32) if bf16 else mr.mixer_ref(x, p)


_cases = {}


def _mixer_case(dim, Lt):
    key = ("mixer", dim, Lt)
    if key not in _cases:
        from ConNexT.models.block.mamba_vision import MambaVisionMixer
        torch.manual_seed(2700 + dim)
        m = _perturb(MambaVisionMixer(dim, d_state=8, d_conv=3, expand=1), 2701)
        g = torch.Generator().manual_seed(2702 + dim)
        x, w = torch.randn(2, Lt, dim, generator=g), torch.randn(2, Lt, dim, generator=g)
        _cases[key] = (m, x, w) + _ref_run(_mixer_fn, m, x, w)
    return _cases[key]


@pytest.mark.parametrize("dim", [32, 80])
def test_mixer_f32_against_float64(dim, f32_mode):
    """MambaVisionMixer(32) at (2, 9, 32); MambaVisionMixer(80) at (2, Lc + 1, 80): dt rank 5, padded to 8"""
    m, x, w, ref, ref_g = _mixer_case(dim, 9 if dim == 32 else _chunk() + 1)
    out, g = _gpu_run(m, x, w, torch.float32)
    assert sorted(g) == sorted(ref_g)
    _assert_f32(f"MambaVisionMixer({dim})", out, g, ref, ref_g)


def test_mixer_bf16_within_twice_the_cpu_bf16_error():
    hamspine.set_compute_dtype("bf16")
    m, x, w, ref, ref_g = _mixer_case(80, _chunk() + 1)
    cpu_out, cpu_g = _ref_run(_mixer_fn, m, x, w, bf16=True)
    out, g = _gpu_run(m, x, w, BF16)
    _assert_within_twice_the_cpu_bf16_error("MambaVisionMixer(80)", out, g, cpu_out, cpu_g, ref, ref_g)


def _block_fn(heads):
    def fn(x, p, bf16):
        return mr.block_ref(x.to(BF16), p, heads, state_dtype=torch.float32) if bf16 else mr.block_ref(x, p, heads)
    return fn


def _block_case(kind, layer_scale, dim=32, rows=2, **kw):
    key = ("block", kind, layer_scale, dim, rows, tuple(sorted(kw.items())))
    if key not in _cases:
        from ConNexT.models.block.mamba_vision import Block
        torch.manual_seed(2800 + dim)
        m = _perturb(Block(dim, 2, 0, [0] if kind == "attn" else [], qkv_bias=True, layer_scale=layer_scale, **kw), 2801)
        g = torch.Generator().manual_seed(2802)
        x, w = torch.randn(rows, 9, dim, generator=g), torch.randn(rows, 9, dim, generator=g)
        _cases[key] = (m, x, w) + _ref_run(_block_fn(2), m, x, w)
    return _cases[key]


@pytest.mark.parametrize("layer_scale", [None, 0.5])
@pytest.mark.parametrize("kind", ["mamba", "attn"])
def test_block_f32_against_float64(kind, layer_scale, f32_mode):
    m, x, w, ref, ref_g = _block_case(kind, layer_scale)
    out, g = _gpu_run(m, x, w, torch.float32)
    assert sorted(g) == sorted(ref_g)
    _assert_f32(f"Block {kind} layer_scale {layer_scale}", out, g, ref, ref_g)


@pytest.mark.parametrize("kind,dim", [("mamba", 32), ("attn", 80)], ids=["mamba-32", "attn-80-head-dim-40"])
def test_block_bf16_within_twice_the_cpu_bf16_error(kind, dim):
    hamspine.set_compute_dtype("bf16")
    m, x, w, ref, ref_g = _block_case(kind, 0.5, dim=dim)
    cpu_out, cpu_g = _ref_run(_block_fn(2), m, x, w, bf16=True)
    out, g = _gpu_run(m, x, w, BF16)
    _assert_within_twice_the_cpu_bf16_error(f"Block {kind} dim {dim}", out, g, cpu_out, cpu_g, ref, ref_g)


def test_drop_path_changes_nothing_in_eval_mode(f32_mode):
    m, x, w, _, _ = _block_case("mamba", 0.5)
    dropped = copy.deepcopy(m)
    dropped.drop_path_rate = 0.7
    with torch.no_grad():
        a = copy.deepcopy(m).to(DEV).eval()(x.to(DEV))
        b = dropped.to(DEV).eval()(x.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_drop_path_draws_per_window_row_and_branch(f32_mode):
    """train mode, drop_path 0.5, no layer scale: every window row of the output is one of the four keep / drop combinations of
    the two branches (kept branches scaled by 1 / (1 - p) = 2), recomputed in float64"""
    m, x, w, _, _ = _block_case("mamba", None, rows=8, drop_path=0.5)
    assert m.drop_path_rate == 0.5
    params = {k: v.double() for k, v in m.state_dict().items()}
    rows = x.shape[0]
    with torch.no_grad():
        combos = {(a, b): mr.block_ref(x.double(), params, 2, torch.full((rows,), a), torch.full((rows,), b))
                  for a in (0.0, 2.0) for b in (0.0, 2.0)}
        torch.manual_seed(2900)
        out = copy.deepcopy(m).to(DEV).train()(x.to(DEV))
    torch.cuda.synchronize()
    seen = set()
    for r in range(rows):
        hits = [k for k, c in combos.items() if _maxrel(out[r], c[r]) <= 1e-4]
        assert len(hits) == 1, (r, hits)
        seen.add(hits[0])
    print("keep / drop combinations drawn:", sorted(seen))
    assert len(seen) >= 2


# ------------------------------------------------------------------------------------------------ stage
def _layer_fn(heads, ws):
    def fn(x, p, bf16):
        return mr.layer_ref(x, p, heads, ws, BF16 if bf16 else None, torch.float32 if bf16 else None)
    return fn


def _golden_case():
    if "golden" not in _cases:
        from ConNexT.models.block.mamba_vision import MambaVisionLayer
        z = np.load(GOLDEN)
        m = MambaVisionLayer(dim=32, depth=2, num_heads=2, window_size=3, conv=False, downsample=False, transformer_blocks=[1],
                             layer_scale=0.5)
        m.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}, strict=True)
        _cases["golden"] = (m, torch.from_numpy(z["x"]), torch.from_numpy(z["cotangent"]), torch.from_numpy(z["out"]),
                            torch.from_numpy(z["dx"]))
    return _cases["golden"]


def test_stage_golden_case_f32_against_the_reference(f32_mode):
    m, x, w, ref, ref_dx = _golden_case()
    out, g = _gpu_run(m, x, w, torch.float32)
    e, edx = _maxrel(out, ref), _rel(g["x"], ref_dx)
    print(f"MambaVisionLayer golden f32: out {e:.2e} dx {edx:.2e}")
    assert e <= 1e-4 and edx <= 1e-3
    assert all(v is not None and torch.isfinite(v).all() for v in g.values())


def test_stage_golden_case_bf16_within_twice_the_cpu_bf16_error():
    hamspine.set_compute_dtype("bf16")
    m, x, w, _, _ = _golden_case()
    ref, ref_g = _ref_run(_layer_fn(2, 3), m, x, w)
    cpu_out, cpu_g = _ref_run(_layer_fn(2, 3), m, x, w, bf16=True)
    out, g = _gpu_run(m, x, w, torch.float32)                  # the stage takes and returns f32 in either mode
    _assert_within_twice_the_cpu_bf16_error("MambaVisionLayer golden", out, g, cpu_out, cpu_g, ref, ref_g)


def test_stage_single_window_f32_against_float64(f32_mode):
    from ConNexT.models.block.mamba_vision import MambaVisionLayer
    torch.manual_seed(3000)
    m = _perturb(MambaVisionLayer(dim=32, depth=2, num_heads=2, window_size=3, conv=False, downsample=False, transformer_blocks=[1]),
                 3001)
    g = torch.Generator().manual_seed(3002)
    x, w = torch.randn(2, 32, 3, 3, generator=g), torch.randn(2, 32, 3, 3, generator=g)
    ref, ref_g = _ref_run(_layer_fn(2, 3), m, x, w)
    out, gg = _gpu_run(m, x, w, torch.float32)
    assert sorted(gg) == sorted(ref_g)
    _assert_f32("MambaVisionLayer (2, 32, 3, 3) ws 3", out, gg, ref, ref_g)


def test_stage_at_the_model_width_bf16():
    """MambaVisionLayer(320, depth 2, 8 heads, window 14) on (2, 320, 14, 14): the only test with 5 channel blocks of the scan
    and 196 steps.  Forward + backward finish and are finite, every parameter has a gradient, and the output agrees with the
    bf16 yardstick under the twice-the-CPU-error rule."""
    from ConNexT.models.block.mamba_vision import MambaVisionLayer
    hamspine.set_compute_dtype("bf16")
    torch.manual_seed(3100)
    m = _perturb(MambaVisionLayer(dim=320, depth=2, num_heads=8, window_size=14, conv=False, downsample=False, transformer_blocks=[1]),
                 3101)
    g = torch.Generator().manual_seed(3102)
    x, w = torch.randn(2, 320, 14, 14, generator=g), torch.randn(2, 320, 14, 14, generator=g)
    out, grads = _gpu_run(m, x, w, torch.float32)
    assert torch.isfinite(out).all()
    for k, v in grads.items():
        assert v is not None and torch.isfinite(v).all() and v.abs().max().item() > 0, k
    with torch.no_grad():
        params = {k: v.detach() for k, v in m.state_dict().items()}
        ref = mr.layer_ref(x.double(), {k: v.double() for k, v in params.items()}, 8, 14)
        cpu = mr.layer_ref(x, params, 8, 14, BF16, torch.float32)
    e_gpu, e_cpu = _maxrel(out, ref), _maxrel(cpu, ref)
    print(f"MambaVisionLayer(320) bf16 against float64 (GPU, CPU bf16 yardstick): out {e_gpu:.2e} {e_cpu:.2e}")
    assert e_gpu <= max(2 * e_cpu, F32_NOISE)


# ------------------------------------------------------------------------------------------------ argument checks
def test_unsupported_arguments_are_refused_without_a_launch():
    lib = L.lib()
    B, Lt, d = 1, 4, 64
    x = torch.zeros(B, Lt, d, device=DEV)
    bc = torch.zeros(B, Lt, 32, device=DEV)
    par = torch.zeros(d, 16, device=DEV)
    out = torch.full((B, Lt, d), 7.0, device=DEV)
    p = rt.p

    def scan(n_state, z):
        st = lib.hs_selective_scan_fwd(L.HS_F32, p(x), d, p(x), d, p(par), p(par), p(bc), p(bc, 4 * n_state), 32, p(par), z, d, p(out), d,
                                       None, B, Lt, d, n_state, rt.stream())
        return st, lib.hs_last_error().decode()

    def conv(k, ldx=d):
        st = lib.hs_conv1d_same_silu_fwd(L.HS_F32, p(x), ldx, p(par), None, p(out), d, B, Lt, d, k, rt.stream())
        return st, lib.hs_last_error().decode()
    st, msg = scan(8, p(x))
    assert st == 3 and "d_state 8" in msg and "gate" in msg, (st, msg)          # HS_ERR_UNSUPPORTED
    st, msg = scan(16, None)
    assert st == 3 and "z = NULL" in msg and "d_state 16" in msg, (st, msg)
    st, msg = conv(4)
    assert st == 3 and "kernel size 4" in msg, (st, msg)
    st, msg = conv(3, ldx=d + 1)
    assert st == 3 and "16 bytes" in msg, (st, msg)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))      # nothing ran
    assert scan(8, None)[0] == 0 and conv(3)[0] == 0        # the supported forms of the same calls run
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out))
    with pytest.raises(L.HamspineError, match="column slice"):
        ops.conv1d_same_silu(x, par[:, :3].reshape(d, 1, 3).contiguous(), None, out=torch.empty(B, Lt, 2 * d, device=DEV)[..., ::2])
