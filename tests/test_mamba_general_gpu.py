"""Selective scan for d_state up to 256, Mamba(d_state=128) and the multimodal Mamba blocks (reference
ConNexT/models/block/len4mamba.py) on the GPU against tests/mamba_general_ref.py in float64.

Gates, f32 mode: outputs <= 1e-4 * max|ref| and every gradient <= 1e-3 in relative L2 norm.  bf16 mode: the
yardstick itself is run on the CPU in bfloat16 with an f32 state; the GPU may show at most twice its error against float64
(bf16 GEMM summation order differs between the two; a factor of two covers that and no more).  A_log and dt_proj.bias come from
the real initialiser, so dt and the decays are in their working range."""
import copy

import pytest
import torch

import mamba_general_ref as gr

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from hamspine import _lib as L  # noqa: E402
from hamspine import rt, ssm  # noqa: E402

DEV = "cuda"
SCAN_GRADS = ("u", "dt", "xz", "bc", "A_log", "D", "dt_bias")


def _chunk(N):
    return int(L.lib().hs_selective_scan_chunk_len_n(N))


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


# ------------------------------------------------------------------------------------------------------ scan
def _scan_inputs(B, Lt, d, N, seed):
    """float64 CPU leaves laid out as the module lays them out: z is the right half of the (B, L, 2d) in_proj output, Bm / Cm
    the halves of the (B, L, 2N) copy of the x_proj output's tail; the per-channel parameters come from Mamba's initialiser."""
    from hamspine.nn import Mamba
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    blk = Mamba(d // 2, d_state=N)
    t = {
        "u": torch.randn(B, Lt, d, generator=g),
        "dt": 0.5 * torch.randn(B, Lt, d, generator=g),
        "xz": torch.randn(B, Lt, 2 * d, generator=g),
        "bc": torch.randn(B, Lt, 2 * N, generator=g),
        "A_log": blk.A_log.detach() + 0.1 * torch.randn(d, N, generator=g),
        "D": blk.D.detach() + 0.3 * torch.randn(d, generator=g),
        "dt_bias": blk.dt_proj.bias.detach().clone(),
        "w": torch.randn(B, Lt, d, generator=g),
    }
    return {k: v.double() for k, v in t.items()}


def _scan_run(t, d, N, device=DEV, dtype=torch.float32):
    """forward + backward of the scan on `device`: the HIP kernels on the GPU in `dtype`; on the CPU the yardstick's loop in
    float64, or (dtype bfloat16) with bfloat16 activations, f32 parameters and an f32 state"""
    acts = ("u", "dt", "xz", "bc", "w")
    if device == "cpu" and dtype != torch.bfloat16:
        leaf = {k: v.clone().requires_grad_(k != "w") for k, v in t.items()}
    else:
        leaf = {k: v.to(device, dtype if k in acts else torch.float32).requires_grad_(k != "w") for k, v in t.items()}
    z = leaf["xz"][..., d:]
    if device == "cpu":
        out = gr.scan_ref(leaf["u"], leaf["dt"], leaf["dt_bias"], leaf["A_log"], leaf["bc"][..., :N], leaf["bc"][..., N:],
                          leaf["D"], z, torch.float32 if dtype == torch.bfloat16 else None)
    else:
        out = ssm.selective_scan(leaf["u"], leaf["dt"], leaf["dt_bias"], leaf["A_log"], leaf["bc"], leaf["D"], z)
    (out.to(leaf["D"].dtype) * leaf["w"].to(leaf["D"].dtype)).sum().backward()
    return out.detach(), {k: leaf[k].grad for k in SCAN_GRADS}


def _scan_shape(N, which):
    lc = _chunk(N)
    return [(1, 1, 64), (2, lc + 1, 80), (1, 2 * lc + 3, 64)][which]


@pytest.mark.parametrize("which", range(3), ids=["1x1x64", "2x(Lc+1)x80", "1x(2Lc+3)x64"])
@pytest.mark.parametrize("N", [32, 64, 128, 256])
def test_selective_scan_f32_against_float64(N, which, f32_mode):
    B, Lt, d = _scan_shape(N, which)
    t = _scan_inputs(B, Lt, d, N, 1000 + 10 * N + which)
    ref_out, ref_g = _scan_run(t, d, N, device="cpu")
    out, g = _scan_run(t, d, N)
    torch.cuda.synchronize()
    e = _maxrel(out, ref_out)
    print(f"scan N {N} {B}x{Lt}x{d}: out {e:.2e}", {k: f"{_rel(g[k], ref_g[k]):.2e}" for k in g})
    assert e <= 1e-4
    assert torch.count_nonzero(g["xz"][..., :d]).item() == 0        # the xs half of the in_proj output gets nothing from the scan
    for k in g:
        assert _rel(g[k], ref_g[k]) <= 1e-3, k


# Relative errors below this are f32 round-off (sums of up to a few hundred f32 terms in another order: some 1e-7), not bf16:
# a quantity with no bf16 on its path (norm2.bias of the attention block) shows the same noise on the CPU and on the GPU, and
# twice one noise says nothing about the other.  The floor is two decades under the smallest bf16 effect seen (2e-4).
F32_NOISE = 1e-6


def _assert_within_twice_the_cpu_bf16_error(what, out, g, cpu_out, cpu_g, ref, ref_g):
    e_gpu, e_cpu = _maxrel(out, ref), _maxrel(cpu_out, ref)
    rows = {k: (_rel(g[k], ref_g[k]) if g[k] is not None else None, _rel(cpu_g[k], ref_g[k])) for k in ref_g}
    print(f"{what} bf16 against float64 (GPU, CPU bf16 yardstick): out {e_gpu:.2e} {e_cpu:.2e}",
          {k: f"{a:.2e} {b:.2e}" if a is not None else "missing" for k, (a, b) in rows.items()})
    assert e_gpu <= max(2 * e_cpu, F32_NOISE)
    for k, (a, b) in rows.items():
        assert a is not None, k
        assert a <= max(2 * b, F32_NOISE), k


@pytest.mark.parametrize("N", [32, 64, 256])
def test_selective_scan_bf16_within_twice_the_cpu_bf16_error(N):
    """the bf16 instantiations the Mamba(d_state=128) tests do not reach: 4-, 8- and 2 x 16-byte loads of Bm / Cm per lane"""
    hamspine.set_compute_dtype("bf16")
    B, Lt, d = _scan_shape(N, 1)
    t = _scan_inputs(B, Lt, d, N, 1300 + N)
    ref_out, ref_g = _scan_run(t, d, N, device="cpu")
    cpu_out, cpu_g = _scan_run(t, d, N, device="cpu", dtype=torch.bfloat16)
    out, g = _scan_run(t, d, N, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and torch.count_nonzero(g["xz"][..., :d]).item() == 0
    _assert_within_twice_the_cpu_bf16_error(f"scan N {N} {B}x{Lt}x{d}", out, g, cpu_out, cpu_g, ref_out, ref_g)


def test_scan_128_states_repeats_bitwise(f32_mode):
    N = 128
    B, Lt, d = 2, _chunk(N) + 1, 80
    t = _scan_inputs(B, Lt, d, N, 1400)
    out1, g1 = _scan_run(t, d, N)
    out2, g2 = _scan_run(t, d, N)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("t_cut", ["1", "Lc"])
def test_scan_128_states_is_causal(t_cut, f32_mode):
    N = 128
    lc = _chunk(N)
    cut = 1 if t_cut == "1" else lc
    B, Lt, d = 2, 2 * lc + 3, 64
    t = _scan_inputs(B, Lt, d, N, 1500)
    base, _ = _scan_run(t, d, N)
    g = torch.Generator().manual_seed(1501)
    t2 = dict(t)
    for k in ("u", "dt", "xz", "bc"):
        v = t[k].clone()
        v[:, cut:] = torch.randn(v[:, cut:].shape, generator=g).double()
        t2[k] = v
    other, _ = _scan_run(t2, d, N)
    torch.cuda.synchronize()
    assert torch.equal(base[:, :cut], other[:, :cut])
    assert not torch.equal(base[:, cut:], other[:, cut:])


# ------------------------------------------------------------------------------------------------ Mamba block
def _leaves(sd, dtype):
    """state dict -> leaves of `dtype` (buffers such as the KAN grid stay constants)"""
    return {k: v.detach().to(dtype).requires_grad_(not k.endswith(".grid")) for k, v in sd.items()}


_mamba_cache = {}


def _mamba_case():
    """seeded Mamba(32, d_state=128), input and weights, and the float64 reference; computed once"""
    if _mamba_cache:
        return _mamba_cache["case"]
    from hamspine.nn import Mamba
    torch.manual_seed(1600)
    m = Mamba(32, d_state=128)
    with torch.no_grad():      # generic values where the initialiser gives constants; A_log and dt_proj.bias stay as initialised
        m.D.add_(0.3 * torch.randn_like(m.D))
    g = torch.Generator().manual_seed(1601)
    x = torch.randn(2, 9, 32, generator=g)
    w = torch.randn(2, 9, 32, generator=g)
    _mamba_cache["case"] = (m, x, w) + _mamba_ref_run(m, x, w, torch.float64)
    return _mamba_cache["case"]


def _mamba_ref_run(m, x, w, dtype, state_dtype=None):
    """the yardstick on the CPU: float64 throughout, or activations and weights in `dtype` with the state in state_dtype"""
    keep = torch.float64 if dtype == torch.float64 else torch.float32
    sd = _leaves(m.state_dict(), keep)
    xin = x.detach().clone().to(keep).requires_grad_(True)      # a fresh leaf: x itself is shared between runs
    out = gr.mamba_ref(xin.to(dtype), sd, state_dtype)
    (out.to(keep) * w.to(keep)).sum().backward()
    grads = {k: v.grad for k, v in sd.items()}
    grads["x"] = xin.grad
    return out.detach(), grads


def _mamba_gpu_run(m, x, w, dtype):
    m = copy.deepcopy(m).to(DEV).train()
    xin = x.to(DEV, dtype).requires_grad_(True)
    out = m(xin)
    assert out.dtype == dtype and tuple(out.shape) == tuple(x.shape)
    (out.float() * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in m.named_parameters()}
    grads["x"] = xin.grad
    return out.detach(), grads


def test_mamba_128_states_f32_against_float64(f32_mode):
    m, x, w, ref, ref_g = _mamba_case()
    out, g = _mamba_gpu_run(m, x, w, torch.float32)
    e = _maxrel(out, ref)
    print(f"Mamba(32, d_state=128) f32: out {e:.2e}", {k: f"{_rel(g[k], ref_g[k]):.2e}" for k in ref_g})
    assert e <= 1e-4
    for k in ref_g:
        assert g[k] is not None, k
        assert _rel(g[k], ref_g[k]) <= 1e-3, k


def test_mamba_128_states_bf16_within_twice_the_cpu_bf16_error():
    hamspine.set_compute_dtype("bf16")
    m, x, w, ref, ref_g = _mamba_case()
    cpu_out, cpu_g = _mamba_ref_run(m, x, w, torch.bfloat16, torch.float32)
    out, g = _mamba_gpu_run(m, x, w, torch.bfloat16)
    _assert_within_twice_the_cpu_bf16_error("Mamba(32, d_state=128)", out, g, cpu_out, cpu_g, ref, ref_g)


# ------------------------------------------------------------------------------------------- len4mamba blocks
SMALL = dict(text_dim=24, img_dim=40, hidden_dim=56, proj_dim=32, num_heads=4)
_BLOCK_CASES = {          # name -> (class name, constructor arguments, B, P)
    "mamba-small": ("MultimodalMamba", {k: v for k, v in SMALL.items() if k != "num_heads"}, 2, 5),
    "kan-small": ("MultimodalMambaWithKANAttention", SMALL, 2, 5),
    "kan-256": ("MultimodalMambaWithKANAttention", dict(SMALL, proj_dim=256), 2, 49),
}
_INPUTS = ("text", "img", "first_hidden", "last_hidden")
_block_cache = {}


def _block_ref_run(name, m, ins, w, dtype, mamba_dtype=None, state_dtype=None):
    cls, kw, _, _ = _BLOCK_CASES[name]
    sd = _leaves(m.state_dict(), dtype)
    xin = [t.detach().clone().to(dtype).requires_grad_(True) for t in ins]      # fresh leaves: `ins` is shared between runs
    if cls == "MultimodalMamba":
        out = gr.multimodal_mamba_ref(*xin, sd, m.positional_encoding, mamba_dtype, state_dtype)
    else:
        out = gr.multimodal_mamba_kan_attention_ref(*xin, sd, m.positional_encoding, kw["num_heads"], mamba_dtype, state_dtype)
    (out * w.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in sd.items() if v.requires_grad}
    grads.update({n: t.grad for n, t in zip(_INPUTS, xin)})
    return out.detach(), grads


def _block_case(name):
    """seeded block + inputs + the float64 reference (output, parameter and input gradients), computed once per case"""
    if name in _block_cache:
        return _block_cache[name]
    import ConNexT.models.block.len4mamba as lm
    cls, kw, B, P = _BLOCK_CASES[name]
    torch.manual_seed(1700 + P + kw["proj_dim"])
    m = getattr(lm, cls)(**kw)
    with torch.no_grad():
        m.mamba.D.add_(0.3 * torch.randn_like(m.mamba.D))
        for n, p in m.named_parameters():      # LayerNorm away from (1, 0)
            if n.startswith("norm"):
                p.add_(0.2 * torch.randn_like(p))
    g = torch.Generator().manual_seed(1701)
    ins = (torch.randn(B, kw["text_dim"], generator=g), torch.randn(B, kw["img_dim"], P, generator=g),
           torch.randn(B, kw["hidden_dim"], generator=g), torch.randn(B, kw["hidden_dim"], generator=g))
    w = torch.randn(B, P + 3, kw["proj_dim"], generator=g)
    _block_cache[name] = (m, ins, w) + _block_ref_run(name, m, ins, w, torch.float64)
    return _block_cache[name]


def _block_gpu_run(m, ins, w):
    m = copy.deepcopy(m).to(DEV).train()
    xin = [t.to(DEV).requires_grad_(True) for t in ins]
    out = m(*xin)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(w.shape)
    (out * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in m.named_parameters()}
    grads.update({n: t.grad for n, t in zip(_INPUTS, xin)})
    return out.detach(), grads


@pytest.mark.parametrize("name", list(_BLOCK_CASES))
def test_len4mamba_block_f32_against_float64(name, f32_mode):
    m, ins, w, ref, ref_g = _block_case(name)
    out, g = _block_gpu_run(m, ins, w)
    assert sorted(ref_g) == sorted(g)
    e = _maxrel(out, ref)
    print(f"{name} f32: out {e:.2e}", {k: f"{_rel(g[k], ref_g[k]):.2e}" if g[k] is not None else "missing" for k in ref_g})
    assert e <= 1e-4
    for k in ref_g:
        assert g[k] is not None, k
        assert _rel(g[k], ref_g[k]) <= 1e-3, k


@pytest.mark.parametrize("name", ["mamba-small", "kan-small"])
def test_len4mamba_block_bf16_within_twice_the_cpu_bf16_error(name):
    hamspine.set_compute_dtype("bf16")
    m, ins, w, ref, ref_g = _block_case(name)
    # the module's policy: everything f32 except the Mamba block, which runs in bf16 with an f32 state
    cpu_out, cpu_g = _block_ref_run(name, m, ins, w, torch.float32, torch.bfloat16, torch.float32)
    out, g = _block_gpu_run(m, ins, w)
    _assert_within_twice_the_cpu_bf16_error(name, out, g, cpu_out, cpu_g, ref, ref_g)


def test_kan_attention_refuses_a_mask():
    from ConNexT.models.block.len4mamba import KANMultiheadAttention
    torch.manual_seed(1800)
    att = KANMultiheadAttention(32, num_heads=4).to(DEV)
    x = torch.randn(2, 8, 32, device=DEV)
    with pytest.raises(NotImplementedError):
        att(x, mask=torch.ones(2, 1, 8, 8, device=DEV))
    assert tuple(att(x).shape) == (2, 8, 32)


# ------------------------------------------------------------------------------------------------ argument checks
def test_unsupported_d_state_is_refused_without_a_launch():
    lib = L.lib()
    B, Lt, d = 1, 4, 64
    x = torch.zeros(B, Lt, d, device=DEV)
    bc = torch.zeros(B, Lt, 1024, device=DEV)
    par = torch.zeros(d, 512, device=DEV)
    out = torch.full((B, Lt, d), 7.0, device=DEV)
    p = rt.p
    for n_state in (24, 512):
        st = lib.hs_selective_scan_fwd(L.HS_F32, p(x), d, p(x), d, p(par), p(par), p(bc), p(bc, 4 * n_state), 1024, p(par), p(x), d,
                                       p(out), d, None, B, Lt, d, n_state, rt.stream())
        msg = lib.hs_last_error().decode()
        assert st == 3 and f"d_state {n_state}" in msg, (st, msg)          # HS_ERR_UNSUPPORTED
        assert lib.hs_selective_scan_chunk_len_n(n_state) < 0
    assert lib.hs_selective_scan_ws_bytes_n(B, Lt, d, 24) < 0
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))      # nothing ran


def test_misaligned_state_operands_are_refused_without_a_launch():
    """N > 16 reads A_log, Bm, Cm and hck as 16-byte vectors: a pointer 4 bytes off is status 3, not a launch"""
    lib = L.lib()
    B, Lt, d, N = 1, 4, 64, 32
    x = torch.zeros(B, Lt, d, device=DEV)
    bc = torch.zeros(B, Lt, 2 * N + 4, device=DEV)
    par = torch.zeros(d * N + 4, device=DEV)
    hck = torch.zeros(d * N + 4, device=DEV)
    out = torch.full((B, Lt, d), 7.0, device=DEV)
    p = rt.p

    def scan(n_state, a_off=0, b_off=0, c_off=0, h_off=0):
        st = lib.hs_selective_scan_fwd(L.HS_F32, p(x), d, p(x), d, p(par), p(par, a_off), p(bc, b_off), p(bc, 4 * n_state + c_off),
                                       2 * N + 4, p(par), p(x), d, p(out), d, p(hck, h_off), B, Lt, d, n_state, rt.stream())
        return st, lib.hs_last_error().decode()
    for off in (dict(a_off=4), dict(b_off=4), dict(c_off=4), dict(h_off=4)):
        st, msg = scan(N, **off)
        assert st == 3 and "16-byte aligned" in msg and f"d_state {N}" in msg, (off, st, msg)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))      # nothing ran
    assert scan(N)[0] == 0 and scan(16, a_off=4, b_off=4, c_off=4)[0] == 0      # aligned, and d_state 16 reads scalars
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out))


def test_positional_encoding_attribute_is_followed():
    """the device copy follows the plain attribute: reassigned -> the new table is added, None -> nothing is added"""
    from ConNexT.models.block.len4mamba import MultimodalMamba
    torch.manual_seed(1850)
    m = MultimodalMamba(text_dim=24, img_dim=40, hidden_dim=56, proj_dim=32).to(DEV)
    g = torch.Generator().manual_seed(1851)
    ins = [t.to(DEV) for t in (torch.randn(2, 24, generator=g), torch.randn(2, 40, 5, generator=g),
                               torch.randn(2, 56, generator=g), torch.randn(2, 56, generator=g))]
    with torch.no_grad():
        base = m._sequence(*ins)
        table = m.positional_encoding
        m.positional_encoding = 2 * table
        doubled = m._sequence(*ins)
        m.positional_encoding = None
        bare = m._sequence(*ins)
    torch.cuda.synchronize()
    pe = table[:, :8].to(DEV)
    scale = base.abs().max().item()
    assert (base - (bare + pe)).abs().max().item() <= 1e-6 * scale
    assert (doubled - (bare + 2 * pe)).abs().max().item() <= 1e-6 * scale


# ------------------------------------------------------------------------------------------------ training
def test_kan_attention_block_trains(f32_mode):
    from ConNexT.models.block.len4mamba import MultimodalMambaWithKANAttention
    from hamspine import functional as F
    from hamspine.nn.layers import Linear
    from hamspine.optim import FusedAdamW
    torch.manual_seed(1900)
    blk = MultimodalMambaWithKANAttention(**SMALL).to(DEV).train()
    head = Linear(SMALL["proj_dim"], 3).to(DEV).train()
    g = torch.Generator().manual_seed(1901)
    B, P = 2, 5
    ins = [t.to(DEV) for t in (torch.randn(B, 24, generator=g), torch.randn(B, 40, P, generator=g),
                               torch.randn(B, 56, generator=g), torch.randn(B, 56, generator=g))]
    labels = torch.tensor([0, 2], device=DEV)
    opt = FusedAdamW(list(blk.parameters()) + list(head.parameters()), lr=1e-3, weight_decay=0.01)
    losses = []
    for step in range(5):
        opt.zero_grad()
        loss = F.cross_entropy(head(F.mean_tokens(blk(*ins), out_f32=True)), labels)
        loss.backward()
        if step == 0:
            for prm in (blk.mamba.A_log, blk.attn.q_proj.layers[0].spline_weight, blk.proj_img.weight):
                assert prm.grad is not None and torch.isfinite(prm.grad).all() and prm.grad.abs().max().item() > 0
        opt.step()
        losses.append(loss.item())
    print("losses", losses)
    assert all(l == l and abs(l) < float("inf") for l in losses)
    assert losses[-1] < losses[0]
