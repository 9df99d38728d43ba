"""Fused bf16 attention at head dim 64 beyond 128 keys: the forward up to 512 keys (64-row query chunks past 256 keys) and
the key-blocked backward for 129..512 keys (csrc/attn_fused.hip).  The lengths are the reference loaders' own: the MIBF-Net
loader pads captions to 256 tokens, the ConNeXT loader to the longest caption of the batch, up to BERT's 512 positions.

Bounds are those of test_fused_attention_general_shapes_match_reference: max error <= 2e-2 * max|ref| on the output and
3e-2 on the gradients, against f32 torch attention on the same bf16-rounded q, k, v.  A CPU emulation of a correct bf16
kernel (bf16 storage of P, O and dS, f32 accumulation) stays at least 4.7x under them on these shapes."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from oracle import towers  # noqa: E402
from oracle.procedural import load_procedural  # noqa: E402

DEV = "cuda"

LONG_SHAPES = [
    (12, 64, 256, 256, True),    # BERT-base heads at the MIBF loader's padding
    (4, 64, 130, 200, True),     # ragged in both directions
    (4, 64, 384, 384, True),     # three key blocks
    (12, 64, 512, 512, True),    # BERT's full position table
    (2, 64, 64, 512, False),     # fewer queries than a chunk
    (4, 64, 600, 300, False),    # more queries than keys, ragged last chunk
]


@pytest.fixture(autouse=True)
def _bf16_mode():
    hamspine.set_compute_dtype("bf16")
    yield
    hamspine.set_compute_dtype("bf16")


def _close(a, b, what, rtol, atol=2e-6):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    print(f"{what}: max err {err:.3e} = {err / scale:.3e} x max|ref|")
    assert err <= rtol * scale + atol, f"{what}: max err {err:.3e} (scale {scale:.3e}, rtol {rtol})"


def _inputs(H, hd, Lq, Lk, masked, B=3):
    g = torch.Generator().manual_seed(Lq * 1000 + Lk)
    q = torch.randn(B, Lq, H * hd, generator=g).bfloat16()
    k, v = (torch.randn(B, Lk, H * hd, generator=g).bfloat16() for _ in range(2))
    cot = torch.randn(B, Lq, H * hd, generator=g).bfloat16().float()
    mask = None
    if masked:
        mask = torch.ones(B, Lk, dtype=torch.long)
        mask[0, Lk // 2:] = 0
        mask[2, 5:] = 0
    return q, k, v, cot, mask


class _GemmLaunches:
    """GEMM launches recorded by the GEMM core's profile hook (the score / context products of the unfused path)."""

    def __init__(self):
        from hamspine import _lib as L
        self.lib = L.lib()
        self.lib.hs_prof_enable.argtypes = [C.c_int32]
        self.lib.hs_prof_collect.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]

    def __enter__(self):
        torch.cuda.synchronize()
        self.lib.hs_prof_enable(1)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        fl, ms, cnt = (C.c_double * 4)(), (C.c_double * 4)(), (C.c_int64 * 4)()
        self.lib.hs_prof_collect(fl, ms, cnt)
        self.lib.hs_prof_enable(0)
        self.count = sum(cnt)
        return False


def _run(q, k, v, cot, mask, H, sc, dropout_p=0.0):
    from hamspine import convnext_ops as X
    qp, kp, vp = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    with _GemmLaunches() as fwd:
        out = X.attention_core(qp, kp, vp, heads=H, scale=sc, key_mask=None if mask is None else mask.to(DEV),
                               dropout_p=dropout_p)
    with _GemmLaunches() as bwd:
        (out.float() * cot.to(DEV)).sum().backward()
    return out.detach(), qp.grad, kp.grad, vp.grad, fwd.count, bwd.count


def _reference(q, k, v, cot, mask, H, hd):
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    sc = hd ** -0.5
    s = qr.view(B, Lq, H, hd).transpose(1, 2) @ kr.view(B, Lk, H, hd).transpose(1, 2).transpose(-1, -2) * sc
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :] == 0, -3.0e38)
    ref = (torch.softmax(s, -1) @ vr.view(B, Lk, H, hd).transpose(1, 2)).transpose(1, 2).reshape(B, Lq, H * hd)
    (ref * cot).sum().backward()
    return ref.detach(), qr.grad, kr.grad, vr.grad


def _check_values(H, hd, Lq, Lk, masked, out, dq, dk, dv):
    q, k, v, cot, mask = _inputs(H, hd, Lq, Lk, masked)
    ref, rq, rk, rv = _reference(q, k, v, cot, mask, H, hd)
    tag = f"H={H} hd={hd} Lq={Lq} Lk={Lk} masked={masked}"
    _close(out, ref, f"{tag} out", 2e-2)
    _close(dq, rq, f"{tag} dq", 3e-2)
    _close(dk, rk, f"{tag} dk", 3e-2)
    _close(dv, rv, f"{tag} dv", 3e-2)


@pytest.mark.parametrize("H,hd,Lq,Lk,masked", LONG_SHAPES)
def test_long_key_attention_launches_no_gemms(H, hd, Lq, Lk, masked):
    """Forward and backward of these shapes run the fused kernels: no score / context GEMM and no softmax pass."""
    q, k, v, cot, mask = _inputs(H, hd, Lq, Lk, masked)
    *_, n_fwd, n_bwd = _run(q, k, v, cot, mask, H, hd ** -0.5)
    print(f"GEMM launches: forward {n_fwd}, backward {n_bwd}")
    assert n_fwd == 0, f"forward launched {n_fwd} GEMMs: the fused kernel should cover Lk={Lk}"
    assert n_bwd == 0, f"backward launched {n_bwd} GEMMs: the fused kernel should cover Lk={Lk}"


@pytest.mark.parametrize("H,hd,Lq,Lk,masked", LONG_SHAPES)
def test_long_key_attention_matches_reference(H, hd, Lq, Lk, masked):
    q, k, v, cot, mask = _inputs(H, hd, Lq, Lk, masked)
    out, dq, dk, dv, _, _ = _run(q, k, v, cot, mask, H, hd ** -0.5)
    _check_values(H, hd, Lq, Lk, masked, out, dq, dk, dv)


@pytest.mark.parametrize("H,hd,Lq,Lk,masked", [(8, 32, 64, 200, True), (4, 64, 130, 600, True)])
def test_shapes_past_the_fused_range_keep_the_fallback(H, hd, Lq, Lk, masked):
    """Head dim 32 beyond 128 keys and head dim 64 beyond 512 keys stay on the GEMM + softmax path, with correct values."""
    q, k, v, cot, mask = _inputs(H, hd, Lq, Lk, masked)
    out, dq, dk, dv, n_fwd, n_bwd = _run(q, k, v, cot, mask, H, hd ** -0.5)
    _check_values(H, hd, Lq, Lk, masked, out, dq, dk, dv)
    print(f"GEMM launches: forward {n_fwd}, backward {n_bwd}")
    assert n_fwd > 0 and n_bwd > 0, (n_fwd, n_bwd)


@pytest.mark.parametrize("L", [384, 512])
def test_long_key_dropout_mask_is_the_same_in_forward_and_backward(L):
    """With V = 1 the output is the row sum of the dropped-out probabilities Pd, and with dO = 1 the gradient dV is its
    column sum: both total sum(Pd), so the forward and the key-blocked backward regenerated the same mask."""
    from hamspine import convnext_ops as X
    hd = 64
    B, H, p = 4, 4, 0.25
    g = torch.Generator().manual_seed(L)
    q, k = (torch.randn(B, L, H * hd, generator=g).bfloat16().to(DEV) for _ in range(2))
    v = torch.ones(B, L, H * hd, dtype=torch.bfloat16, device=DEV).requires_grad_(True)
    out = X.attention_core(q, k, v, heads=H, scale=hd ** -0.5, dropout_p=p)
    out.float().sum().backward()
    fwd_total = out.float()[:, :, ::hd].sum().item()          # one column per head: sum over rows of Pd
    bwd_total = v.grad.float()[:, :, ::hd].sum().item()       # sum over columns of Pd
    print(f"L={L}: forward total {fwd_total:.6g}, backward total {bwd_total:.6g}, rows {B * H * L}")
    assert abs(fwd_total - bwd_total) <= 5e-3 * abs(fwd_total), (fwd_total, bwd_total)
    assert abs(fwd_total / (B * H * L) - 1.0) < 0.05
    o2 = X.attention_core(q, k, v.detach(), heads=H, scale=hd ** -0.5, dropout_p=p)
    assert not torch.equal(o2, out.detach())                   # a new call draws a new mask


def test_long_key_attention_is_bitwise_repeatable():
    """Same seed, same inputs: forward and backward at 512 x 512 with attention dropout give identical bits (dQ is summed
    over the key blocks in a fixed order, no atomics)."""
    from hamspine import rt
    H, hd, L = 12, 64, 512
    q, k, v, cot, mask = _inputs(H, hd, L, L, True)
    runs = []
    for _ in range(2):
        rt.reset_seed(4321)
        out, dq, dk, dv, _, _ = _run(q, k, v, cot, mask, H, hd ** -0.5, dropout_p=0.1)
        runs.append((out, dq, dk, dv))
    rt.reset_seed(None)
    for name, a, b in zip(("out", "dq", "dk", "dv"), *runs):
        assert torch.equal(a, b), f"{name} differs between two identical runs"


def _bert_pair(cfg, seed):
    from hamspine.nn import BertConfig, BertModel
    o = load_procedural(towers.OBertModel(**cfg), seed)
    p = BertModel(BertConfig(**cfg))
    p.load_state_dict(o.state_dict(), strict=False)
    return p.to(DEV), o


_BERT_CFG = dict(vocab_size=90, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                 max_position_embeddings=512, type_vocab_size=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


@pytest.mark.parametrize("L", [384, 512])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_bert_at_the_loaders_lengths(L, mode):
    """Tiny BERT (2 heads of 64) at the ConNeXT loader's lengths against the oracle, with ragged masks: a row with one
    valid token, a half row, all but the last, a full row.  Padded positions are left out of the comparison."""
    hamspine.set_compute_dtype(mode)
    p, o = _bert_pair(_BERT_CFG, 31)
    p.train()
    o.train()
    g = torch.Generator().manual_seed(L)
    B = 4
    ids = torch.randint(1, 90, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, 1:] = 0
    mask[2, (L + 1) // 2:] = 0
    mask[3, L - 1:] = 0
    ids = ids * mask
    cot = torch.randn(B, L, 128, generator=g) * mask[..., None]
    ho = o(ids, mask)
    (ho * cot).sum().backward()
    hp = p(input_ids=ids.to(DEV), attention_mask=mask.to(DEV)).last_hidden_state
    (hp.float() * cot.to(DEV)).sum().backward()
    valid = mask.bool()
    tol_out, tol_grad = (1e-4, 2e-3) if mode == "f32" else (3e-2, 6e-2)
    err = (hp.float().cpu()[valid] - ho[valid]).abs().max().item()
    print(f"L={L} {mode}: hidden err {err:.3e} (max|ref| {ho[valid].abs().max().item():.3e})")
    assert err <= tol_out * ho[valid].abs().max().item() + 1e-5, f"L={L} {mode}: hidden err {err:.3e}"
    op = dict(o.named_parameters())
    bad = []
    for k, prm in p.named_parameters():
        if "pooler" in k or prm.grad is None or k.endswith("attention.self.key.bias"):
            continue      # the key bias shifts every score of a row equally: its gradient is analytically zero (rounding noise)
        e = _rel(prm.grad, op[k].grad)
        if e > tol_grad:
            bad.append(f"{k}: {e:.3e}")
    assert not bad, f"L={L} {mode}: gradients off: {bad}"


def test_bert_train_step_with_attention_dropout_at_512():
    """bf16 train mode with attention dropout 0.1 at 512 tokens: finite loss, finite and nonzero gradients."""
    cfg = dict(_BERT_CFG, attention_probs_dropout_prob=0.1)
    p, _ = _bert_pair(cfg, 32)
    p.train()
    g = torch.Generator().manual_seed(5)
    B, L = 2, 512
    ids = torch.randint(1, 90, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, 300:] = 0
    cot = torch.randn(B, L, 128, generator=g)
    hp = p(input_ids=ids.to(DEV), attention_mask=mask.to(DEV)).last_hidden_state
    loss = (hp.float() * cot.to(DEV)).sum()
    loss.backward()
    assert torch.isfinite(loss).item(), loss.item()
    for k, prm in p.named_parameters():
        if "pooler" in k or prm.grad is None or k.endswith("attention.self.key.bias"):
            continue
        assert torch.isfinite(prm.grad).all().item(), f"{k}: non-finite gradient"
        assert prm.grad.abs().max().item() > 0, f"{k}: zero gradient"
