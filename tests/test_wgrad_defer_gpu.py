"""Deferred head-path weight gradients (HAMSPINE_WGRAD_DEFER, hs_wgrad_defer_* in csrc/blocks.hip, plumbing in hamspine/rt.py).

With the switch on, LinearFn / MHAFn / MlpGeluFn launch only their data-gradient GEMMs where autograd runs them; the weight and
bias gradients wait in a per-stream set and run as one grouped split-K grid plus one multi-problem column-sum pair at the next
whole-tower backward or at the end of the backward pass.  Every problem keeps the tile, the split, the slab reduction and the
column-sum chunking of its own launch, so every case compares HAMSPINE_WGRAD_DEFER=1 against =0 BIT FOR BIT (outputs, dx, every
parameter gradient, the loss), each setting run twice.  The counters in hamspine.rt say which path ran."""
import os

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from hamspine import _lib as L  # noqa: E402
from hamspine import functional as F  # noqa: E402
from hamspine import rt  # noqa: E402
from hamspine.nn import Linear, MultiheadAttention  # noqa: E402
from hamspine.nn.layers import MLPHead  # noqa: E402
from modules.fusion_blocks import FusionModule  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
SWITCH = "HAMSPINE_WGRAD_DEFER"


@pytest.fixture(autouse=True)
def _restore():
    os.environ.pop(SWITCH, None)
    yield
    os.environ.pop(SWITCH, None)
    os.environ.pop("HAMSPINE_DDP_SINGLE", None)
    assert not rt.wgrad_defer_open()


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, f"{what}: {k} changed shape or dtype"
        assert torch.equal(_bits(a[k]), _bits(b[k])), \
            f"{what}: {k} differs by {(a[k].float() - b[k].float()).abs().max().item():.3e}"


def _counters():
    torch.cuda.synchronize()
    return rt.wgrad_defer_counters()


def _delta(before):
    now = _counters()
    return {k: now[k] - before[k] for k in now}


def _ab(run):
    """run() -> {name: tensor}: the default (on), "1" and "0", each twice, interleaved; -> (result, counter deltas of one "1" run)"""
    res, delta = {}, None
    for rep in (0, 1):
        for setting in ("1", "0", None):
            if setting is None:
                os.environ.pop(SWITCH, None)
            else:
                os.environ[SWITCH] = setting
            c0 = _counters()
            res[setting, rep] = run()
            d = _delta(c0)
            assert not rt.wgrad_defer_open()
            if setting == "0":
                assert d["deferred"] == 0 and d["flushed"] == 0 and d["grouped_launches"] == 0, d
            else:
                assert d["deferred"] == d["flushed"], d
            if setting == "1":
                delta = d
    os.environ.pop(SWITCH, None)
    for setting in ("1", None):
        _assert_same(res[setting, 0], res["0", 0], f"{SWITCH}={setting} vs 0")
    for setting in ("1", "0", None):
        _assert_same(res[setting, 1], res[setting, 0], f"{SWITCH}={setting}, second run")
    return res["1", 0], delta


def _grads(mod):
    return {"grad." + k: p.grad.detach().clone() for k, p in mod.named_parameters() if p.grad is not None}


def _run_module(mod, inputs, call=None, seed=11):
    """one forward + backward of mod on fresh leaf copies of `inputs` (dict; float ones get a gradient)"""
    mod.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    rt.reset_seed(seed)
    leaves = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in inputs.items()}
    y = call(mod, **leaves) if call else mod(**leaves)
    w = torch.linspace(-1.0, 1.0, y.numel(), device=y.device).view(y.shape)
    loss = (y.float() * w).sum()
    loss.backward()
    out = {"y": y.detach().clone(), "loss": loss.detach().clone()}
    for k, v in leaves.items():
        if v.is_floating_point():
            assert v.grad is not None
            out["d" + k] = v.grad.detach().clone()
    out.update(_grads(mod))
    assert all(p.grad is not None for p in mod.parameters())
    return out


def _linear(in_f, out_f, bias, dtype, seed=3):
    torch.manual_seed(seed)
    return Linear(in_f, out_f, bias=bias).to(DEV).train(), dtype


def _x(M, in_f, dtype, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, in_f, generator=g).to(DEV).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# LinearFn
# ---------------------------------------------------------------------------------------------------------------------------
def test_linear_bf16_split():
    M, in_f, out_f = 1568, 256, 256
    assert L.lib().hs_gemm_suggest_split(out_f, in_f, M, L.HS_BF16) > 1          # the split-K + separate column-sum branch
    lin, _ = _linear(in_f, out_f, True, BF)
    x = _x(M, in_f, BF)
    _, d = _ab(lambda: _run_module(lin, {"x": x}))
    assert d["deferred"] == 1 and d["grouped_launches"] == 1 and d["colsum_launches"] == 2, d


@pytest.mark.parametrize("bias", [True, False])
def test_linear_bf16_unsplit(bias):
    M, in_f, out_f = 96, 64, 72
    assert L.lib().hs_gemm_suggest_split(out_f, in_f, M, L.HS_BF16) <= 1         # the bias gradient rides in the GEMM as row sums
    lin, _ = _linear(in_f, out_f, bias, BF)
    x = _x(M, in_f, BF)
    _, d = _ab(lambda: _run_module(lin, {"x": x}))
    assert d["deferred"] == 1 and d["grouped_launches"] == 1 and d["colsum_launches"] == 0, d


@pytest.mark.parametrize("out_f", [7, 256])
def test_linear_f32_head(out_f):
    M, in_f = 32, 256
    lin, _ = _linear(in_f, out_f, True, torch.float32)
    x = _x(M, in_f, torch.float32)
    _, d = _ab(lambda: _run_module(lin, {"x": x}))
    # 32 rows are one row group: the partial launch writes the bias gradient itself, as hs_colsum does
    assert d["deferred"] == 1 and d["grouped_launches"] == 0 and d["colsum_launches"] == 1, d


# ---------------------------------------------------------------------------------------------------------------------------
# MHAFn
# ---------------------------------------------------------------------------------------------------------------------------
def test_mha_packed_self_attention():
    torch.manual_seed(7)
    mha = MultiheadAttention(256, 8, dropout=0.1, batch_first=True).to(DEV).train()
    x = torch.randn(2, 49, 256, generator=torch.Generator().manual_seed(8)).to(DEV).to(BF)
    _, d = _ab(lambda: _run_module(mha, {"query": x}, call=lambda m, query: m.attend(query, residual=query)))
    assert d["deferred"] == 2 and d["grouped_launches"] == 1, d


def test_mha_split_cross_attention_ragged():
    torch.manual_seed(9)
    mha = MultiheadAttention(256, 8, dropout=0.1, batch_first=True, kdim=768, vdim=768).to(DEV).train()
    g = torch.Generator().manual_seed(10)
    q = torch.randn(2, 49, 256, generator=g).to(DEV).to(BF)
    k = torch.randn(2, 16, 768, generator=g).to(DEV).to(BF)
    valid = torch.ones(2, 16, dtype=torch.int64)
    valid[1, 5:] = 0
    assert bool(valid[0].all()) and 0 < int(valid[1].sum()) < 16                  # one full row, one short row
    valid = valid.to(DEV)
    _, d = _ab(lambda: _run_module(mha, {"query": q, "key": k},
                                   call=lambda m, query, key: m.attend(query, key=key, valid_mask=valid, residual=query)))
    assert d["deferred"] == 4 and d["grouped_launches"] == 1, d


# ---------------------------------------------------------------------------------------------------------------------------
# fusion block + head + loss, end to end
# ---------------------------------------------------------------------------------------------------------------------------
class _FusionHead(nn.Module):
    def __init__(self):
        super().__init__()
        self.fusion = FusionModule(768, 256, num_heads=8, dropout=0.1)
        self.head = MLPHead(256, 256, 7, 0.1)

    def forward(self, img, txt, mask, labels):
        logits = self.head(self.fusion(img, txt, mask))
        return logits, F.cross_entropy(logits, labels, label_smoothing=0.02)


def _fusion_case():
    torch.manual_seed(21)
    m = _FusionHead().to(DEV).train()
    g = torch.Generator().manual_seed(22)
    img = torch.randn(2, 49, 256, generator=g).to(DEV).to(BF)
    txt = torch.randn(2, 16, 768, generator=g).to(DEV).to(BF)
    mask = torch.ones(2, 16, dtype=torch.int64)
    mask[1, 9:] = 0
    labels = torch.tensor([1, 5], device=DEV)
    return m, img, txt, mask.to(DEV), labels


def _run_fusion(m, img, txt, mask, labels, backward=None):
    m.zero_grad(set_to_none=True)
    torch.manual_seed(23)
    rt.reset_seed(23)
    img = img.detach().clone().requires_grad_(True)
    txt = txt.detach().clone().requires_grad_(True)
    logits, loss = m(img, txt, mask, labels)
    (backward or (lambda l: l.backward()))(loss)
    out = {"logits": logits.detach().clone(), "loss": loss.detach().clone(), "dimg": img.grad.detach().clone(),
           "dtxt": txt.grad.detach().clone()}
    out.update(_grads(m))
    assert all(p.grad is not None for p in m.parameters())
    return out


def test_fusion_head_end_to_end_and_launch_counts():
    m, img, txt, mask, labels = _fusion_case()
    _, d = _ab(lambda: _run_fusion(m, img, txt, mask, labels))
    # 2 + 4 attention projections, the feed-forward pair, the head pair; no tower executor: one flush at the end of backward
    assert d["deferred"] == 10 and d["flushed"] == 10, d
    # ONE grouped grid for the eight bf16 weight gradients.  Column sums: at these 98 / 32 / 2 rows every bf16 weight gradient
    # is unsplit and carries its bias gradient as row sums, so the table holds the two f32 head layers alone -- 2 rows, one row
    # group, whose partial launch writes the result itself (hs_colsum's single-launch form, kept per problem): one launch, no
    # final.  A problem with more than one row group brings the second launch (test_linear_bf16_split asserts the two).
    split = [L.lib().hs_gemm_suggest_split(o, i, r, L.HS_BF16) for (o, i, r) in
             ((256, 256, 98), (768, 256, 98), (256, 768, 32), (1024, 256, 98), (256, 1024, 98))]
    assert d["grouped_launches"] == 1, d
    assert d["colsum_launches"] == (1 if max(split) <= 1 else 2), (d, split)


def test_two_backwards_in_a_row_leave_no_set():
    m, img, txt, mask, labels = _fusion_case()
    a = _run_fusion(m, img, txt, mask, labels)
    assert not rt.wgrad_defer_open()
    b = _run_fusion(m, img, txt, mask, labels)
    assert not rt.wgrad_defer_open()
    _assert_same(a, b, "second backward")


# ---------------------------------------------------------------------------------------------------------------------------
# a full set: the 65th layer takes the immediate path
# ---------------------------------------------------------------------------------------------------------------------------
def test_sixty_five_layers():
    torch.manual_seed(31)
    layers = nn.ModuleList([Linear(64, 64) for _ in range(65)]).to(DEV).train()
    x = _x(96, 64, BF, seed=32)

    def call(mod, x):
        for l in mod:
            x = l(x, residual=x)
        return x

    _, d = _ab(lambda: _run_module(layers, {"x": x}, call=call))
    assert d["deferred"] == 64 and d["flushed"] == 64, d


# ---------------------------------------------------------------------------------------------------------------------------
# fallbacks
# ---------------------------------------------------------------------------------------------------------------------------
def test_existing_grad_accumulates_immediately():
    lin, _ = _linear(256, 256, True, BF)
    x = _x(1568, 256, BF)
    os.environ[SWITCH] = "0"
    one = _run_module(lin, {"x": x})
    os.environ.pop(SWITCH)
    _run_module(lin, {"x": x})
    c0 = _counters()
    y = lin(x)                                          # second backward onto the existing .grad
    w = torch.linspace(-1.0, 1.0, y.numel(), device=DEV).view(y.shape)
    (y.float() * w).sum().backward()
    assert _delta(c0)["deferred"] == 0
    for k, p in lin.named_parameters():
        ref = one["grad." + k]
        assert torch.equal(_bits(p.grad), _bits(ref + ref)), k


def test_hooked_parameter_is_not_deferred():
    lin, _ = _linear(256, 256, True, BF)
    x = _x(1568, 256, BF)
    os.environ[SWITCH] = "0"
    ref = _run_module(lin, {"x": x})
    os.environ.pop(SWITCH)
    seen = {}
    h = lin.weight.register_hook(lambda g: seen.__setitem__("w", g.detach().clone()))
    c0 = _counters()
    got = _run_module(lin, {"x": x})
    h.remove()
    assert _delta(c0)["deferred"] == 0
    _assert_same(got, ref, "hooked parameter")
    assert torch.equal(_bits(seen["w"]), _bits(ref["grad.weight"]))          # the hook saw the finished gradient
    h2 = lin.bias.register_post_accumulate_grad_hook(lambda p: seen.__setitem__("b", p.grad.detach().clone()))
    c0 = _counters()
    got = _run_module(lin, {"x": x})
    h2.remove()
    assert _delta(c0)["deferred"] == 0
    assert torch.equal(_bits(seen["b"]), _bits(ref["grad.bias"]))


def test_data_parallel_defers_nothing():
    import torch.distributed as dist
    from hamspine.ddp import DataParallel
    m, img, txt, mask, labels = _fusion_case()
    os.environ[SWITCH] = "0"
    ref = _run_fusion(m, img, txt, mask, labels)
    os.environ.pop(SWITCH)
    os.environ["HAMSPINE_DDP_SINGLE"] = "1"
    made = not dist.is_initialized()
    ifname = os.environ.get("GLOO_SOCKET_IFNAME")
    if made:                                            # a group of one rank in this process, over the loopback interface
        os.environ["GLOO_SOCKET_IFNAME"] = "lo"
        dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    ddp = None
    try:
        ddp = DataParallel(m)
        assert ddp.collective
        c0 = _counters()
        got = _run_fusion(ddp, img, txt, mask, labels)
        ddp.finish()
        torch.cuda.synchronize()
        assert _delta(c0)["deferred"] == 0
        assert torch.equal(_bits(got["loss"]), _bits(ref["loss"]))
        for k, p in m.named_parameters():
            assert torch.equal(_bits(p.grad), _bits(ref["grad." + k])), k
    finally:
        if ddp is not None:
            ddp.detach()
        if made:
            dist.destroy_process_group()
            if ifname is None:
                os.environ.pop("GLOO_SOCKET_IFNAME", None)
            else:
                os.environ["GLOO_SOCKET_IFNAME"] = ifname


def test_autograd_grad_returns_filled_tensors():
    m, img, txt, mask, labels = _fusion_case()
    os.environ[SWITCH] = "0"
    ref = _run_fusion(m, img, txt, mask, labels)
    os.environ.pop(SWITCH)
    m.zero_grad(set_to_none=True)
    torch.manual_seed(23)
    rt.reset_seed(23)
    _, loss = m(img, txt, mask, labels)
    names, params = zip(*m.named_parameters())
    c0 = _counters()
    grads = torch.autograd.grad(loss, params)
    d = _delta(c0)
    assert d["deferred"] == 10 and d["flushed"] == 10 and not rt.wgrad_defer_open(), d
    for k, g in zip(names, grads):
        assert torch.equal(_bits(g), _bits(ref["grad." + k])), k


class _Boom(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError("boom")


def test_exception_in_backward_leaves_no_set():
    torch.manual_seed(41)
    a, b = Linear(64, 64).to(DEV).train(), Linear(64, 64).to(DEV).train()
    x = _x(96, 64, BF, seed=42).requires_grad_(True)
    c0 = _counters()
    y = b(_Boom.apply(a(x)))                       # backward: b defers, then the node in the middle raises
    with pytest.raises(RuntimeError, match="boom"):
        y.float().sum().backward()
    d = _delta(c0)
    assert d["deferred"] == 1 and d["flushed"] == 0, d
    assert not rt.wgrad_defer_open()
    assert L.lib().hs_wgrad_defer_open(rt.stream()) == 0 and L.lib().hs_wgrad_defer_pending(rt.stream()) == 0
    # and the next backward is whole
    lin, _ = _linear(256, 256, True, BF)
    xx = _x(1568, 256, BF)
    os.environ[SWITCH] = "0"
    ref = _run_module(lin, {"x": xx})
    os.environ.pop(SWITCH)
    _assert_same(_run_module(lin, {"x": xx}), ref, "backward after a failed one")
