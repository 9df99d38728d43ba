"""Global gradient-norm clipping, host side: the float64 yardstick of tests/gradclip_ref.py against
torch.nn.utils.clip_grad_norm_ followed by torch.optim in float64, the declarations of the new entry points, and the refusals
of hamspine.optim that need no device.  No GPU."""
import re

import numpy as np
import pytest
import torch

import gradclip_ref as gr
from kernel_ref import gen

import hamspine._lib as L  # noqa: E402

F64 = torch.float64
MAX_NORM = 0.75


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _state(seed, target):
    """two parameters (257 and 31 elements) and three steps of float64 gradients whose global norm is `target` (None: all zero)"""
    g = gen(seed)
    ps = [4.0 * torch.rand(n, generator=g, dtype=F64) - 2.0 for n in (257, 31)]
    steps = []
    for _ in range(3):
        gs = [torch.randn(p.numel(), generator=g, dtype=F64) for p in ps]
        if target is None:
            gs = [torch.zeros_like(x) for x in gs]
        else:
            k = target / gr.norm64(gs)
            gs = [x * k for x in gs]
        steps.append(gs)
    return ps, steps


# norms below, at (within float64 rounding of) and above max_norm, and all-zero gradients
TARGETS = {"below": 0.4 * MAX_NORM, "at": MAX_NORM, "above": 7.0 * MAX_NORM, "zero": None}


def _torch_side(ps, make_opt):
    tps = [p.clone().requires_grad_(True) for p in ps]
    return tps, make_opt(tps)


def _clip_torch(tps, gs):
    for tp, g in zip(tps, gs):
        tp.grad = g.clone()
    return float(torch.nn.utils.clip_grad_norm_(tps, MAX_NORM))


@pytest.mark.parametrize("case", list(TARGETS))
@pytest.mark.parametrize("decoupled", (0, 1))
def test_yardstick_is_torch_clip_then_adam_in_float64(decoupled, case):
    ps, steps = _state(11, TARGETS[case])
    lr, b1, b2, eps, wd = 1e-2, 0.9, 0.999, 1e-8, 0.05
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    tps, opt = _torch_side(ps, lambda t: cls(t, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd))
    cur = [{"p": p, "m": torch.zeros_like(p), "v": torch.zeros_like(p)} for p in ps]
    for k, gs in enumerate(steps):
        tnorm = _clip_torch(tps, gs)
        opt.step()
        norm = gr.norm64(gs)
        c = gr.coef(norm, MAX_NORM, np.float64)
        assert abs(norm - tnorm) <= 1e-12 * tnorm
        assert (c < 1.0) == (case in ("at", "above")) and (case != "zero" or (norm == 0.0 and c == 1.0))
        for i, (tp, g) in enumerate(zip(tps, gs)):
            r = gr.adam_clip_ref64(cur[i]["p"], g, cur[i]["m"], cur[i]["v"], lr, b1, b2, eps, wd, k + 1, decoupled, 1.0, c)
            cur[i] = {kk: torch.from_numpy(r[kk]) for kk in ("p", "m", "v")}
            st = opt.state[tp]
            assert _rel(cur[i]["p"], tp.detach()) <= 1e-12, (case, k, i)
            assert _rel(cur[i]["m"], st["exp_avg"]) <= 1e-12 and _rel(cur[i]["v"], st["exp_avg_sq"]) <= 1e-12, (case, k, i)
            if case == "zero" and decoupled:          # (Adam's L2 decay adds wd p to a zero gradient; AdamW's does not)
                assert not cur[i]["m"].any() and not st["exp_avg"].any() and not cur[i]["v"].any()


@pytest.mark.parametrize("case", list(TARGETS))
@pytest.mark.parametrize("momentum,nesterov", ((0.0, 0), (0.9, 0), (0.9, 1)))
def test_yardstick_is_torch_clip_then_sgd_in_float64(momentum, nesterov, case):
    ps, steps = _state(12, TARGETS[case])
    lr, wd = 0.05, 1e-2
    tps, opt = _torch_side(ps, lambda t: torch.optim.SGD(t, lr=lr, momentum=momentum, weight_decay=wd, nesterov=bool(nesterov)))
    cur = [{"p": p, "buf": None} for p in ps]
    for k, gs in enumerate(steps):
        _clip_torch(tps, gs)
        opt.step()
        c = gr.coef(gr.norm64(gs), MAX_NORM, np.float64)
        for i, (tp, g) in enumerate(zip(tps, gs)):
            r = gr.sgd_clip_ref64(cur[i]["p"], g, cur[i]["buf"], lr, momentum, wd, nesterov, 1 if k == 0 else 0, 1.0, c)
            cur[i] = {"p": torch.from_numpy(r["p"]), "buf": None if r["buf"] is None else torch.from_numpy(r["buf"])}
            assert _rel(cur[i]["p"], tp.detach()) <= 1e-12, (case, k, i)
            if momentum:
                assert _rel(cur[i]["buf"], opt.state[tp]["momentum_buffer"]) <= 1e-12, (case, k, i)


def test_float32_forms_of_the_yardstick():
    """the record: one rounding of the float64 norm, the stated float32 coefficient, the flags; and the float32 step forms
    multiply in the kernel's order, within a few float32 roundings of the float64 form"""
    f = np.float32
    assert gr.coef(f(0.0), 1.0) == f(1.0) and gr.coef(f(2.0), np.inf) == f(1.0)
    assert gr.coef(f(np.inf), 1.0) == f(0.0) and np.isnan(gr.coef(f(np.nan), 1.0)) and np.isnan(gr.coef(f(np.inf), np.inf))
    assert gr.coef(f(4.0), 1.0) == f(1.0) / (f(4.0) + f(1e-6)) and gr.coef(f(4.0), 1.0).dtype == np.float32
    g = gen(13)
    gs = [torch.randn(n, generator=g) for n in (5, 0, 1029)]
    rec = gr.record(gs, 0.5)
    want = np.sqrt(sum(float((x.double() ** 2).sum()) for x in gs))
    assert rec.dtype == np.float32 and rec[0] == f(want) and rec[1] == gr.coef(rec[0], 0.5) and rec[2] == 1 and rec[3] == 0
    big = [torch.tensor([1e20, 3.0])]
    assert np.isfinite(gr.record(big, 1.0)[0]) and gr.record(big, 1.0)[0] == f(1e20)
    over = [torch.full((4,), 3e38)]             # float64 norm 6e38 > float32 max
    assert list(gr.record(over, 1.0)) == [np.inf, 0.0, 0.0, 0.0] and list(gr.record(over, 1.0, True))[2:] == [0.0, 1.0]
    nan = gr.record([torch.tensor([1.0, float("nan")])], 1.0, True)
    assert np.isnan(nan[0]) and np.isnan(nan[1]) and nan[2] == 0 and nan[3] == 1
    p, gg, m, v = (torch.randn(64, generator=g) for _ in range(4))
    v = v.abs()
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.05, 2, 1, 0.125)
    a, b = gr.adam_clip_ref64(p, gg, m, v, *hyper, 0.3), gr.adam_clip_yard(p, gg, m, v, *hyper, 0.3)
    assert _rel(b["m"], a["m"]) <= 1e-6 and _rel(b["v"], a["v"]) <= 1e-5 and _rel(b["p"], a["p"]) <= 1e-6
    hs = (0.05, 0.9, 1e-2, 1, 0, 0.5)
    a, b = gr.sgd_clip_ref64(p, gg, m, *hs, 0.3), gr.sgd_clip_yard(p, gg, m, *hs, 0.3)
    assert _rel(b["p"], a["p"]) <= 1e-6 and _rel(b["buf"], a["buf"]) <= 1e-6


# the new entry points and their parameter counts (include/hamspine.h)
ENTRIES = {"hs_grad_sumsq_multi": 5, "hs_grad_norm_partials": 2, "hs_grad_norm_finish": 6, "hs_grad_scale_multi": 5,
           "hs_adam_step_multi_clip": 17, "hs_sgd_step_multi_clip": 13}


def test_header_declares_the_entry_points_and_the_binding_types_them():
    text = open(L.HEADER_PATH).read()
    h = L.parse_header(text)
    assert set(ENTRIES) <= set(L.exported_symbols())
    for name, count in ENTRIES.items():
        ret, params = h.prototypes[name]
        assert len(params) == count, (name, params)
        assert ret == ("int64_t" if name == "hs_grad_norm_partials" else "hs_status")
        # every declaration says what it replaces
        head = text[:re.search(r"^\w+ " + name + r"\(", text, flags=re.M).start()]
        comment = head[head.rindex("/*"):]
        assert "no reference counterpart" in " ".join(comment.lower().split()), name
    assert "torch.nn.utils.clip_grad_norm_" in text
    assert h.prototypes["hs_grad_sumsq_multi"][1] == ["int32_t", "const float*const*", "const int64_t*", "double*", "void*"]
    assert h.prototypes["hs_grad_norm_finish"][1] == ["const double*", "int64_t", "float", "int32_t", "float*", "void*"]
    # the _clip steps: the arguments of the entry points they extend, plus `const float* rec` in front of the stream
    for clip, plain in (("hs_adam_step_multi_clip", "hs_adam_step_multi_shadow"), ("hs_sgd_step_multi_clip", "hs_sgd_step_multi")):
        a, b = h.prototypes[clip][1], h.prototypes[plain][1]
        assert a == b[:-1] + ["const float*", "void*"], clip
    assert h.constants["HS_GRADCLIP_MAX"] == gr.GRADCLIP_MAX == L.GRADCLIP_MAX
    # the existing optimizer entry points keep their signatures
    assert len(h.prototypes["hs_adam_step_multi_shadow"][1]) == 16 and len(h.prototypes["hs_sgd_step_multi"][1]) == 12
    assert len(h.prototypes["hs_adam_step_multi"][1]) == 15
    lib = L.lib()
    for name, count in ENTRIES.items():
        assert len(getattr(lib, name).argtypes) == count, name
    assert lib.hs_grad_norm_partials.restype is L.C.c_int64
    # the host-only helper: one slot per tensor at least, laid end to end; refusals
    cnt = lambda ns: (L.C.c_int64 * max(len(ns), 1))(*ns)
    assert lib.hs_grad_norm_partials(3, cnt([0, 1, 5])) == 3 and lib.hs_grad_norm_partials(0, None) == 0
    big = lib.hs_grad_norm_partials(1, cnt([1 << 22]))
    assert 1 < big <= (1 << 22) // 256
    assert lib.hs_grad_norm_partials(2, cnt([1 << 22, 7])) == big + 1
    assert lib.hs_grad_norm_partials(-1, cnt([1])) == -1 and lib.hs_grad_norm_partials(gr.GRADCLIP_MAX + 1, cnt([1])) == -1
    assert lib.hs_grad_norm_partials(1, cnt([-1])) == -1 and lib.hs_grad_norm_partials(1, None) == -1


def test_python_refusals_that_need_no_device():
    from hamspine import optim
    mk = lambda: [torch.nn.Parameter(torch.zeros(4))]
    for cls in (optim.FusedAdam, optim.FusedAdamW):
        with pytest.raises(ValueError, match="overlap_backward"):
            cls(mk(), max_grad_norm=1.0, overlap_backward=True)
    for cls in (optim.FusedAdam, optim.FusedAdamW, optim.FusedSGD):
        with pytest.raises(ValueError, match="nonfinite"):
            cls(mk(), max_grad_norm=1.0, nonfinite="ignore")
        with pytest.raises(ValueError, match="nonfinite"):
            cls(mk(), nonfinite="raise")
        for bad in (-1.0, float("nan")):
            with pytest.raises(ValueError, match="max_grad_norm"):
                cls(mk(), max_grad_norm=bad)
        o = cls(mk(), lr=1e-3, max_grad_norm=2, nonfinite="skip")
        assert o.max_grad_norm == 2.0 and o.nonfinite == "skip" and o.grad_norm is None and o.grad_clip_coef is None
        assert o.grad_finite is None
        # the settings are attributes: param_groups and state_dict() keep torch.optim's layout
        plain = cls(mk(), lr=1e-3)
        assert plain.max_grad_norm is None and plain.nonfinite == "propagate"
        assert set(o.param_groups[0]) == set(plain.param_groups[0])
        assert set(o.state_dict()) == set(plain.state_dict()) == {"state", "param_groups"}
        assert o.state_dict()["param_groups"] == plain.state_dict()["param_groups"]
        assert cls(mk(), max_grad_norm=float("inf")).max_grad_norm == float("inf")
    p = mk()
    p[0].grad = torch.ones(4)
    with pytest.raises(NotImplementedError, match="norm_type"):
        optim.clip_grad_norm_(p, 1.0, norm_type=3)
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_(p, 1.0, norm_type=float("inf"))
    with pytest.raises(ValueError):
        optim.clip_grad_norm_(p, -1.0)
    with pytest.raises(TypeError):
        optim.clip_grad_norm_(p, None)
    assert torch.equal(p[0].grad, torch.ones(4))
    # no gradient at all: torch returns a zero norm, and so does this
    assert float(optim.clip_grad_norm_(mk(), 1.0)) == 0.0
    # a CPU gradient is refused, not clipped by another route
    import hamspine
    with pytest.raises(hamspine.HamspineError):
        optim.clip_grad_norm_(p, 1.0)
    assert torch.equal(p[0].grad, torch.ones(4))


def test_settings_survive_pickling_and_deepcopy():
    """torch.optim.Optimizer pickles defaults, state and param_groups only: the clip settings travel with them"""
    import copy
    import pickle
    from hamspine import optim
    for cls in (optim.FusedSGD, optim.FusedAdamW):
        o = cls([torch.nn.Parameter(torch.zeros(4))], lr=1e-3, max_grad_norm=2.0, nonfinite="skip")
        for back in (copy.deepcopy(o), pickle.loads(pickle.dumps(o))):
            assert back.max_grad_norm == 2.0 and back.nonfinite == "skip" and back._skip_nonfinite and back.grad_norm is None
            assert back._gradnorm is not None and back._gradnorm is not o._gradnorm
        plain = copy.deepcopy(cls([torch.nn.Parameter(torch.zeros(4))], lr=1e-3))
        assert plain.max_grad_norm is None and plain.nonfinite == "propagate" and plain._gradnorm is None
