"""MuonWithAuxAdam on the HIP kernels of csrc/muon.hip (reference scripts/train.py:262-307) against the float64 restatement of
the specification in tests/muon_ref.py.

Tolerance of the f32-mode checks ("the tolerance of test 1" below): max-abs error relative to max|reference| <= 10 x the
distance of the float32 CPU restatement from float64 on the same input (measured in the test) + 1e-5.  The factor 10 is the
margin the project uses for summation-order differences between two f32 evaluations."""
import ctypes as C
import io
import math
import os

import pytest
import torch

import golden_cases as gc
import muon_ref as mr

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from hamspine import _lib as L  # noqa: E402
from hamspine import rt  # noqa: E402
from hamspine.optim import MuonWithAuxAdam  # noqa: E402

F64 = torch.float64
# (count, rows, cols): eight single matrices, a group of three (the batched launch), two long-K matrices (split-K)
SHAPES = [(1, 1, 128), (1, 2, 768), (1, 7, 256), (1, 256, 7), (1, 64, 147), (1, 72, 200), (1, 200, 72), (1, 136, 136),
          (3, 72, 200), (1, 96, 2304), (1, 2304, 96)]
KINDS = ("gauss", "lowrank")


def _input(count, rows, cols, kind):
    g = torch.Generator().manual_seed(1000 * rows + cols + (7 if kind == "lowrank" else 0) + count)
    if kind == "gauss":
        return torch.randn(count, rows, cols, generator=g)
    k = max(1, min(rows, cols) // 4)          # rank min/4, plus noise at 1e-3
    return torch.randn(count, rows, k, generator=g) @ torch.randn(count, k, cols, generator=g) + 1e-3 * torch.randn(count, rows, cols, generator=g)


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _orthogonalize_on_device(U, mode):
    """U: (count, rows, cols) f32 on the CPU -> the product's Newton-Schulz result, through the three entry points the optimizer
    uses: the pre-pass with beta = 0 and m = 0 (u = g, packed = g / (|g| + 1e-7)), one hs_muon_orthogonalize over the group, and
    the apply pass onto p = 0 with lr = -1, scale 1 (p = O)."""
    lib = L.lib()
    count, rows, cols = U.shape
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    hs_dt = rt.hs_dtype(dt)
    r8, c8 = (rows + 7) // 8 * 8, (cols + 7) // 8 * 8
    g = U.cuda().contiguous()
    m = torch.zeros_like(g)
    p = torch.zeros_like(g)
    packed = torch.full((count, r8, c8), float("nan"), dtype=dt, device="cuda")      # the pad must be written, not assumed
    partials = torch.empty(count * L.MUON_PARTIALS, dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.hs_muon_ws_bytes(hs_dt, count, rows, cols)), dtype=torch.uint8, device="cuda")
    ptrs = lambda t: _arr(C.c_void_p, [t[i].data_ptr() for i in range(count)])
    rws, cls = _arr(C.c_int32, [rows] * count), _arr(C.c_int32, [cols] * count)
    s = rt.stream()
    L.check(lib.hs_muon_prepare_multi(hs_dt, count, ptrs(m), ptrs(g), ptrs(packed), rws, cls, 0.0, partials.data_ptr(), s), "prepare")
    L.check(lib.hs_muon_orthogonalize(hs_dt, count, rows, cols, packed.data_ptr(), ws.data_ptr(), ws.numel(), s), "orthogonalize")
    L.check(lib.hs_muon_apply_multi(hs_dt, count, ptrs(p), None, ptrs(packed), rws, cls, _arr(C.c_float, [1.0] * count), -1.0, 0.0, s),
            "apply")
    torch.cuda.synchronize()
    assert torch.equal(m, g), "momentum with beta = 0 is the gradient"
    pk = packed.float().cpu()
    assert float(pk[:, rows:, :].abs().max() if r8 > rows else 0.0) == 0.0 and float(pk[:, :, cols:].abs().max() if c8 > cols else 0.0) == 0.0, \
        "the pad of the packed matrices stays zero through the iteration"
    return p.cpu()


_cache = {}


def _case(count, rows, cols, kind):
    """input, float64 reference and the float32 / bfloat16 CPU restatements' distances from it, computed once"""
    key = (count, rows, cols, kind)
    if key not in _cache:
        U = _input(count, rows, cols, kind)
        ref = mr.newton_schulz(U, F64)
        scale = ref.abs().amax(dim=(-2, -1))
        d32 = ((mr.newton_schulz(U, torch.float32).double() - ref).abs().amax(dim=(-2, -1)) / scale)
        bf = mr.newton_schulz(U, torch.bfloat16).double()
        dbf = (bf - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
        _cache[key] = (U, ref, d32, dbf)
    return _cache[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_orthogonalisation_f32_mode(shape, kind):
    U, ref, d32, _ = _case(*shape, kind)
    got = _orthogonalize_on_device(U, "f32").double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().amax(dim=(-2, -1)) / ref.abs().amax(dim=(-2, -1))
    print(f"f32 {shape} {kind}: err {err.tolist()} f32-restatement {d32.tolist()}")
    assert bool((err <= 10 * d32 + 1e-5).all()), (shape, kind, err.tolist(), d32.tolist())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_orthogonalisation_bf16_mode(shape, kind):
    """bf16 Newton-Schulz is ill-conditioned on low-rank and square-ish inputs (the bf16 torch restatement itself is 0.3-1.6 away
    from float64 in relative Frobenius norm on rank-deficient inputs), so an elementwise comparison there tests nothing.  The
    distance from float64 is therefore asserted only for the Gaussian inputs of the rectangular shapes, 10 of the 11 (aspect
    ratio min/max <= 0.4, and (64, 147) at 0.435, the stem filter's shape): the square shape (136, 136) and every low-rank input
    are left to the two checks that hold for all inputs -- finite values and a largest singular value <= 1.3.  Where it is
    asserted the bound is the bf16 torch-CPU restatement's own distance on the same input, with no extra factor: rounding the
    f32-normalised input once and keeping f32 accumulators sits below it (measured on an MI355X: 0.012-0.016 against the
    restatement's 0.025-0.040)."""
    count, rows, cols = shape
    U, ref, _, dbf = _case(*shape, kind)
    got = _orthogonalize_on_device(U, "bf16").double()
    assert torch.isfinite(got).all()
    smax = torch.linalg.svdvals(got).amax(dim=-1)
    dist = (got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    print(f"bf16 {shape} {kind}: dist {dist.tolist()} bf16-restatement {dbf.tolist()} sigma_max {smax.tolist()}")
    assert bool((smax <= 1.3).all()), (shape, kind, smax.tolist())
    if kind == "gauss" and min(rows, cols) / max(rows, cols) <= 0.45:
        assert bool((dist <= dbf).all()), (shape, dist.tolist(), dbf.tolist())


# ------------------------------------------------------------------------------------------------------ the optimizer
TRAJ_SHAPES = [(300, 7), (64, 3, 3, 3), (128, 64, 1, 1), (40,), (5,)]
MUON_KW = dict(lr=0.05, momentum=0.9, weight_decay=0.1)
ADAM_KW = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-10, weight_decay=0.05)


def _traj_tensors(seed):
    g = torch.Generator().manual_seed(seed)
    ts = [torch.randn(*s, generator=g) for s in TRAJ_SHAPES]
    ts[1] = ts[1].contiguous(memory_format=torch.channels_last)
    return ts


def _groups(params):
    return [dict(params=[p for p in params if p.ndim >= 2], use_muon=True, **MUON_KW),
            dict(params=[p for p in params if p.ndim < 2], use_muon=False, **ADAM_KW)]


def _set_grads(params, step, dtype, device):
    for i, (p, g) in enumerate(zip(params, _traj_tensors(50 + step))):
        skip = step == 1 and i in (2, 4)            # second step: one Muon and one auxiliary parameter without a gradient
        p.grad = None if skip else g.to(device=device, dtype=dtype)


def _new_params(dtype, device):
    return [torch.nn.Parameter(t.to(device=device, dtype=dtype)) for t in _traj_tensors(40)]


def _ref_trajectory(dtype, steps=3):
    params = _new_params(dtype, "cpu")
    opt = mr.RefMuonWithAuxAdam(_groups(params))
    out = []
    for s in range(steps):
        _set_grads(params, s, dtype, "cpu")
        opt.step()
        out.append([p.detach().double().clone() for p in params])
    return out, opt, params


def _within_test1_tolerance(got, ref64, ref32, what):
    scale = ref64.abs().max()
    err = (got.double() - ref64).abs().max() / scale
    d32 = (ref32 - ref64).abs().max() / scale
    print(f"{what}: err {float(err):.3e} f32-restatement {float(d32):.3e}")
    assert float(err) <= 10 * float(d32) + 1e-5, (what, float(err), float(d32))


@pytest.fixture()
def f32_mode():
    hamspine.set_compute_dtype("f32")
    try:
        yield
    finally:
        hamspine.set_compute_dtype("bf16")


def test_optimizer_trajectory_f32_mode(f32_mode):
    ref64, ropt, rparams = _ref_trajectory(F64)
    ref32, _, _ = _ref_trajectory(torch.float32)
    params = _new_params(torch.float32, "cuda")
    assert params[1].is_contiguous(memory_format=torch.channels_last) and not params[1].is_contiguous()
    opt = MuonWithAuxAdam(_groups(params))
    for s in range(3):
        _set_grads(params, s, torch.float32, "cuda")
        before = [p.detach().clone() for p in params]
        st_before = {i: {k: v.clone() for k, v in opt.state[params[i]].items()} for i in (2, 4)}
        opt.step()
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            _within_test1_tolerance(p.detach().cpu(), ref64[s][i], ref32[s][i], f"step {s} parameter {TRAJ_SHAPES[i]}")
        if s == 1:      # no gradient: values and states untouched
            for i in (2, 4):
                assert torch.equal(params[i].detach(), before[i])
                assert set(opt.state[params[i]]) == set(st_before[i])
                for k, v in st_before[i].items():
                    assert torch.equal(opt.state[params[i]][k], v), (i, k)
    assert float(opt.state[params[3]]["step"]) == 3 and float(opt.state[params[4]]["step"]) == 2     # per parameter
    assert set(opt.state[params[0]]) == {"momentum_buffer"} and set(opt.state[params[3]]) == {"step", "exp_avg", "exp_avg_sq"}
    for i in (0, 1, 2):
        m64 = ropt.state[rparams[i]]["momentum_buffer"]
        assert (opt.state[params[i]]["momentum_buffer"].cpu().double() - m64).abs().max().item() <= 1e-6 * m64.abs().max().item()


def test_state_dict_round_trip_continues_bit_identically(f32_mode):
    pa = _new_params(torch.float32, "cuda")
    oa = MuonWithAuxAdam(_groups(pa))
    for s in range(2):
        _set_grads(pa, s, torch.float32, "cuda")
        oa.step()
    pb = [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in pa]
    ob = MuonWithAuxAdam(_groups(pb))
    buf = io.BytesIO()                       # through a file, as a checkpoint goes: the loaded state shares no memory with oa's
    torch.save(oa.state_dict(), buf)
    buf.seek(0)
    ob.load_state_dict(torch.load(buf))
    assert set(ob.state_dict()["state"][0]) == {"momentum_buffer"} and set(ob.state_dict()["state"][3]) == {"step", "exp_avg", "exp_avg_sq"}
    for params, opt in ((pa, oa), (pb, ob)):
        _set_grads(params, 2, torch.float32, "cuda")
        opt.step()
    torch.cuda.synchronize()
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
    for a, b in zip(pa, pb):
        for k in oa.state[a]:
            assert torch.equal(torch.as_tensor(oa.state[a][k]).cpu(), torch.as_tensor(ob.state[b][k]).cpu()), k


def _baseline_model(tmp_path):
    import model as product_model
    from oracle.procedural import load_procedural
    seed, kw = gc.E2E_CASES["e2e_basic_mlp"]
    d = gc.save_bert_dir(gc.TINY_BERT, os.path.join(str(tmp_path), "bert"))
    m = product_model.MultimodalBaselineModel(pretrained_image=False, image_weights_path=None, text_model_name=d,
                                              **gc.E2E_COMMON, **kw)
    load_procedural(m, seed)
    return m.to("cuda").train()


def _train_py_groups(params):
    """scripts/train.py:289-306"""
    muon_params, aux_params = [], []
    for p in params:
        (muon_params if p.ndim >= 2 else aux_params).append(p)
    return [dict(params=muon_params, use_muon=True, lr=0.02, weight_decay=0.01),
            dict(params=aux_params, use_muon=False, lr=3e-4, betas=(0.9, 0.95), weight_decay=0.01)]


def _forward(m, batch):
    images, ids, mask, _ = batch
    return m.classifier(m.forward_features(images.cuda(), ids.cuda(), mask.cuda(), tabular_input=None, ablation_mode=None))


def test_real_layouts_of_the_baseline_model(tmp_path):
    from oracle.procedural import synthetic_batch
    batch = synthetic_batch(4, 64, 24, gc.TINY_BERT["vocab_size"], 7, seed=900, min_len=3)
    hamspine.set_compute_dtype("f32")
    try:
        m = _baseline_model(tmp_path)
        params = [p for p in m.parameters() if p.requires_grad]
        torch.nn.functional.cross_entropy(_forward(m, batch), batch[3].cuda()).backward()
        params = [p for p in params if p.grad is not None]
        assert any(p.ndim == 4 and not p.is_contiguous() for p in params), "the image tower keeps channels_last filters"
        refs = {}
        for dt in (F64, torch.float32):
            clones = [torch.nn.Parameter(p.detach().cpu().to(dt)) for p in params]
            for c, p in zip(clones, params):
                c.grad = p.grad.detach().cpu().to(dt)
            mr.RefMuonWithAuxAdam(_train_py_groups(clones)).step()
            refs[dt] = [c.detach().double() for c in clones]
        MuonWithAuxAdam(_train_py_groups(params)).step()
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            _within_test1_tolerance(p.detach().cpu(), refs[F64][i], refs[torch.float32][i], f"parameter {i} {tuple(p.shape)}")
    finally:
        hamspine.set_compute_dtype("bf16")
    # bf16 mode: the apply pass also writes the bf16 weight shadows the towers read -- a stale shadow is a silent wrong forward
    m = _baseline_model(tmp_path)
    params = [p for p in m.parameters() if p.requires_grad]
    opt = MuonWithAuxAdam(_train_py_groups(params))
    for _ in range(2):          # the second step runs with the shadow pointers the first forward registered
        opt.zero_grad()
        torch.nn.functional.cross_entropy(_forward(m, batch), batch[3].cuda()).backward()
        opt.step()
    assert any(rt.shadow_ptr_of(p) is not None for p in params if p.ndim >= 2)
    with torch.no_grad():
        a = _forward(m, batch).float().clone()
        rt.shadows_stale(params)
        b = _forward(m, batch).float().clone()
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_lr_schedulers_drive_both_groups(f32_mode):
    for make in (lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda step: 1.0 / (1 + step)),
                 lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=4)):
        params = _new_params(torch.float32, "cuda")
        opt = MuonWithAuxAdam(_groups(params))
        rparams = _new_params(F64, "cpu")
        ropt = mr.RefMuonWithAuxAdam(_groups(rparams))
        sched, rsched = make(opt), make(ropt)
        lrs = []
        for s in range(3):
            _set_grads(params, 0, torch.float32, "cuda")
            _set_grads(rparams, 0, F64, "cpu")
            opt.step()
            ropt.step()
            sched.step()
            rsched.step()
            lrs.append((opt.param_groups[0]["lr"], opt.param_groups[1]["lr"]))
            assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in ropt.param_groups]
        assert lrs[0][0] != MUON_KW["lr"] and lrs[0][1] != ADAM_KW["lr"] and lrs[0] != lrs[2]
        assert math.isclose(lrs[0][0] / MUON_KW["lr"], lrs[0][1] / ADAM_KW["lr"], rel_tol=1e-12)
        torch.cuda.synchronize()
        for p, r in zip(params, rparams):
            err = (p.detach().cpu().double() - r.detach()).abs().max().item() / r.detach().abs().max().item()
            assert err <= 1e-4, err       # the lr reached the kernels: an unscheduled run differs by lr * O(1) >> 1e-4
