"""The float64 references of tests/head_ref.py against torch autograd in double, the data conditions under which float64 and
float32 take the same branches, and the finiteness of every reference of every case that the GPU tests run.  No GPU."""
import numpy as np
import torch
import torch.nn.functional as F

import head_ref as hr
from oracle import models as om

F64 = torch.float64


def _close(a, b, tol, what):
    a, b = a.double(), b.double()
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
    assert err <= tol, f"{what}: {err:.3e} > {tol:.1e}"


def _finite(ref, tag):
    for k, v in ref.items():
        assert bool(torch.isfinite(v).all()), f"{tag}: the float64 reference of {k} is not finite"


def _sane(tag, yard, ref, keys, floors=None, loose=2e-5):
    """the float32 yardstick is a float32 evaluation of the reference: far closer to it than any defect would be"""
    for k in keys:
        top = ref[k].double().abs().max().item()
        err = (yard[k].double() - ref[k].double()).abs().max().item()
        allowed = max(loose, 4.0 * (floors or {}).get(k, 0.0)) * top + 1e-30
        assert err <= allowed, f"{tag} {k}: yardstick off by {err / max(top, 1e-300):.3e}"


# ----------------------------------------------------------------------------------------------------------------------
# cross entropy, focal
# ----------------------------------------------------------------------------------------------------------------------
def test_cross_entropy_reference():
    for c in hr.ce_cases():
        z, y, w, s = c["z"], c["y"], c["weight"], c["s"]
        assert 0 <= int(y.min()) and int(y.max()) < z.shape[1]
        ref = hr.ce_ref64(z, y, w, s)
        _finite(ref, c["tag"])
        zd = z.double().requires_grad_(True)
        wd = None if w is None else w.double()
        loss = F.cross_entropy(zd, y, weight=wd, label_smoothing=hr._f32(s))
        loss.backward()
        _close(ref["loss"], loss.detach().reshape(1), 1e-12, c["tag"] + " loss")
        _close(ref["dlogits"], zd.grad, 1e-11, c["tag"] + " dlogits")
        rows = F.cross_entropy(z.double(), y, weight=wd, label_smoothing=hr._f32(s), reduction="none")
        _close(ref["row_loss"], rows, 1e-12, c["tag"] + " row_loss")
        _sane(c["tag"], hr.ce_yard(z, y, w, s), ref, ("loss", "row_loss", "dlogits"), hr.ce_floors(z, y, w, s, ref))
        if c["margin_row"] is not None:       # the margin row: p is exactly 1 in float32 (exp(-200) < 2^-25)
            r = c["margin_row"]
            others = torch.cat([z[r, :y[r]], z[r, y[r] + 1:]])
            assert others.numel() == 0 or (z[r, y[r]] - others.max()).item() >= hr.MARGIN - 1e-3


def test_focal_reference():
    saturated = 0
    for c in hr.focal_cases():
        z, y, w, gamma = c["z"], c["y"], c["weight"], c["gamma"]
        assert 0 <= int(y.min()) and int(y.max()) < z.shape[1]
        ref = hr.focal_ref64(z, y, w, gamma)
        _finite(ref, c["tag"])
        zd = z.double().requires_grad_(True)
        wd = None if w is None else w.double()
        loss = om.ofocal(zd, y, gamma=hr._f32(gamma), weight=wd)
        loss.backward()
        _close(ref["loss"], loss.detach().reshape(1), 1e-12, c["tag"] + " loss")
        _close(ref["dlogits"], zd.grad, 1e-11, c["tag"] + " dlogits")
        ce = F.cross_entropy(z.double(), y, weight=wd, reduction="none")
        sat = bool((ce < 1e-16).any())
        saturated += sat
        if 0.0 < gamma < 1.0:
            assert not sat and c["kind"] == "randn", c["tag"]
        if gamma == 0.0:                      # plain CE (F.cross_entropy normalises by sum w_y; focal takes the plain mean)
            ce_ref = hr.ce_ref64(z, y, w, 0.0)
            scale = 1.0 if w is None else w.double()[y].sum().item() / z.shape[0]
            _close(ref["loss"], ce_ref["loss"] * scale, 1e-12, c["tag"] + " loss = CE")
            _close(ref["dlogits"], ce_ref["dlogits"] * scale, 1e-11, c["tag"] + " dlogits = CE")
        _sane(c["tag"], hr.focal_yard(z, y, w, gamma), ref, ("loss", "dlogits"), hr.focal_floors(z, y, w, gamma, ref))
    assert saturated >= 10                    # every gamma >= 1 and gamma = 0 meet a saturated row


def test_focal_excluded_case_is_not_finite():
    """the one exclusion (hr.NONFINITE_REFERENCE): 0 < gamma < 1 on a saturated row has no finite float64 gradient"""
    assert len(hr.NONFINITE_REFERENCE) == 1
    g = hr.gen(1)
    y = torch.randint(0, 7, (5,), generator=g)
    z = hr._logits(g, 5, 7, "margin", y)
    ref = hr.focal_ref64(z, y, None, 0.5)
    assert not bool(torch.isfinite(ref["dlogits"]).all())
    for gamma in hr.GAMMAS:
        assert bool(torch.isfinite(hr.focal_ref64(z, y, None, gamma)["dlogits"]).all())


# ----------------------------------------------------------------------------------------------------------------------
# entropy, KL, MP-Loss
# ----------------------------------------------------------------------------------------------------------------------
def test_entropy_reference():
    for c in hr.entropy_cases():
        z, g = c["z"], c["g"]
        ref = hr.entropy_ref64(z, g)
        _finite(ref, c["tag"])
        p = torch.softmax(z.double(), 1)          # the analytic backward, independently of autograd
        t = -(torch.log(p + hr.E8) + p / (p + hr.E8))
        hand = g.double()[:, None] * p * (t - (p * t).sum(1, keepdim=True))
        # (on a saturated row t - sum p t cancels in float64 too: the two evaluations agree to 1e-16 of |g| |t|, not of dz)
        assert (ref["dlogits"] - hand).abs().max().item() <= 1e-10 * hand.abs().max().item() + 1e-14, c["tag"] + " dlogits"
        _close(ref["ent"], -(p * torch.log(p + hr.E8)).sum(1), 1e-12, c["tag"] + " ent")
        _sane(c["tag"], hr.entropy_yard(z, g), ref, ("ent", "dlogits"), hr.entropy_floors(z, g, ref))


def _off_bounds(v, eps, what):
    """no value within 1e-3 relative of eps or of 1 unless exactly on it"""
    v = v.double()
    for b in (hr._f32(eps), 1.0):
        near = ((v / b - 1.0).abs() < 1e-3) & (v != b)
        assert not bool(near.any()), f"{what}: a value within 1e-3 of the clamp bound {b:g}"


def test_kl_rows_reference():
    planted = set()
    for c in hr.kl_cases():
        p, q, w, eps = c["p"], c["q"], c["w"], c["eps"]
        _off_bounds(p, eps, c["tag"] + " p")
        _off_bounds(q, eps, c["tag"] + " q")
        ref = hr.kl_rows_ref64(p, q, eps, w)
        _finite(ref, c["tag"])
        pd, qd = p.double().requires_grad_(True), q.double().requires_grad_(True)
        out = om.okl(pd, qd, eps=hr._f32(eps))
        (w.double() * out).sum().backward()
        _close(ref["out"], out.detach(), 1e-12, c["tag"] + " out")
        _close(ref["dp"], pd.grad, 1e-12, c["tag"] + " dp")
        _close(ref["dq"], qd.grad, 1e-12, c["tag"] + " dq")
        # the reference's clamp passes the gradient on both bounds
        e32 = torch.tensor(np.float32(eps))
        for t, gname in ((p, "dp"), (q, "dq")):
            on = (t == 1.0) | (t == e32)
            if bool(on.any()):
                assert bool((ref[gname][on] != 0).all()), f"{c['tag']}: {gname} is 0 on a clamp bound"
            out_of = (t > 1.0) | (t < e32)
            assert bool((ref[gname][out_of] == 0).all())
            planted |= {float(v) for v in t[on | out_of].tolist()}
        _sane(c["tag"], hr.kl_rows_yard(p, q, eps, w), ref, ("out", "dp", "dq"), hr.kl_rows_floors(p, q, eps, w, ref))
    assert planted >= {float(np.float32(v)) for v in hr.kl_planted()}


def test_mp_loss_reference():
    seen = set()
    for c in hr.mp_cases():
        zi, zt, zf, y = c["zi"], c["zt"], c["zf"], c["y"]
        assert 0 <= int(y.min()) and int(y.max()) < zi.shape[1]
        ref = hr.mp_ref64(zi, zt, zf, y)
        _finite(ref, c["tag"])
        # the oracle's own pieces with the kernel's float32 constants (0.3f, 0.6f, 1.1f, 1e-8f) ...
        a, t, f = (v.double().requires_grad_(True) for v in (zi, zt, zf))
        pi, pt = F.softmax(a, dim=-1), F.softmax(t, dim=-1)
        kl = (om.okl(pi, pt, eps=hr.E8) + om.okl(pt, pi, eps=hr.E8)) / 2
        kl = torch.nan_to_num(kl, nan=0.0, posinf=10.0, neginf=0.0).clamp(0.0, 10.0)
        loss = (hr.C03 * F.cross_entropy(a, y) + hr.C06 * F.cross_entropy(t, y)
                + hr.C11 * torch.mean(torch.exp(kl) * F.cross_entropy(f, y)))
        loss.backward()
        _close(ref["loss"], loss.detach().reshape(1), 1e-12, c["tag"] + " loss")
        for k, v in (("d_image", a), ("d_text", t), ("d_fused", f)):
            _close(ref[k], v.grad, 1e-10, c["tag"] + " " + k)
        # ... and omp_loss as it stands: its constants are doubles, 4e-8 and (1e-8 against 1e-8f) 6e-8 apart, which exp(kl)
        # with kl up to 10 magnifies to 1e-6
        a, t, f = (v.double().requires_grad_(True) for v in (zi, zt, zf))
        loss = om.omp_loss({"image": a, "text": t, "image_text": f}, y)
        loss.backward()
        _close(ref["loss"], loss.detach().reshape(1), 5e-6, c["tag"] + " loss (omp_loss)")
        for k, v in (("d_image", a), ("d_text", t), ("d_fused", f)):
            _close(ref[k], v.grad, 5e-6, c["tag"] + " " + k + " (omp_loss)")
        kl = hr.mp_raw_kl64(zi, zt)
        assert not bool(((kl > 9.99) & (kl < 10.01)).any()), c["tag"] + ": a raw kl next to the clamp at 10"
        assert not bool(((kl > 0.0) & (kl < 1e-6)).any()), c["tag"] + ": a raw kl next to the clamp at 0"
        for v in (zi, zt):                       # softmax probabilities never exceed 1: only the lower bound can be met
            pr = torch.softmax(v.double(), 1)
            assert not bool(((pr / hr.E8 - 1.0).abs() < 1e-3).any()), c["tag"] + ": a probability next to 1e-8"
        if c["kind"] == "identical":
            assert bool((kl == 0).all())
        if c["kind"] == "disagree":
            assert bool((kl > 10.01).all())
        if c["kind"] == "margin":
            assert bool((torch.softmax(zi.double(), 1).min(1).values < hr.E8).all())
        if c["kind"] == "agree":
            assert bool((kl < 0.1).all())
        seen.add(c["kind"])
        _sane(c["tag"], hr.mp_yard(zi, zt, zf, y), ref, ("loss", "d_image", "d_text", "d_fused"), hr.mp_floors(zi, zt, zf, y, ref))
    assert seen == set(hr.MP_KINDS)


# ----------------------------------------------------------------------------------------------------------------------
# SupCon, KAN regularisation
# ----------------------------------------------------------------------------------------------------------------------
def test_supcon_reference():
    for c in hr.supcon_cases():
        f, lab, T = c["feat"], c["labels"], c["T"]
        assert bool((f.double().norm(dim=1) > 1e-3).all()), c["tag"] + ": a zero-norm row"
        ref = hr.supcon_ref64(f, lab, T)
        _finite(ref, c["tag"])
        fd = f.double().requires_grad_(True)
        loss = om.osupcon(fd, lab, temperature=hr._f32(T))
        loss.backward()
        top = max(ref["dfeat"].abs().max().item(), 1e-300)
        assert abs(ref["loss"].item() - loss.item()) <= 1e-7 * max(abs(loss.item()), 1e-30) + 1e-14, c["tag"] + " loss"
        assert (ref["dfeat"] - fd.grad).abs().max().item() <= 1e-7 * top + 1e-13, c["tag"] + " dfeat"
        if c["pattern"] == "distinct":
            assert ref["loss"].item() == 0.0 and bool((ref["dfeat"] == 0).all())
        fl = hr.supcon_floors(f, lab, T, ref)
        yard = hr.supcon_yard(f, lab, T)
        _sane(c["tag"], yard, ref, ("loss",), fl)
        if f.shape[1] == 1:
            assert (yard["dfeat"].double() - ref["dfeat"]).abs().max().item() <= 4.0 * fl["dfeat_abs"] + 1e-30
        else:
            _sane(c["tag"], yard, ref, ("dfeat",), fl)


def test_kan_regularization_reference():
    for c in hr.kan_reg_cases():
        w, ra, re = c["w"], c["ra"], c["re"]
        assert bool((w.abs().sum(1) > 0).all())
        ref = hr.kan_reg_ref64(w, ra, re)
        _finite(ref, c["tag"])
        l = w.double().abs().mean(1)              # the kernel's closed form of the gradient, independently of autograd
        A = l.sum()
        E = -((l / A) * (l / A).log()).sum()
        dl = hr._f32(ra) - hr._f32(re) * ((l / A).log() + E) / A
        _close(ref["dw"], torch.sign(w.double()) * (dl / w.shape[1])[:, None], 1e-10, c["tag"] + " dw")
        _close(ref["loss"], (hr._f32(ra) * A + hr._f32(re) * E).reshape(1), 1e-12, c["tag"] + " loss")
        _sane(c["tag"], hr.kan_reg_yard(w, ra, re), ref, ("loss", "dw"), hr.kan_reg_floors(w, ra, re, ref))


# ----------------------------------------------------------------------------------------------------------------------
# LSTM / GRU cells
# ----------------------------------------------------------------------------------------------------------------------
def _torch_cell(cell_cls, gates, gx, gh, prev, c_prev, dh, dc):
    """torch's cell in double, one row at a time: W_ih = identity and b_ih = 0 feed gx through, W_hh = 0 and b_hh = gh[b] feed
    gh through, so that x.grad is the gradient of gx, b_hh.grad that of gh, and h_prev.grad the direct path only"""
    B, H = prev.shape
    G = gates * H
    out = {k: [] for k in ("h", "c", "dgx", "dgh", "dprev", "dc_prev")}
    for b in range(B):
        cell = cell_cls(G, H).double()
        with torch.no_grad():
            cell.weight_ih.copy_(torch.eye(G, dtype=F64))
            cell.bias_ih.zero_()
            cell.weight_hh.zero_()
            cell.bias_hh.copy_(gh[b].double())
        x = gx[b:b + 1].double().requires_grad_(True)
        hp = prev[b:b + 1].double().requires_grad_(True)
        if gates == 4:
            cp = c_prev[b:b + 1].double().requires_grad_(True)
            h, c = cell(x, (hp, cp))
            ((h * dh[b:b + 1].double()).sum() + (c * dc[b:b + 1].double()).sum()).backward()
            out["c"].append(c.detach())
            out["dc_prev"].append(cp.grad)
        else:
            h = cell(x, hp)
            (h * dh[b:b + 1].double()).sum().backward()
            out["dprev"].append(hp.grad)
        out["h"].append(h.detach())
        out["dgx"].append(x.grad)
        out["dgh"].append(cell.bias_hh.grad.reshape(1, -1).clone())
    return {k: torch.cat(v, 0) for k, v in out.items() if v}


def test_lstm_cell_reference():
    for c in hr.cell_cases(4):
        gx, gh, cp, dh, dc = c["gx"], c["gh"], c["prev"], c["dh"], c["dc"]
        fw = hr.lstm_fwd_ref64(gx, gh, cp)
        _finite(fw, c["tag"])
        tc = _torch_cell(torch.nn.LSTMCell, 4, gx, gh, torch.zeros_like(cp), cp, dh, dc)
        _close(fw["h"], tc["h"], 1e-12, c["tag"] + " h")
        _close(fw["c"], tc["c"], 1e-12, c["tag"] + " c")
        bw = hr.lstm_bwd_ref64(dh, dc, fw["act"], cp, fw["c"])
        _finite(bw, c["tag"])
        _close(bw["dgates"], tc["dgx"], 1e-10, c["tag"] + " dgates")
        _close(bw["dgates"], tc["dgh"], 1e-10, c["tag"] + " dgates (gh)")
        _close(bw["dc_prev"], tc["dc_prev"], 1e-10, c["tag"] + " dc_prev")
        _sane(c["tag"], hr.lstm_fwd_yard(gx, gh, cp), fw, ("h", "c", "act"))
        act, cc = fw["act"].float(), fw["c"].float()
        for a, b in ((dh, dc), (None, dc), (dh, None)):
            r = hr.lstm_bwd_ref64(a, b, act, cp, cc)
            _finite(r, c["tag"])
            _sane(c["tag"], hr.lstm_bwd_yard(a, b, act, cp, cc), r, ("dgates", "dc_prev"), hr.lstm_bwd_floors(a, b, act, cp, cc, r))
        if c["scale"] > 1.0:
            y = hr.lstm_fwd_yard(gx, gh, cp)["act"]
            assert bool(((y == 0) | (y == 1) | (y == -1)).any()), c["tag"] + ": no gate saturates exactly"


def test_gru_cell_reference():
    for c in hr.cell_cases(3):
        gx, gh, hp, dh = c["gx"], c["gh"], c["prev"], c["dh"]
        fw = hr.gru_fwd_ref64(gx, gh, hp)
        _finite(fw, c["tag"])
        tc = _torch_cell(torch.nn.GRUCell, 3, gx, gh, hp, None, dh, None)
        _close(fw["h"], tc["h"], 1e-12, c["tag"] + " h")
        bw = hr.gru_bwd_ref64(dh, fw["act"], hp)
        _finite(bw, c["tag"])
        _close(bw["dgx"], tc["dgx"], 1e-10, c["tag"] + " dgx")
        _close(bw["dgh"], tc["dgh"], 1e-10, c["tag"] + " dgh")
        _close(bw["dh_prev"], tc["dprev"], 1e-10, c["tag"] + " dh_prev")
        _sane(c["tag"], hr.gru_fwd_yard(gx, gh, hp), fw, ("h", "act"))
        act = fw["act"].float()
        r = hr.gru_bwd_ref64(dh, act, hp)
        _finite(r, c["tag"])
        _sane(c["tag"], hr.gru_bwd_yard(dh, act, hp), r, ("dgx", "dgh", "dh_prev"), hr.gru_bwd_floors(dh, act, hp, r))


# ----------------------------------------------------------------------------------------------------------------------
# KAN features
# ----------------------------------------------------------------------------------------------------------------------
_ACT_MODULES = (torch.nn.SiLU, torch.nn.GELU, torch.nn.ReLU, torch.nn.Identity)


def test_kan_features_reference():
    on_knot = below = above = 0
    for c in hr.kan_cases():
        x, grid, gs, order, act, dfeat = c["x"], c["grid"], c["gs"], c["order"], c["act"], c["dfeat"]
        B, in_f = x.shape
        assert grid.shape == (in_f, gs + 2 * order + 1) and grid.shape[1] <= 32
        assert bool((grid[:, 1:] > grid[:, :-1]).all()), c["tag"] + ": knots not strictly increasing"
        dist = (x.double()[:, :, None] - grid.double()[None]).abs()
        assert not bool(((dist < 1e-4) & (dist != 0)).any()), c["tag"] + ": an x within 1e-4 of a knot"
        on_knot += int((dist == 0).sum())
        below += int((x < grid[None, :, 0]).sum())
        above += int((x > grid[None, :, -1]).sum())
        ref = hr.kan_ref64(x, grid, order, act, dfeat)
        _finite(ref, c["tag"])
        layer = om.OKANLinear(in_f, 1, grid_size=gs, spline_order=order, base_activation=_ACT_MODULES[act]).double()
        layer.grid.copy_(grid.double())
        xd = x.double().requires_grad_(True)
        feat = torch.cat([layer.base_activation(xd), layer.b_splines(xd).reshape(B, -1)], 1)
        (feat * dfeat.double()).sum().backward()
        _close(ref["feat"], feat.detach(), 1e-12, c["tag"] + " feat")
        _close(ref["dx"], xd.grad, 1e-10, c["tag"] + " dx")
        nb = gs + order
        outside = (x < grid[None, :, 0]) | (x >= grid[None, :, -1])
        bases = ref["feat"][:, in_f:].reshape(B, in_f, nb)
        assert bool((bases[outside] == 0).all()), c["tag"] + ": a basis outside the grid is not 0"
        _sane(c["tag"], hr.kan_yard(x, grid, order, act, dfeat), ref, ("feat", "dx"))
    assert on_knot > 100 and below > 20 and above > 20
