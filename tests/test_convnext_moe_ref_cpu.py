"""The float64 references of tests/convnext_moe_ref.py against torch's own convolutions and autograd in double, the selection
margins of every gating case, the exactness of the integer cases, and every float32 yardstick against its floor.  No GPU."""
import numpy as np
import torch
import torch.nn.functional as F

import convnext_moe_ref as cm

F64 = torch.float64
TWO24 = float(2 ** 24)


def _close(a, b, tol, what):
    a, b = a.double(), b.double()
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
    assert err <= tol, f"{what}: {err:.3e} > {tol:.1e}"


def _yard_ok(tag, yard, ref, floor=0.0, reduced=False, dtype=torch.float32):
    """the yardstick is a float32 evaluation of the reference: within the a-priori floor where the output has one, else within
    a few float32 roundings (2e-5 of the largest value; bf16 outputs: one rounding, 2^-8)"""
    err = (cm.rel if reduced else cm.maxrel)(yard, ref)
    allowed = max(floor, 1e-6) if floor > 0.0 else (2.0 ** -8 if dtype == torch.bfloat16 else 2e-5)
    assert err <= allowed, f"{tag}: yardstick off by {err:.3e} (allowed {allowed:.3e})"
    return err


# ----------------------------------------------------------------------------------------------------------------------
# depthwise convolution
# ----------------------------------------------------------------------------------------------------------------------
def _conv2d_all(x, w, bias, dy, ks):
    """F.conv2d(groups=C) in float64 and its autograd -> y, dx, dw, db in the layouts of the reference"""
    Cc = x.shape[3]
    xn = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = w.double().reshape(Cc, 1, ks, ks).clone().requires_grad_(True)
    b = (torch.zeros(Cc, dtype=F64) if bias is None else bias.double().clone()).requires_grad_(True)
    y = F.conv2d(xn, wt, b, padding=ks // 2, groups=Cc)
    y.backward(dy.double().permute(0, 3, 1, 2))
    return {"y": y.detach().permute(0, 2, 3, 1), "dx": xn.grad.permute(0, 2, 3, 1), "dw": wt.grad.reshape(Cc, ks * ks), "db": b.grad}


def test_dwconv_reference_and_yardstick():
    for dtype in cm.DTYPES:
        for c in cm.dwconv_fwd_cases() + cm.dwconv_wgrad_cases():
            x, dy, w, bias = cm.dwconv_data(c, dtype)
            ks = c["ks"]
            ref, yard = cm.dwconv_ref64(x, w, bias, dy, ks), cm.dwconv_yard(x, w, bias, dy, ks)
            t = _conv2d_all(x, w, bias, dy, ks)
            tag = f"{c['tag']} {cm.dname(dtype)}"
            for k in ("y", "dx", "dw", "db"):
                _close(ref[k], t[k], 1e-13, f"{tag} {k} against conv2d")
            assert not torch.equal(w, w.flip(1)), tag + ": symmetric filter"
            fl = cm.dwconv_wgrad_floor(ref, c["N"], c["H"], c["W"], c["C"])
            _yard_ok(tag + " y", yard["y"], ref["y"], dtype=dtype)
            _yard_ok(tag + " dx", yard["dx"], ref["dx"], dtype=dtype)
            _yard_ok(tag + " dw", yard["dw"], ref["dw"], fl["dw"], reduced=True)
            _yard_ok(tag + " db", yard["db"], ref["db"], fl["db"], reduced=True)
            if c["kind"] == "int":
                assert bool((x.float() == x.float().round()).all()) and x.float().abs().max() <= 3
                wa, ba = w.double().abs(), (0.0 if bias is None else bias.double().abs())
                assert cm._dw_corr(x.double().abs(), wa, None, ks, False).max().item() + float(np.max(ba.numpy() if bias is not None else 0)) < TWO24
                assert cm._dw_corr(dy.double().abs(), wa, None, ks, True).max().item() < TWO24
                assert ref["terms"].abs().sum(0).max().item() < TWO24 and dy.double().abs().reshape(-1, c["C"]).sum(0).max() < TWO24
                assert cm.bits_equal(yard["dw"], ref["dw"].float()) and cm.bits_equal(yard["y"], ref["y"].to(dtype))


def test_dwconv_case_coverage():
    f, g = cm.dwconv_fwd_cases(), cm.dwconv_wgrad_cases()
    assert {c["ks"] for c in f} == {3, 5, 7} and {c["W"] for c in f} == {1, 3, 4, 5, 9}
    assert {c["H"] for c in f} == {1, 2, 7} and {c["C"] for c in f} == {4, 8, 132}
    assert any(not c["bias"] for c in f) and {c["ks"] for c in f if c["kind"] == "int"} == {3, 5, 7}
    th = [c["N"] * c["H"] * -(-c["W"] // 4) * (c["C"] // 4) for c in f]
    assert any(t > 256 and t % 256 for t in th)
    assert {1, 15, 16, 17, 33} <= {c["W"] for c in g} and {4, 124, 128, 132, 260} <= {c["C"] for c in g}
    nh = {c["N"] * c["H"] for c in g if c["C"] == 8 and c["W"] == 3}
    assert {1, 3, 4, 5, 8, 9, 12, 13} <= nh
    assert all(cm.dw_chunks(c["N"], c["H"], 8) == c["N"] * c["H"] for c in g if c["C"] == 8 and c["W"] == 3)
    assert any(c["C"] == 1024 and cm.dw_chunks(c["N"], c["H"], c["C"]) == 128 and c["N"] * c["H"] == 150 for c in g)


# ----------------------------------------------------------------------------------------------------------------------
# layer scale
# ----------------------------------------------------------------------------------------------------------------------
def test_layerscale_reference_and_yardstick():
    seen = set()
    for dtype in cm.DTYPES:
        for c in cm.layerscale_cases():
            u, res, dy, gamma, rs = cm.layerscale_data(c, dtype)
            M, Cc, rps = c["M"], c["C"], c["rps"]
            tag = f"{c['tag']} {cm.dname(dtype)}"
            ref, yard = cm.layerscale_ref64(u, res, dy, gamma, rs, rps), cm.layerscale_yard(u, res, dy, gamma, rs, rps)
            ud = u.double().clone().requires_grad_(True)
            gd = gamma.double().clone().requires_grad_(True)
            fac = torch.ones(M, 1, dtype=F64) if rs is None else rs.double().repeat_interleave(rps)[:M, None]
            out = res.double() + gd * fac * ud
            out.backward(dy.double())
            _close(ref["out"], out.detach(), 1e-14, tag + " out")
            _close(ref["du"], ud.grad, 1e-14, tag + " du")
            _close(ref["dgamma"], gd.grad, 1e-12, tag + " dgamma")
            fl = cm.layerscale_floor(ref, M, Cc)
            _yard_ok(tag + " out", yard["out"], ref["out"], dtype=dtype)
            _yard_ok(tag + " du", yard["du"], ref["du"], dtype=dtype)
            _yard_ok(tag + " dgamma", yard["dgamma"], ref["dgamma"], fl, reduced=True)
            if c["kind"] == "int":
                assert ref["terms"].abs().sum(0).max().item() < TWO24
                assert cm.bits_equal(yard["dgamma"], ref["dgamma"].float())
            if rs is not None and rs.numel() >= 2 and c["zero"]:
                assert rs[1] == 0.0 and rs[0] != 0.0
            gy, blocks = cm.ls_geometry(M, Cc)
            seen |= {("ncol", n) for n, _ in blocks} | {("rpb", r) for _, r in blocks} | {("gy", gy), ("blocks", len(blocks))}
    assert {("ncol", n) for n in (1, 3, 33, 256, 129)} <= seen and ("rpb", 1) in seen and ("gy", 256) in seen and ("blocks", 2) in seen
    cs = cm.layerscale_cases()
    assert {c["C"] for c in cs} == {4, 12, 132, 1024, 1028, 1540} and {1, 5, 31, 32, 257, 4112} == {c["M"] for c in cs}
    assert {(c["M"], c["C"]) for c in cs} >= {(4112, 4), (4112, 1028)}
    assert {None, 1, 7} <= {c["rps"] for c in cs} and any(c["rps"] == c["M"] for c in cs)


# ----------------------------------------------------------------------------------------------------------------------
# patchify
# ----------------------------------------------------------------------------------------------------------------------
def test_patchify_reference():
    for c in cm.patchify_cases():
        N, H, W, Cc, k = c["N"], c["H"], c["W"], c["C"], c["k"]
        x = cm.patchify_data(c, torch.float32).double()
        wt = torch.zeros(k * k * Cc, Cc, k, k, dtype=F64)
        for r in range(k):
            for s in range(k):
                for ch in range(Cc):
                    wt[(r * k + s) * Cc + ch, ch, r, s] = 1.0
        xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        y = F.conv2d(xn, wt, stride=k)                                    # [N][k*k*C][P][Q]
        ref = cm.patchify_ref(x, k)
        assert torch.equal(ref, y.detach().permute(0, 2, 3, 1).reshape(-1, k * k * Cc)), c["tag"]
        dp = torch.randn(ref.shape, dtype=F64, generator=cm.gen(c["seed"]))
        y.backward(dp.reshape(N, H // k, W // k, k * k * Cc).permute(0, 3, 1, 2))
        dx = cm.patchify_bwd_ref(dp, N, H, W, Cc, k)
        assert torch.equal(dx, xn.grad.permute(0, 2, 3, 1)), c["tag"] + " bwd"
        P, Q = H // k, W // k
        assert torch.equal(cm.patchify_bwd_ref(ref, N, H, W, Cc, k)[:, :P * k, :Q * k], x[:, :P * k, :Q * k]), c["tag"] + " round trip"
        if k > 1:
            assert H % k and W % k, c["tag"]
    cs = cm.patchify_cases()
    assert {c["C"] for c in cs} == {3, 4, 8, 12, 24} and {c["k"] for c in cs} == {1, 2, 3, 4}
    assert any((c["N"] * (c["H"] // c["k"]) * (c["W"] // c["k"]) * c["ld"]) % 256 for c in cs)


# ----------------------------------------------------------------------------------------------------------------------
# gating
# ----------------------------------------------------------------------------------------------------------------------
def _moe_py(clean, raw, z, k, noisy, eps, coef):
    """the reference model's gating (moe.py:171-291) with torch.topk, softplus, Normal.cdf and Tensor.var in double"""
    c = clean.double()
    B, E = c.shape
    if noisy:
        std = F.softplus(raw.double()) + eps
        h = c + z.double() * std
    else:
        h = c
    p = torch.softmax(h, 1)
    tv, ti = p.topk(min(k + 1, E), dim=1)
    tg = tv[:, :k] / (tv[:, :k].sum(1, keepdim=True) + 1e-6)
    gates = torch.zeros_like(p).scatter(1, ti[:, :k], tg)
    if noisy and k < E:
        normal = torch.distributions.Normal(torch.tensor(0.0, dtype=F64), torch.tensor(1.0, dtype=F64))
        thr_in, thr_out = tv[:, k:k + 1], tv[:, k - 1:k]
        load = torch.where(h > thr_in, normal.cdf((c - thr_in) / std), normal.cdf((c - thr_out) / std)).sum(0)
    else:
        load = (gates > 0).sum(0).double()

    def cv(x):
        return torch.zeros((), dtype=F64) if x.shape[0] == 1 else x.var() / (x.mean() ** 2 + 1e-10)

    return gates, ti, load, coef * (cv(gates.sum(0)) + cv(load))


def test_gate_reference_margins_and_yardstick():
    for c in cm.gate_cases():
        B, E, k, noisy, tag = c["B"], c["E"], c["k"], c["noisy"], c["tag"]
        clean, raw, z, redraws = cm.gate_data(B, E, k, noisy, c["seed"])
        assert redraws <= 100, f"{tag}: {redraws} redraws"
        if noisy and B * E >= 2:
            assert bool((raw > 20).any()) and bool(((raw < 20) & (raw > 19)).any()), tag + ": no raw_noise on both sides of 20"
        dg, gl = cm.gate_bwd_inputs(c)
        ref = cm.gate_fwd64(clean, raw, z, k, noisy, grad=(dg, gl))
        assert ref["rel_gap"] >= cm.REL_MARGIN and ref["thr_gap"] >= cm.THR_MARGIN, f"{tag}: {ref['rel_gap']:.2e} {ref['thr_gap']:.2e}"
        for kk in ("gates", "p", "sigma", "loadrow", "loss", "d_imp", "d_load", "d_clean", "d_raw"):
            assert bool(torch.isfinite(ref[kk]).all()), f"{tag}: {kk} not finite"
        g2, ti, load, loss = _moe_py(clean, raw, z, k, noisy, cm._f32(cm.GATE_EPS), cm._f32(cm.GATE_COEF))
        _close(ref["gates"], g2, 1e-6, tag + " gates against moe.py")          # (moe.py adds the double 1e-6, 1e-10, the kernel's
        _close(ref["load"], load, 1e-12, tag + " load against moe.py")         # are float32 constants widened)
        assert torch.equal(ref["top"].long(), ti), tag + " top"
        if ref["loss"].abs().item() > 0:
            _close(ref["loss"], loss.reshape(1), 1e-5, tag + " loss against moe.py")
        # float32 takes the same decisions, the yardstick stays within its floors
        yard = cm.gate_fwd_yard(clean, raw, z, k, noisy)
        assert torch.equal(yard["top"], ref["top"]), tag + ": float32 selects differently"
        fl = cm.gate_aux_floors(ref, B, E)
        for kk in ("gates", "p", "sigma", "loadrow"):
            _yard_ok(f"{tag} {kk}", yard[kk], ref[kk])
        for kk in ("loss", "d_imp", "d_load"):
            if ref[kk].abs().max() > 0:
                _yard_ok(f"{tag} {kk}", yard[kk], ref[kk], fl[kk], reduced=(kk == "loss"))
            else:
                assert bool((yard[kk] == 0).all()), f"{tag} {kk}: not exactly 0"
        sv = cm.gate_saved32(ref)
        by = cm.gate_bwd_yard(clean, raw, sv, dg, gl, k, noisy)
        bf = cm.gate_bwd_floors(clean, raw, ref, dg, gl, k, noisy)
        for kk in ("d_clean", "d_raw"):
            if ref[kk].abs().max() > 0:
                _yard_ok(f"{tag} {kk}", by[kk], ref[kk], bf[kk])
            else:
                assert bool((by[kk] == 0).all()), f"{tag} {kk}: not exactly 0"
    assert {(c["E"], c["k"]) for c in cm.gate_cases()} == set(cm.GATE_EK) and {c["B"] for c in cm.gate_cases()} == set(cm.GATE_BS)


def test_gate_tie_rule():
    """equal logits, no noise: the documented rule takes the lowest indices first"""
    clean = torch.zeros(3, 4)
    clean[2] = torch.tensor([1.0, 2.0, 2.0, 1.0])
    ref = cm.gate_fwd64(clean, None, None, 2, 0)
    assert ref["top"].tolist() == [[0, 1, 2], [0, 1, 2], [1, 2, 0]]
    assert torch.equal(cm.gate_fwd_yard(clean, None, None, 2, 0)["top"], ref["top"])


# ----------------------------------------------------------------------------------------------------------------------
# combine, dispatch, rows, KAN pack
# ----------------------------------------------------------------------------------------------------------------------
def test_combine_reference_and_yardstick():
    for c in cm.combine_cases():
        gates, outs, dy = cm.combine_data(c)
        E = c["E"]
        assert bool((gates == 0).any()) or E == 1
        ref, yard = cm.combine_ref64(gates, outs, dy), cm.combine_yard(gates, outs, dy)
        safe = [torch.where(gates[:, e:e + 1] == 0, torch.zeros_like(o), o).double().requires_grad_(True) for e, o in enumerate(outs)]
        gd = gates.double().clone().requires_grad_(True)
        y = sum(gd[:, e:e + 1] * safe[e] for e in range(E))
        y.backward(dy.double())
        _close(ref["y"], y.detach(), 1e-14, c["tag"] + " y")
        live = gates != 0
        _close(torch.where(live, ref["dgates"], torch.zeros_like(ref["dgates"])), torch.where(live, gd.grad, torch.zeros_like(gd.grad)),
               1e-13, c["tag"] + " dgates")
        for e in range(E):
            _close(ref["douts"][e], safe[e].grad, 1e-14, c["tag"] + " douts")
        _yard_ok(c["tag"] + " y", yard["y"], ref["y"], cm.elem_floor(ref["terms"], E + 1))
        m = live.reshape(-1)
        _yard_ok(c["tag"] + " dgates", yard["dgates"].reshape(-1)[m], ref["dgates"].reshape(-1)[m], cm.sum_floor(ref["dterms"][:, m]), reduced=True)
    cs = cm.combine_cases()
    assert {c["E"] for c in cs} == {1, 3, 16} and {c["O"] for c in cs} == {1, 63, 64, 65, 200} and {c["B"] for c in cs} == {1, 5, 67}


def test_dispatch_reference():
    for c in cm.dispatch_cases():
        gates = cm.dispatch_data(c)
        idx, count = cm.dispatch_ref(gates)
        B, E = gates.shape
        assert count[0] == B
        if E >= 3:
            assert count[1] == 0 and count[2] == B // 2 and bool(torch.isnan(gates[:, 1]).any() or B < 3)
        for e in range(E):
            sel = idx[e, :count[e]].long()
            assert bool((gates[sel, e] > 0).all()) and bool((sel[1:] > sel[:-1]).all()) and bool((idx[e, count[e]:] == int(cm.SENT)).all())
            assert int((gates[:, e] > 0).sum()) == count[e]
    assert {c["B"] for c in cm.dispatch_cases()} == {1, 63, 64, 65, 129, 200}


def test_rows_and_kan_yardsticks():
    for c in cm.rows_cases():
        full, rows, idx, gates = cm.rows_data(c)
        assert idx.numel() == c["n"] and bool((idx[1:] > idx[:-1]).all())
        t = (full[idx.long()].double() * rows.double()).t()                # [D][n]: dgates[idx[i]] = <dy[idx[i]], src[i]>
        yard = torch.from_numpy(cm.seq_sum32((full[idx.long()] * rows).numpy(), 1))
        _yard_ok(c["tag"] + " dgates", yard, t.sum(0), cm.sum_floor(t), reduced=True)
    for i, (o, n, nb) in enumerate(cm.KAN_SHAPES):
        bw, sw, sc, dw = cm.kan_pack_data(o, n, nb, 1100 + i)
        r = cm.kan_unpack_ref(dw, sw, sc)
        _yard_ok(f"kan {o} {n} {nb} d_scaler", r["d_scaler_yard"], r["d_scaler"], cm.sum_floor(r["terms"]), reduced=True)
        # the packed weight against the reference model's expression (kan1.py scaled_spline_weight, torch.cat) in double
        wc = torch.cat([bw.double(), (sw.double() * sc.double()[:, :, None]).reshape(o, -1)], 1)
        _close(cm.kan_pack_ref32(bw, sw, sc), wc, 2.0 ** -23, "kan wcat")
        wcr = torch.cat([bw.double(), (sw.double() * sc.double()[:, :, None]).reshape(o, -1)], 1).requires_grad_(True)
        swd, scd, bwd_ = sw.double().requires_grad_(True), sc.double().requires_grad_(True), bw.double().requires_grad_(True)
        torch.cat([bwd_, (swd * scd[:, :, None]).reshape(o, -1)], 1).backward(dw.double())
        _close(r["d_base"], bwd_.grad, 0.0, "kan d_base")
        _close(r["d_spline"].reshape(o, n, nb), swd.grad, 2.0 ** -23, "kan d_spline")
        _close(r["d_scaler"], scd.grad, 1e-13, "kan d_scaler")
        del wcr
