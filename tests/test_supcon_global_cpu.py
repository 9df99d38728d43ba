"""SupCon over the global batch, the parts that need no GPU: the gradient scaling convention of supcon_loss(group=...) shown
in float64 with plain autograd, the block-wise yardstick against head_ref's, the a-priori floors of the tiled kernels on every
case of the GPU test, and the workspace formula of hs_supcon_tiled."""
import numpy as np
import torch

import head_ref as hr
import kernel_ref as kr
import supcon_global_ref as sg

F64 = torch.float64


def _supcon64(feat, labels, T):
    """SupConLoss in float64, differentiable (the formula of head_ref.supcon_ref64)"""
    B = feat.shape[0]
    fn = feat / feat.norm(dim=1, keepdim=True).clamp_min(hr.E12)
    sim = fn @ fn.T / T
    sim = sim - sim.max(1, keepdim=True).values.detach()
    off = ~torch.eye(B, dtype=torch.bool)
    pos = (off & (labels[:, None] == labels[None, :])).double()
    logp = sim - torch.log((sim.exp() * off.double()).sum(1, keepdim=True) + hr.E8)
    return -((pos * logp).sum(1) / (pos.sum(1) + hr.E8)).mean()


def test_two_rank_scaling_identity():
    """Two "ranks" own 37 rows each of the features of one shared linear layer.  Rank r back-propagates world * (its rows of
    d loss_global / d features) -- what supcon_loss(group=..., average_across_ranks=True) hands to autograd -- and the
    parameter gradients are averaged, as DataParallel does.  The average is the gradient of the concatenated-batch loss."""
    g = kr.gen(31)
    W, B, T = 2, 37, 0.07
    x = torch.randn(W * B, 48, generator=g, dtype=F64)
    y = torch.randint(0, 7, (W * B,), generator=g)
    lin = torch.nn.Linear(48, 65).double()
    with torch.no_grad():
        lin.weight.copy_(torch.randn(65, 48, generator=g, dtype=F64) * 0.2)
        lin.bias.copy_(torch.randn(65, generator=g, dtype=F64) * 0.1)
    lin.zero_grad()
    _supcon64(lin(x), y, T).backward()
    want = [lin.weight.grad.clone(), lin.bias.grad.clone()]
    # the gathered features carry no graph; the global gradient with respect to them
    feat_all = lin(x).detach().requires_grad_(True)
    loss_all = _supcon64(feat_all, y, T)
    loss_all.backward()
    got = [torch.zeros_like(want[0]), torch.zeros_like(want[1])]
    rank_losses = []
    for r in range(W):
        lin.zero_grad()
        rows = slice(r * B, (r + 1) * B)
        lin(x[rows]).backward(W * feat_all.grad[rows])
        got[0] += lin.weight.grad / W
        got[1] += lin.bias.grad / W
        rank_losses.append(_supcon64(lin(x[rows]).detach(), y[rows], T).item())
    for a, b, name in zip(got, want, ("weight", "bias")):
        err = (a - b).abs().max().item() / b.abs().max().item()
        assert err <= 1e-12, f"{name}: averaged rank gradients off the concatenated-batch gradient by {err:.3e}"
    # and the objective itself differs: the mean of the rank losses is not the global loss
    assert abs(np.mean(rank_losses) - loss_all.item()) > 1e-3 * abs(loss_all.item())


def test_blocked_yardstick_is_the_yardstick_bitwise():
    for c in sg.tiled_cases():
        f, lab, T = c["feat"], c["labels"], c["T"]
        N, D = f.shape
        if N * N * D > 1 << 21:
            continue
        whole = hr.supcon_yard(f, lab, T)
        for max_elems in (1, 3 * N * D, 1 << 22):           # one anchor per block, three, all
            blocked = sg.supcon_yard_blocked(f, lab, T, max_elems=max_elems)
            for k in ("loss", "dfeat"):
                assert kr.bits_equal(whole[k], blocked[k]), f"{c['tag']} {k}: block-wise yardstick differs (max_elems {max_elems})"


def test_cases_cover_the_issue_and_the_tile_edges():
    shapes = {tuple(c["feat"].shape) for c in sg.tiled_cases()}
    assert {(1, 1), (2, 1), (63, 5), (64, 64), (65, 65), (129, 130), (257, 3), (300, 257), (513, 260), (70, 1024)} <= shapes
    assert sg.MULTI in shapes and sg.key_splits(sg.MULTI[0])[0] == 2 and sg.key_splits(1024)[0] == 1
    assert {c["T"] for c in sg.tiled_cases()} == {0.07, 0.5}
    assert {c["pattern"] for c in sg.tiled_cases()} == set(sg.PATTERNS)
    assert sum("dup" in c["tag"] for c in sg.tiled_cases()) == 2 and sum("near" in c["tag"] for c in sg.tiled_cases()) == 2


def test_floors_are_finite_and_above_noise():
    for c in sg.tiled_cases():
        f, lab, T = c["feat"], c["labels"], c["T"]
        ref = hr.supcon_ref64(f, lab, T)
        assert all(bool(torch.isfinite(v).all()) for v in ref.values()), c["tag"]
        fl = sg.supcon_tiled_floors(f, lab, T, ref)
        for k in ("loss", "dfeat", "dfeat_abs"):
            assert np.isfinite(fl[k]) and fl[k] >= 0.0, f"{c['tag']}: floor {k} = {fl[k]}"
        for k in ("loss", "dfeat"):
            assert fl[k] >= kr.F32_NOISE, f"{c['tag']}: floor {k} = {fl[k]}"
        if c["pattern"] == "distinct":
            assert ref["loss"].item() == 0.0 and bool((ref["dfeat"] == 0).all())


def test_workspace_formula_and_abi():
    from hamspine import _lib as L
    h = L.parse_header(open(L.HEADER_PATH).read())
    assert h.prototypes["hs_supcon_tiled_ws_bytes"] == ("int64_t", ["int32_t", "int32_t"])
    ret, params = h.prototypes["hs_supcon_tiled"]
    assert ret == "hs_status" and len(params) == 12
    max_n, max_d = h.constants["HS_SUPCON_TILED_MAX_N"], h.constants["HS_SUPCON_TILED_MAX_D"]
    assert max_n == 65536 and max_d >= 2048
    # the single-workgroup entries are declared as before
    assert len(h.prototypes["hs_supcon_loss"][1]) == 9 and h.prototypes["hs_supcon_ws_bytes"] == ("int64_t", ["int32_t", "int32_t"])
    lib = L.lib()                                                # loads without a GPU: the helper is host code
    ws = lib.hs_supcon_tiled_ws_bytes
    for N, D in ((1, 1), (37, 65), (65, 3), (130, 70), (513, 260), (4096, 128), (8192, 128), (32769, 5), (65536, max_d)):
        Dp, (tps, KS) = -(-D // 4) * 4, sg.key_splits(N)
        assert 1 <= KS <= 16 and (KS - 1) * tps < -(-N // 64) <= KS * tps           # every run holds a tile
        assert ws(N, D) == 4 * (N * Dp + 6 * N + (KS * N * (Dp + 5) if KS > 1 else 0))
    assert sg.key_splits(64) == (1, 1) and sg.key_splits(65) == (1, 2) and sg.key_splits(32769)[1] == 1
    assert ws(8192, 128) < 4 * ws(4096, 128)                     # no N^2 term
    for N, D in ((0, 8), (8, 0), (max_n + 1, 8), (8, max_d + 1), (-1, 8)):
        assert ws(N, D) == -1
