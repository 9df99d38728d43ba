"""MuonWithAuxAdam, host side (reference scripts/train.py:262-307): properties of the float64 restatement of the
specification (tests/muon_ref.py) that need no source to check against, and the optimizer's constructor, defaults, state
layout and refusal of CPU tensors."""
import pytest
import torch

import muon_ref as mr

F64 = torch.float64


def _gauss(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


@pytest.mark.parametrize("shape", [(72, 200), (200, 72), (96, 576), (64, 147)])
def test_newton_schulz_brings_every_singular_value_near_one(shape):
    sv = torch.linalg.svdvals(mr.newton_schulz(_gauss(shape, 11)))
    print(shape, float(sv.min()), float(sv.max()))
    assert sv.min() >= 0.65 and sv.max() <= 1.25, (shape, float(sv.min()), float(sv.max()))


def test_newton_schulz_commutes_with_column_permutations():
    """why a channels_last filter is read as its memory lies: (K, R S C) is a column permutation of (K, C R S)"""
    for shape, seed in (((64, 147), 3), ((200, 72), 4)):
        U = _gauss(shape, seed)
        perm = torch.randperm(shape[1], generator=torch.Generator().manual_seed(5))
        d = (mr.newton_schulz(U[:, perm]) - mr.newton_schulz(U)[:, perm]).abs().max().item()
        assert d <= 1e-12, (shape, d)


def test_newton_schulz_of_a_tall_matrix_is_the_transpose_of_the_wide_one():
    U = _gauss((200, 72), 6)
    d = (mr.newton_schulz(U) - mr.newton_schulz(U.T.contiguous()).T).abs().max().item()
    assert d <= 1e-12, d


def test_one_optimizer_step_on_a_2x3_parameter_by_hand():
    """momentum 0.5, first step (m = 0): m = g / 2, u = g + (m - g) / 2 = 0.75 g.  With g of rank one, g = x y^T with |x| = |y| =
    1 (up to the 1e-7 of the normalisation), the iteration acts on the one singular value: s <- a s + b s^3 + c s^5, from s = 1."""
    x = torch.tensor([0.6, 0.8], dtype=F64)
    y = torch.tensor([1.0, 2.0, 2.0], dtype=F64) / 3.0
    g = torch.outer(x, y) * 4.0
    p = torch.nn.Parameter(torch.tensor([[1.0, -2.0, 3.0], [0.5, 0.25, -1.0]], dtype=F64))
    p0 = p.detach().clone()
    p.grad = g.clone()
    opt = mr.RefMuonWithAuxAdam([dict(params=[p], use_muon=True, lr=0.1, momentum=0.5, weight_decay=0.2)])
    opt.step()
    a, b, c = mr.NS_COEFFS
    s = 1.0
    for _ in range(5):
        s = a * s + b * s ** 3 + c * s ** 5
    want = p0 * (1 - 0.1 * 0.2) - 0.1 * 1.0 * s * torch.outer(x, y)      # shape[-2] / shape[-1] = 2 / 3 -> scale 1
    assert (p.detach() - want).abs().max().item() <= 1e-6
    assert (opt.state[p]["momentum_buffer"] - 0.5 * g).abs().max().item() <= 1e-15
    # a tall parameter scales its update by sqrt(rows / cols)
    assert mr.muon_scale((300, 7)) == (300 / 7) ** 0.5 and mr.muon_scale((128, 64, 1, 1)) == 1.0 and mr.muon_scale((64, 3, 3, 3)) == 1.0


# ---------------------------------------------------------------------------------------------- the product optimizer
def _params():
    w = torch.nn.Parameter(torch.zeros(4, 6))
    f = torch.nn.Parameter(torch.zeros(8, 3, 3, 3))
    b = torch.nn.Parameter(torch.zeros(6))
    return w, f, b


def test_the_top_level_muon_module_exports_the_optimizer_only():
    import muon
    import hamspine.optim as ho
    assert muon.MuonWithAuxAdam is ho.MuonWithAuxAdam
    assert muon.__all__ == ["MuonWithAuxAdam"]
    assert issubclass(muon.MuonWithAuxAdam, torch.optim.Optimizer)


def test_constructor_validation():
    from muon import MuonWithAuxAdam
    w, f, b = _params()
    with pytest.raises(ValueError):
        MuonWithAuxAdam([dict(params=[w, f]), dict(params=[b], use_muon=False)])          # a group without use_muon
    with pytest.raises(ValueError):
        MuonWithAuxAdam([dict(params=[w, b], use_muon=True)])                               # a 1-D parameter in a Muon group
    MuonWithAuxAdam([dict(params=[w, f], use_muon=True), dict(params=[b], use_muon=False)])


def test_defaults_are_those_of_the_published_package():
    from muon import MuonWithAuxAdam
    w, f, b = _params()
    opt = MuonWithAuxAdam([dict(params=[w, f], use_muon=True), dict(params=[b], use_muon=False)])
    gm, ga = opt.param_groups
    assert (gm["lr"], gm["momentum"], gm["weight_decay"], gm["use_muon"]) == (0.02, 0.95, 0.0, True)
    assert (ga["lr"], tuple(ga["betas"]), ga["eps"], ga["weight_decay"], ga["use_muon"]) == (3e-4, (0.9, 0.95), 1e-10, 0.0, False)
    # the group list of scripts/train.py:297-306 keeps what it sets
    opt = MuonWithAuxAdam([dict(params=[w, f], use_muon=True, lr=0.03, weight_decay=0.01),
                           dict(params=[b], use_muon=False, lr=1e-3, betas=(0.8, 0.9), weight_decay=0.02)])
    gm, ga = opt.param_groups
    assert (gm["lr"], gm["momentum"], gm["weight_decay"]) == (0.03, 0.95, 0.01)
    assert (ga["lr"], tuple(ga["betas"]), ga["eps"], ga["weight_decay"]) == (1e-3, (0.8, 0.9), 1e-10, 0.02)


def test_state_dict_keys():
    from muon import MuonWithAuxAdam
    w, f, b = _params()
    opt = MuonWithAuxAdam([dict(params=[w, f], use_muon=True), dict(params=[b], use_muon=False)])
    sd = opt.state_dict()
    assert sd["state"] == {} and [g["params"] for g in sd["param_groups"]] == [[0, 1], [2]]
    assert [g["use_muon"] for g in sd["param_groups"]] == [True, False]
    # a state in the documented layout loads, and comes back under the same keys
    sd["state"] = {0: {"momentum_buffer": torch.ones(4, 6)}, 1: {"momentum_buffer": torch.ones(8, 3, 3, 3)},
                   2: {"step": torch.tensor(3.0), "exp_avg": torch.ones(6), "exp_avg_sq": torch.ones(6)}}
    opt.load_state_dict(sd)
    back = opt.state_dict()["state"]
    assert set(back[0]) == {"momentum_buffer"} and set(back[1]) == {"momentum_buffer"}
    assert set(back[2]) == {"step", "exp_avg", "exp_avg_sq"}


def test_cpu_tensors_are_refused_at_step():
    import hamspine
    from muon import MuonWithAuxAdam
    w, f, b = _params()
    for group in ([dict(params=[w, f], use_muon=True)], [dict(params=[b], use_muon=False)]):
        opt = MuonWithAuxAdam(group)
        for p in group[0]["params"]:
            p.grad = torch.ones_like(p)
        with pytest.raises(hamspine.HamspineError, match="no CPU fallback"):
            opt.step()
    assert float(w.detach().abs().max()) == 0.0 and float(b.detach().abs().max()) == 0.0
