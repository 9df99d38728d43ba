"""The downsample data gradient as a dense GEMM with a compact result (HAMSPINE_DS_COMPACT, csrc/blocks.hip: ds_compact).

bf16 mode writes the data gradient of a 1x1 stride-2 downsample convolution as [N][P][Q][Cin] -- only the even pixels, the
rest of the full-size gradient being structural zeros -- and the block's stage-0 data gradient gathers it as its residual
(GemmArgs.res_gather).  Nothing of the arithmetic changes: the same products are summed in the same order and an odd pixel
adds +0.0f where it used to add a stored zero, so every case compares HAMSPINE_DS_COMPACT=1 against =0 bit for bit, on the
input gradient and on every parameter gradient, and runs each setting twice."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from oracle.procedural import load_procedural  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(autouse=True)
def _restore():
    hamspine.set_compute_dtype("bf16")
    yield
    os.environ.pop("HAMSPINE_DS_COMPACT", None)
    os.environ.pop("HAMSPINE_XBLOCK_BN", None)
    hamspine.set_compute_dtype("bf16")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs by {(a[k].float() - b[k].float()).abs().max().item():.3e}"
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs in the sign of a zero"


def _ab(run):
    """run(): one forward + backward -> {name: gradient}.  Both settings, twice each, interleaved."""
    res = {}
    for rep in (0, 1):
        for setting in ("1", "0"):
            os.environ["HAMSPINE_DS_COMPACT"] = setting
            res[setting, rep] = run()
    _assert_same(res["1", 0], res["0", 0], "compact vs full-size")
    _assert_same(res["1", 1], res["1", 0], "compact, second run")
    _assert_same(res["0", 1], res["0", 0], "full-size, second run")
    return res["1", 0]


def _strided_block(kind, cin, planes, seed=11):
    import torch.nn as nn
    from hamspine.nn import resnet as pr
    blk = pr.Bottleneck if kind == "bottleneck" else pr.BasicBlock
    cout = planes * blk.expansion
    ds = nn.Sequential(pr.ConvParams(cin, cout, 1, 2), pr.BatchNormParams(cout))
    return load_procedural(blk(cin, planes, 2, ds), seed).to(DEV).train()


def _block_run(p, x, cot):
    def run():
        p.zero_grad(set_to_none=True)
        xp = x.clone().requires_grad_(True)
        y = p(xp)
        (y.float() * cot).sum().backward()
        torch.cuda.synchronize()
        out = {"dx": xp.grad.detach().clone()}
        out.update({k: q.grad.detach().clone() for k, q in p.named_parameters()})
        return out
    return run


def _inputs(n, cin, hw, cout, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, hw, hw, generator=g).to(DEV).to(BF).contiguous(memory_format=torch.channels_last)
    po = (hw - 1) // 2 + 1
    cot = torch.randn(n, cout, po, po, generator=g).to(DEV)
    return x, cot


@pytest.mark.parametrize("n,hw", [
    (2, 8),      # consumer 128 rows; the compact result has 32: less than one tile, generic epilogue
    (3, 12),     # 432 rows: edge tiles in the dense GEMM and in the consumer
    (4, 16),     # 1024 rows: full tiles, the branch-free epilogue case
    (2, 7),      # odd extent: the full-size route is not parity-ordered, P = 4
])
def test_bottleneck_first_block(n, hw):
    """64 -> planes 64 -> 256 with a stride-2 downsample, train-mode BatchNorm: the consumer is the 1x1 stage-0 data gradient"""
    p = _strided_block("bottleneck", 64, 64)
    x, cot = _inputs(n, 64, hw, 256)
    out = _ab(_block_run(p, x, cot))
    assert out["dx"].dtype == BF and out["dx"].float().abs().max().item() > 0


def test_switch_selects_the_route(tmp_path):
    """what the comparisons above rest on: under =1 the backward launches the dense [N*P*Q x Cin x Cout] GEMM and no 1x1
    stride-2 data-gradient convolution, under =0 the reverse (the library's per-launch records)"""
    from hamspine import _lib as L
    lib = L.lib()
    p = _strided_block("bottleneck", 128, 64)       # (128 input channels: no other GEMM of the block has the dense one's shape)
    x, cot = _inputs(4, 128, 16, 256)
    run = _block_run(p, x, cot)
    seen = {}
    for setting in ("1", "0"):
        os.environ["HAMSPINE_DS_COMPACT"] = setting
        run()
        lib.hs_prof_enable(1)
        try:
            run()
            path = str(tmp_path / f"launches{setting}.csv")
            L.check(lib.hs_prof_dump(path.encode()), "hs_prof_dump")
        finally:
            lib.hs_prof_enable(0)
        rows = [ln.strip().split(",") for ln in open(path) if ln.strip() and ln[0].isdigit()]
        # class, operand combo, tile cfg, M, N, K, batch, split_k, filter R, stride, ms
        seen[setting] = [tuple(int(float(v)) for v in r[:10]) for r in rows]
    dense = lambda r: r[0] == 0 and r[3:6] == (4 * 8 * 8, 128, 256)          # noqa: E731
    strided = lambda r: r[0] == 1 and r[8] == 1 and r[9] == 2 and r[3:6] == (4 * 16 * 16, 128, 256)   # noqa: E731
    assert sum(map(dense, seen["1"])) == 1 and sum(map(strided, seen["1"])) == 0, seen["1"]
    assert sum(map(dense, seen["0"])) == 0 and sum(map(strided, seen["0"])) == 1, seen["0"]


def test_basic_block_parity_ordered_consumer():
    """BasicBlock 64 -> 128, stride 2: the consumer is the 3x3 stride-2 data gradient, whose parity-ordered rows m < quarter
    are the compact rows in order"""
    p = _strided_block("basic", 64, 128)
    x, cot = _inputs(2, 64, 8, 128)
    _ab(_block_run(p, x, cot))


def test_basic_block_odd_extent():
    """the same block on a 7x7 grid: the 3x3 stride-2 consumer walks its rows in natural order and divides"""
    p = _strided_block("basic", 64, 128)
    x, cot = _inputs(2, 64, 7, 128)
    _ab(_block_run(p, x, cot))


def _two_block_tower(planes2):
    """stem + one identity-free bottleneck (64 -> 256, stride 1) + the downsample block (256 -> planes2 -> 4 planes2, stride 2)"""
    import torch.nn as nn
    from hamspine.nn import resnet as pr
    m = pr.ResNet(pr.Bottleneck, [1, 1, 1, 1], num_classes=8)
    ds = nn.Sequential(pr.ConvParams(256, 4 * planes2, 1, 2), pr.BatchNormParams(4 * planes2))
    m.layer2 = nn.Sequential(pr.Bottleneck(256, planes2, 2, ds))
    m.layer3 = nn.Sequential()
    m.layer4 = nn.Sequential()
    m.fc = nn.Identity()
    return load_procedural(m, 5).to(DEV).train()


@pytest.mark.parametrize("xblock,planes2", [
    ("0", 128),      # the ordinary epilogue reads the compact residual
    ("2", 128),      # the block-output rider reads it: prefetch in front of the K walk
    ("2", 1024),     # K = 1024 under 8 output tiles: a split-K launch, the rider's fallback read
])
def test_two_block_tower(xblock, planes2):
    """N = 2, 32x32 image -> 8x8 block input, through the tower executor (the cross-block BatchNorm sums exist only there)"""
    from hamspine import tower
    os.environ["HAMSPINE_XBLOCK_BN"] = xblock
    m = _two_block_tower(planes2)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 3, 32, 32, generator=g).to(DEV)
    cot = torch.randn(2, 4 * planes2, 4, 4, generator=g).to(DEV)
    names = {id(q): k for k, q in m.named_parameters()}
    params, _ = tower.resnet_params(m)

    def run():
        m.zero_grad(set_to_none=True)
        taps = tower.resnet_taps(m, x, ("layer2",))
        assert taps is not None, "the tower executor did not take the model"
        (taps[0].float() * cot).sum().backward()
        torch.cuda.synchronize()
        return {names[id(q)]: q.grad.detach().clone() for q in params}
    out = _ab(run)
    assert out["layer1.0.conv1.weight"].abs().max().item() > 0


def test_negative_zero_accumulator_at_odd_pixels():
    """An odd pixel adds +0.0f, it does not skip the addition: a -0 accumulator must leave as +0, as it does against the
    stored zeros of the full-size route.  The MFMA chain starts at +0, so a -0 accumulator can only come from a negative
    underflow: the stage-0 filter is +-2^-100 and the cotangent is scaled by 2^-90, so every product of the stage-0 data
    gradient lies near 2^-185 and each accumulator rounds to +-0 with the sign of its exact sum.  Odd pixels of dx are then
    zeros, and none may carry a sign bit -- under either setting; even pixels hold the downsample gradient."""
    p = _strided_block("bottleneck", 64, 64)
    with torch.no_grad():
        w = p.conv1.weight
        sign = torch.where(torch.randn(w.shape, generator=torch.Generator().manual_seed(9)) < 0, -1.0, 1.0).to(w.device)
        w.copy_((sign * 2.0 ** -100).contiguous(memory_format=torch.channels_last))
    x, cot = _inputs(4, 64, 16, 256)
    cot = cot * 2.0 ** -90
    res = {}
    run = _block_run(p, x, cot)
    for setting in ("1", "0"):
        os.environ["HAMSPINE_DS_COMPACT"] = setting
        res[setting] = run()
    _assert_same(res["1"], res["0"], "compact vs full-size")
    for setting in ("1", "0"):
        dx = res[setting]["dx"]                       # (N, C, H, W)-shaped, bf16
        odd = torch.zeros(16, 16, dtype=torch.bool, device=dx.device)
        odd[1::2, :] = True
        odd[:, 1::2] = True
        at_odd = dx.permute(0, 2, 3, 1)[:, odd]
        assert (at_odd == 0).all(), "the stage-0 products did not underflow: the case does not reach a zero accumulator"
        assert not torch.signbit(at_odd).any(), f"HAMSPINE_DS_COMPACT={setting}: -0 stored at an odd pixel"
        assert dx.permute(0, 2, 3, 1)[:, ~odd].float().abs().max().item() > 0
