"""The lean image-tower passes (HAMSPINE_IMG_LEAN, csrc/blocks.hip: img_lean; kernels in csrc/norm.hip).

In bf16 mode four full-size tensors are no longer written to memory for the next elementwise kernel to read back: the stem's
relu(bn(c)) (bit 0: pooled straight from c), the stem's un-pooled gradient map (bit 1: gathered in registers by the BatchNorm
backward), a block's downsample identity (bit 2: formed inside the block output's apply pass) and the gradient that enters the
downsample BatchNorm backward (bit 3: one partial / final / apply pass serves both BatchNorms).  No sum changes its terms or
their order and every value that used to cross memory as bf16 is rounded to bf16 in registers, so every case compares the
default (bits 0, 2, 3: bit 1 measured no gain and stays off) and 15 (all four) against HAMSPINE_IMG_LEAN=0 (the separate
launches) BIT FOR BIT, each setting run twice."""
import os

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from oracle.procedural import load_procedural  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
SWITCH = "HAMSPINE_IMG_LEAN"


@pytest.fixture(autouse=True)
def _restore():
    hamspine.set_compute_dtype("bf16")
    os.environ.pop(SWITCH, None)
    yield
    os.environ.pop(SWITCH, None)
    os.environ.pop("HAMSPINE_XBLOCK_BN", None)
    hamspine.set_compute_dtype("bf16")


def _set(setting):
    if setting is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = setting


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, f"{what}: {k} changed shape or dtype"
        assert torch.equal(_bits(a[k]), _bits(b[k])), \
            f"{what}: {k} differs by {(a[k].float() - b[k].float()).abs().max().item():.3e}"


def _ab(run, lean=(None, "15")):
    """run() -> {name: tensor}.  Every lean setting (None = the default, "15" = all four parts) against 0, each setting twice,
    interleaved."""
    settings = tuple(lean) + ("0",)
    res = {}
    for rep in (0, 1):
        for setting in settings:
            _set(setting)
            res[setting, rep] = run()
    _set(None)
    for setting in settings:
        _assert_same(res[setting, 0], res["0", 0], f"{SWITCH}={setting} vs 0")
        _assert_same(res[setting, 1], res[setting, 0], f"{SWITCH}={setting}, second run")
    return res[settings[0], 0]


def _reset_running(m):
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.running_mean.zero_()
            mod.running_var.fill_(1.0)


def _running(m):
    out = {}
    for k, mod in m.named_modules():
        if isinstance(mod, nn.BatchNorm2d):
            out[k + ".running_mean"] = mod.running_mean.detach().clone()
            out[k + ".running_var"] = mod.running_var.detach().clone()
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# stem
# ---------------------------------------------------------------------------------------------------------------------------
def _align(n, a=256):
    return (n + a - 1) // a * a


def _stem_arena(n, h, w, cout, es):
    """byte offsets of the stem composite's saved arena (csrc/blocks.hip: stem_layout; every buffer starts on 256 bytes)"""
    p, q = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    hp = max(h + 6, 2 * p + 5)
    wp = (max(w + 6, 2 * q + 6) + 1) // 2 * 2
    p2, q2 = (p + 2 - 3) // 2 + 1, (q + 2 - 3) // 2 + 1
    off, o = {}, 0
    for name, size in (("packed", n * hp * wp * 4 * es), ("w", cout * 7 * 32 * es), ("c", n * p * q * cout * es),
                       ("a", n * p * q * cout * es), ("idx", n * p2 * q2 * cout), ("stats", cout * 4 * 4)):
        off[name] = o
        o += _align(size)
    off["end"] = o
    return off, (p, q, p2, q2)


def _stem(cout, seed=2):
    from hamspine.nn import resnet as pr
    s = pr.Stem(pr.ConvParams(3, cout, 7, 2, 3), pr.BatchNormParams(cout), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1))
    return load_procedural(s, seed).to(DEV).train()


def _stem_run(s, x, cot, es=2):
    n, _, h, w = x.shape
    cout = s[0].out_channels
    off, (p, q, p2, q2) = _stem_arena(n, h, w, cout, es)

    def run():
        s.zero_grad(set_to_none=True)
        _reset_running(s)
        y = s(x)
        saved = y.grad_fn.saved_tensors[4]
        assert saved.dtype == torch.uint8 and saved.numel() >= off["end"], "the saved arena is not laid out as this test assumes"
        out = {"y": y.detach().clone(),
               "argmax": saved[off["idx"]:off["idx"] + n * p2 * q2 * cout].clone().view(n, p2, q2, cout)}
        (y.float() * cot).sum().backward()
        torch.cuda.synchronize()
        out.update({"d_" + k: v.grad.detach().clone() for k, v in s.named_parameters()})
        out.update(_running(s))
        return out
    return run, (p, q, p2, q2)


def _stem_inputs(n, h, w, cout, seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, h, w, generator=g).to(DEV)
    p, q = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    cot = torch.randn(n, cout, (p - 1) // 2 + 1, (q - 1) // 2 + 1, generator=g)
    cot = torch.where(cot.abs() < 2.0 ** -6, torch.ones_like(cot), cot).to(DEV)     # nonzero at every position, also as bf16
    return x, cot


def _window_counts(argmax, p, q):
    """how many pooling windows chose each pixel of the [N][P][Q][C] map"""
    n, p2, q2, c = argmax.shape
    t = argmax.long()
    hh = 2 * torch.arange(p2, device=t.device).view(1, p2, 1, 1) - 1 + t // 3
    ww = 2 * torch.arange(q2, device=t.device).view(1, 1, q2, 1) - 1 + t % 3
    assert (hh >= 0).all() and (hh < p).all() and (ww >= 0).all() and (ww < q).all(), "an arg-max tap points outside the map"
    nn_ = torch.arange(n, device=t.device).view(n, 1, 1, 1).expand_as(t)
    cc = torch.arange(c, device=t.device).view(1, 1, 1, c).expand_as(t)
    flat = ((nn_ * p + hh) * q + ww) * c + cc
    return torch.zeros(n * p * q * c, dtype=torch.long, device=t.device).scatter_add_(0, flat.reshape(-1),
                                                                                      torch.ones_like(flat).reshape(-1))


@pytest.mark.parametrize("n,h,w,cout", [
    (2, 32, 32, 64),     # 16x16 map, 8x8 pooled: windows clipped at the top and left borders
    (3, 30, 30, 16),     # 15x15 map: the last window of a row / column lies partly outside; two channel chunks
    (2, 38, 26, 64),     # 19x13 map, not square
])
def test_stem(n, h, w, cout):
    """pooled output, arg-max bytes, running statistics, dw / dgamma / dbeta; the cotangent is nonzero everywhere, and the arg-max
    map must hold pixels chosen by two and by four windows (the gather's sums of several terms)"""
    s = _stem(cout)
    x, cot = _stem_inputs(n, h, w, cout)
    run, (p, q, _, _) = _stem_run(s, x, cot)
    out = _ab(run)
    assert int(out["argmax"].max()) <= 8
    counts = _window_counts(out["argmax"], p, q)
    assert (counts == 2).any() and (counts == 4).any(), "no pixel was chosen by two / by four windows: the case proves nothing"
    assert out["d_0.weight"].abs().max().item() > 0 and out["y"].dtype == BF


def test_stem_all_zero_windows():
    """beta strongly negative: most windows are all zeros after the ReLU, and the first tap inside the map must win the tie"""
    s = _stem(64)
    with torch.no_grad():
        s[1].bias.fill_(-1.5)
        s[1].weight.fill_(1.0)
    x, cot = _stem_inputs(2, 32, 32, 64)
    run, _ = _stem_run(s, x, cot)
    out = _ab(run)
    zero_windows = (out["y"].permute(0, 2, 3, 1) == 0)
    assert zero_windows.float().mean().item() > 0.3 and not zero_windows.all(), "the case does not reach the tie rule"
    inner = out["argmax"][:, 1:, 1:, :][zero_windows[:, 1:, 1:, :]]
    assert (inner == 0).all(), "an all-zero window away from the border must keep its first tap"


def test_stem_single_bits():
    """each stem bit alone: the forward without the lean backward and the reverse"""
    s = _stem(64)
    x, cot = _stem_inputs(2, 38, 26, 64)
    run, _ = _stem_run(s, x, cot)
    _ab(run, ("1", "2"))


def test_switch_between_forward_and_backward():
    """the forward under one setting, the backward under the other: no backward may read a buffer only some forward writes"""
    s = _stem(64)
    blk = _ds_block("bottleneck", 64, 64, 1)
    x, cot = _stem_inputs(2, 32, 32, 64)
    cot = torch.randn(2, 256, 8, 8, generator=torch.Generator().manual_seed(8)).to(DEV)

    def run(fwd, bwd):
        for m in (s, blk):
            m.zero_grad(set_to_none=True)
            _reset_running(m)
        _set(fwd)
        y = blk(s(x))
        _set(bwd)
        (y.float() * cot).sum().backward()
        torch.cuda.synchronize()
        _set(None)
        out = {"y": y.detach().clone()}
        out.update({"stem." + k: v.grad.detach().clone() for k, v in s.named_parameters()})
        out.update({"blk." + k: v.grad.detach().clone() for k, v in blk.named_parameters()})
        return out
    ref = run("0", "0")
    _assert_same(run("15", "0"), ref, "lean forward, plain backward")
    _assert_same(run("0", "15"), ref, "plain forward, lean backward")
    _assert_same(run("15", "15"), ref, "lean both")
    _assert_same(run(None, "2"), ref, "default forward, stem-only lean backward")


# ---------------------------------------------------------------------------------------------------------------------------
# blocks with a downsample branch
# ---------------------------------------------------------------------------------------------------------------------------
def _ds_block(kind, cin, planes, stride, seed=11):
    from hamspine.nn import resnet as pr
    blk = pr.Bottleneck if kind == "bottleneck" else pr.BasicBlock
    cout = planes * blk.expansion
    ds = nn.Sequential(pr.ConvParams(cin, cout, 1, stride), pr.BatchNormParams(cout))
    return load_procedural(blk(cin, planes, stride, ds), seed).to(DEV).train()


def _block_run(p, x, cot):
    def run():
        p.zero_grad(set_to_none=True)
        _reset_running(p)
        xp = x.clone().requires_grad_(True)
        y = p(xp)
        (y.float() * cot).sum().backward()
        torch.cuda.synchronize()
        out = {"y": y.detach().clone(), "dx": xp.grad.detach().clone()}
        out.update({"d_" + k: q.grad.detach().clone() for k, q in p.named_parameters()})
        out.update(_running(p))
        return out
    return run


def _block_inputs(n, cin, hw, cout, stride, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, hw, hw, generator=g).to(DEV).to(BF).contiguous(memory_format=torch.channels_last)
    po = (hw - 1) // stride + 1
    cot = torch.randn(n, cout, po, po, generator=g).to(DEV)
    return x, cot


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind,cin,planes,stride,hw", [
    ("bottleneck", 64, 64, 1, 8),       # layer1.0's shape: 256 output channels, 32 chunk columns, 8 rows per workgroup pass
    ("bottleneck", 64, 64, 1, 12),      # 288 / 432 rows: more than one row block, a tail in the two-rows-in-flight loop
    ("bottleneck", 256, 128, 2, 8),     # 512 output channels: 64 chunk columns, the LDS-only column reduction
    ("bottleneck", 256, 128, 2, 7),     # odd extent, 4x4 output: 32 / 48 rows
    ("basic", 64, 128, 2, 8),           # BasicBlock: two main stages, 16 chunk columns
    ("basic", 64, 128, 2, 7),
])
def test_downsample_block(kind, cin, planes, stride, hw, n):
    """block output, dx, every parameter gradient, running statistics (single blocks make their own sums: bit 3 runs)"""
    p = _ds_block(kind, cin, planes, stride)
    cout = planes * (4 if kind == "bottleneck" else 1)
    x, cot = _block_inputs(n, cin, hw, cout, stride)
    out = _ab(_block_run(p, x, cot))
    assert out["dx"].dtype == BF and out["dx"].float().abs().max().item() > 0
    assert out["d_downsample.1.weight"].abs().max().item() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# tower
# ---------------------------------------------------------------------------------------------------------------------------
def _two_block_tower():
    """stem + a stride-1 bottleneck with a downsample branch (64 -> 256) + a stride-2 one (256 -> 128 -> 512)"""
    from hamspine.nn import resnet as pr
    m = pr.ResNet(pr.Bottleneck, [1, 1, 1, 1], num_classes=8)
    ds = nn.Sequential(pr.ConvParams(256, 512, 1, 2), pr.BatchNormParams(512))
    m.layer2 = nn.Sequential(pr.Bottleneck(256, 128, 2, ds))
    m.layer3 = nn.Sequential()
    m.layer4 = nn.Sequential()
    m.fc = nn.Identity()
    return load_procedural(m, 5).to(DEV).train()


def _tower_run(m, x, cot):
    from hamspine import tower
    names = {id(q): k for k, q in m.named_parameters()}
    params, _ = tower.resnet_params(m)

    def run():
        m.zero_grad(set_to_none=True)
        _reset_running(m)
        taps = tower.resnet_taps(m, x, ("layer2",))
        assert taps is not None, "the tower executor did not take the model"
        out = {"tap": taps[0].detach().clone()}
        (taps[0].float() * cot).sum().backward()
        torch.cuda.synchronize()
        out.update({"d_" + names[id(q)]: q.grad.detach().clone() for q in params})
        out.update(_running(m))
        return out
    return run


def _tower_inputs():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 3, 32, 32, generator=g).to(DEV)
    cot = torch.randn(2, 512, 4, 4, generator=g).to(DEV)
    return x, cot


@pytest.mark.parametrize("xblock", [
    "0",      # every block makes its own last-stage sums: bit 3 runs in both blocks
    "2",      # layer1.0's sums come from layer2.0's data-gradient GEMM: bit 3 stands aside there and runs in layer2.0
])
def test_two_block_tower(xblock):
    os.environ["HAMSPINE_XBLOCK_BN"] = xblock
    m = _two_block_tower()
    out = _ab(_tower_run(m, *_tower_inputs()))
    assert out["d_conv1.weight"].abs().max().item() > 0 and out["d_layer1.0.downsample.1.weight"].abs().max().item() > 0


@pytest.mark.parametrize("bit", ["1", "2", "4", "8"])
def test_two_block_tower_single_bit(bit):
    m = _two_block_tower()
    _ab(_tower_run(m, *_tower_inputs()), (bit,))


# ---------------------------------------------------------------------------------------------------------------------------
# f32 mode keeps its route and its buffers
# ---------------------------------------------------------------------------------------------------------------------------
def test_f32_mode_is_untouched():
    """stem + block in the exact-f32 mode: both settings agree and the stem's BN+ReLU buffer is written -- it equals
    relu(c * scale + shift) of the saved c.  The kernel forms one fma per element; the check forms the product and the sum
    exactly in f64, so the two differ by the fma's rounding: half an ulp of the result, bounded here by 2^-24 of the largest
    |c * scale| + |shift| (the rounding back from f64 adds 2^-53 of the same)."""
    hamspine.set_compute_dtype("f32")
    s = _stem(64)
    blk = _ds_block("bottleneck", 64, 64, 1)
    n, h, w = 2, 32, 32
    x, _ = _stem_inputs(n, h, w, 64)
    cot = torch.randn(n, 256, 8, 8, generator=torch.Generator().manual_seed(8)).to(DEV)
    off, (p, q, _, _) = _stem_arena(n, h, w, 64, 4)

    def run():
        for m in (s, blk):
            m.zero_grad(set_to_none=True)
            _reset_running(m)
        ys = s(x)
        saved = ys.grad_fn.saved_tensors[4]
        assert saved.numel() >= off["end"]
        cnt = n * p * q * 64
        y = blk(ys)
        (y * cot).sum().backward()
        torch.cuda.synchronize()
        out = {"y": y.detach().clone(), "pooled": ys.detach().clone(),
               "c": saved[off["c"]:off["c"] + cnt * 4].clone().view(torch.float32).view(-1, 64),
               "a": saved[off["a"]:off["a"] + cnt * 4].clone().view(torch.float32).view(-1, 64),
               "stats": saved[off["stats"]:off["stats"] + 4 * 64 * 4].clone().view(torch.float32).view(4, 64)}
        out.update({"stem." + k: v.grad.detach().clone() for k, v in s.named_parameters()})
        out.update({"blk." + k: v.grad.detach().clone() for k, v in blk.named_parameters()})
        out.update(_running(s))
        return out
    out = _ab(run)
    c, scale, shift = out["c"].double(), out["stats"][2].double(), out["stats"][3].double()
    want = torch.clamp_min(c * scale + shift, 0.0)
    bound = 2.0 ** -24 * (c.abs() * scale.abs() + shift.abs()).max().item() * (1 + 2.0 ** -20)
    err = (out["a"].double() - want).abs().max().item()
    assert out["a"].abs().max().item() > 0, "the stem's BN+ReLU buffer was not written"
    assert err <= bound, f"saved relu(bn(c)) is off by {err:.3e} (bound {bound:.3e})"
