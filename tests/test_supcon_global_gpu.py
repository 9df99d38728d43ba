"""The tiled SupCon kernels (hs_supcon_tiled) against the float64 reference, and hamspine.kan.supcon_loss over one process and
over two ranks that share the one card (gloo carries the gather through host memory).

Gate of every value: error against float64 at most twice the sequential-float32 yardstick's, or the a-priori floor of
supcon_global_ref.supcon_tiled_floors; D = 1 takes the absolute bound, as test_loss_head_gpu.test_supcon_loss does.

Measured on an MI355X (records, not thresholds; relative L2 for the loss, max-relative for dfeat, gpu / yardstick):
  N=64   D=64   T=0.5  singleton  loss 2.17e-08 / 2.17e-08   dfeat 3.47e-07 / 3.64e-07
  N=65   D=65   T=0.07 random     loss 1.42e-09 / 1.71e-07   dfeat 4.66e-07 / 5.89e-07   (dup 6.44e-07 / 5.83e-07, near 8.67e-07 / 8.67e-07)
  N=129  D=130  T=0.5  equal      loss 2.55e-08 / 2.55e-08   dfeat 5.36e-07 / 1.22e-06   (dup 2.92e-07 / 4.57e-07, near 2.33e-07 / 4.88e-07)
  N=300  D=257  T=0.5  singleton  loss 3.21e-08 / 5.17e-08   dfeat 2.81e-07 / 7.61e-07
  N=513  D=260  T=0.07 random     loss 1.98e-08 / 1.24e-07   dfeat 5.42e-07 / 9.68e-07
  N=70   D=1024 T=0.5  equal      loss 1.17e-08 / 2.37e-07   dfeat 1.77e-06 / 2.30e-06
  N=66   D=33   T=0.5  singleton  loss 4.67e-08 / 4.67e-08   dfeat 2.92e-07 / 2.64e-07
  N=20   D=255  T=0.07 random     loss 1.55e-08 / 5.90e-08   dfeat 2.76e-07 / 3.55e-07
  N=17   D=256  T=0.5  equal      loss 2.22e-08 / 2.22e-08   dfeat 6.64e-07 / 1.12e-06
  N=1089 D=12   T=0.07 random     loss 2.12e-08 / 9.43e-08   dfeat 1.27e-06 / 3.59e-06
  the "distinct" cases (N=63 D=5, N=257 D=3, N=33 D=31) and N=1: exactly 0; N=2 D=1: dfeat exactly 0 (absolute bound 4.3e-05)
  python B=300 D=40: loss 1.27e-08 / 1.27e-08, grad 6.72e-07 / 1.10e-06; B=40 D=33 tiled: 9.24e-09 / 6.50e-08, 2.86e-07 / 3.10e-07
  DataParallel, 2 x 37 rows: weight gradient 4.42e-07 (one process 4.32e-07), bias gradient 3.53e-07 (one process 3.22e-07)
No case needed its a-priori floor: every error is within twice the yardstick's.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import head_ref as hr
import kernel_ref as kr
import supcon_global_ref as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sg.tiled_cases()
_REFS = {}


def _refs(i):
    """float64 reference, yardstick and floors of case i, computed once"""
    if i not in _REFS:
        c = CASES[i]
        f, lab, T = c["feat"], c["labels"], c["T"]
        ref = hr.supcon_ref64(f, lab, T)
        _REFS[i] = (ref, sg.supcon_yard_blocked(f, lab, T), sg.supcon_tiled_floors(f, lab, T, ref))
    return _REFS[i]


def _same(a, b, keys, what):
    for k in keys:
        assert kr.bits_equal(a[k], b[k]), f"{what}: {k} differs bitwise"


def _zero(t):
    return bool((t == 0).all())


def _gate(tag, loss, dfeat, ref, yard, fl):
    kr.gate(f"{tag} loss", loss, yard["loss"], ref["loss"], reduced=True, floor=fl["loss"])
    if ref["dfeat"].shape[1] == 1:   # D = 1: the projection off the unit vector leaves nothing (1e-16 in float64); absolute bound
        worst = dfeat.double().abs().max().item()
        print(f"{tag} dfeat: gpu max|.| {worst:.3e}, a-priori absolute bound {fl['dfeat_abs']:.3e}")
        assert ref["dfeat"].abs().max().item() <= 1e-9 * fl["dfeat_abs"] and worst <= fl["dfeat_abs"]
    else:
        kr.gate(f"{tag} dfeat", dfeat, yard["dfeat"], ref["dfeat"], floor=fl["dfeat"])


# ======================================================================================================================
# the C entry
# ======================================================================================================================
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c["tag"].replace("supcon tiled ", "") for c in CASES])
def test_tiled_against_float64(i):
    c = CASES[i]
    f, lab, T, tag = c["feat"], c["labels"], c["T"], c["tag"]
    ref, yard, fl = _refs(i)
    r = sg.call_supcon_tiled(f, lab, T)
    assert r["guards"], tag
    _gate(tag, r["loss"], r["dfeat"], ref, yard, fl)
    _same(r, sg.call_supcon_tiled(f, lab, T), ("loss", "dfeat"), tag + " repeat")
    lo = sg.call_supcon_tiled(f, lab, T, want_d=False)
    assert lo["guards"]
    _same(r, lo, ("loss",), tag + " dfeat NULL")
    if c["pattern"] == "distinct":                                 # no anchor has a positive
        assert _zero(r["loss"]) and _zero(r["dfeat"]), tag + ": loss / gradient without positives is not exactly 0"


def test_slices_and_grad_scale_are_bitwise():
    g = kr.gen(77)
    f, lab = torch.randn(130, 70, generator=g), torch.randint(0, 7, (130,), generator=g)
    full = sg.call_supcon_tiled(f, lab, 0.07)
    lo, hi = sg.call_supcon_tiled(f, lab, 0.07, row0=0, M=65), sg.call_supcon_tiled(f, lab, 0.07, row0=65, M=65)
    assert full["guards"] and lo["guards"] and hi["guards"]
    assert kr.bits_equal(torch.cat([lo["dfeat"], hi["dfeat"]]), full["dfeat"]), "the two halves differ from the full call"
    assert kr.bits_equal(lo["loss"], full["loss"]) and kr.bits_equal(hi["loss"], full["loss"])
    two = sg.call_supcon_tiled(f, lab, 0.07, grad_scale=2.0)
    assert kr.bits_equal(two["dfeat"], 2.0 * full["dfeat"]) and kr.bits_equal(two["loss"], full["loss"])
    f65, lab65 = f[:65].contiguous(), lab[:65].contiguous()
    full65 = sg.call_supcon_tiled(f65, lab65, 0.5)
    one = sg.call_supcon_tiled(f65, lab65, 0.5, row0=1, M=1)
    assert one["guards"] and one["dfeat"].shape == (1, 70)
    assert kr.bits_equal(one["dfeat"], full65["dfeat"][1:2]) and kr.bits_equal(one["loss"], full65["loss"])


def test_refusals_write_nothing():
    from hamspine import _lib as L
    g = kr.gen(78)
    f, lab = torch.randn(8, 8, generator=g), torch.randint(0, 3, (8,), generator=g)
    cap = L._header.constants["HS_SUPCON_TILED_MAX_D"]
    for what, kw in (("N = 0", dict(N=0, row0=0, M=1)), ("M = 0", dict(M=0)), ("row0 + M > N", dict(row0=4, M=5)),
                     ("row0 < 0", dict(row0=-1, M=2)), ("D = 0", dict(D=0)), ("D above the cap", dict(D=cap + 1)),
                     ("N = 65537", dict(N=65537))):
        for want_d in (True, False):
            r = sg.call_supcon_tiled(f, lab, 0.07, want_d=want_d, check=False, **kw)
            assert r["status"] != 0, f"{what}: accepted"
            assert r["untouched"], f"{what}: refused, but an output or its guard band was written"
            with pytest.raises(L.HamspineError):
                L.check(r["status"], what)
    assert L.lib().hs_supcon_tiled_ws_bytes(8192, 128) < 4 * L.lib().hs_supcon_tiled_ws_bytes(4096, 128)


# ======================================================================================================================
# hamspine.kan.supcon_loss, one process
# ======================================================================================================================
def _py(f, lab, T=0.07, **kw):
    from hamspine import kan
    x = f.cuda().requires_grad_(True)
    loss = kan.supcon_loss(x, lab.cuda(), T, **kw)
    loss.backward()
    return loss.detach().cpu().reshape(1), x.grad.detach().cpu()


def test_python_beyond_256_rows():
    g = kr.gen(79)
    f, lab = torch.randn(300, 40, generator=g), torch.randint(0, 7, (300,), generator=g)
    ref, yard = hr.supcon_ref64(f, lab, 0.07), sg.supcon_yard_blocked(f, lab, 0.07)
    loss, grad = _py(f, lab)                                      # the single-workgroup entry refuses 300 rows
    _gate("python B=300", loss, grad, ref, yard, sg.supcon_tiled_floors(f, lab, 0.07, ref))


def test_python_default_route_is_unchanged_and_tiled_is_opt_in():
    from hamspine import kan
    g = kr.gen(80)
    f, lab = torch.randn(40, 33, generator=g), torch.randint(0, 7, (40,), generator=g)
    direct = hr.call_supcon(f, lab, 0.07)
    loss, grad = _py(f, lab)
    assert kr.bits_equal(loss, direct["loss"]) and kr.bits_equal(grad, direct["dfeat"]), "B = 40: the default route changed"
    ref, yard = hr.supcon_ref64(f, lab, 0.07), hr.supcon_yard(f, lab, 0.07)
    tl, tg = _py(f, lab, tiled=True)
    _gate("python B=40 tiled", tl, tg, ref, yard, sg.supcon_tiled_floors(f, lab, 0.07, ref))
    tiled = sg.call_supcon_tiled(f, lab, 0.07)
    assert kr.bits_equal(tl, tiled["loss"]) and kr.bits_equal(tg, tiled["dfeat"])
    x = f.cuda().requires_grad_(True)
    m = kan.SupConLoss(0.07)
    assert m.temperature == 0.07 and m.group is None and kan.SupConLoss().temperature == 0.07
    lm = m(x, lab.cuda())
    lm.backward()
    assert kr.bits_equal(lm.detach().cpu().reshape(1), loss) and kr.bits_equal(x.grad.cpu(), grad)


def test_python_tiled_route_does_not_synchronise():
    from hamspine import kan
    g = kr.gen(82)
    x = torch.randn(300, 40, generator=g).cuda().requires_grad_(True)
    y = torch.randint(0, 7, (300,), generator=g).cuda()
    kan.supcon_loss(x, y, 0.07).backward()                         # library loaded, allocator pools warm
    x.grad = None
    probe = torch.ones(4, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            probe.cpu()
        except RuntimeError:
            raised = True
        assert raised, "torch.cuda.set_sync_debug_mode('error') does not raise for .cpu() in this build: the test cannot see a sync"
        loss = kan.supcon_loss(x, y, 0.07)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all())


# ======================================================================================================================
# two ranks on the one card
# ======================================================================================================================
RANK_ROWS, RANK_D, IN_F = 37, 65, 48


def _rank_data():
    g = kr.gen(81)
    f = torch.randn(2 * RANK_ROWS, RANK_D, generator=g)
    lab = torch.randint(0, 7, (2 * RANK_ROWS,), generator=g)
    x = torch.randn(2 * RANK_ROWS, IN_F, generator=g)
    w = torch.randn(RANK_D, IN_F, generator=g) * 0.2
    b = torch.randn(RANK_D, generator=g) * 0.1
    return f, lab, x, w, b


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _projection(w, b):
    import hamspine.nn as hnn
    net = hnn.Linear(IN_F, RANK_D)
    with torch.no_grad():
        net.weight.copy_(w)
        net.bias.copy_(b)
    return net.to("cuda").train()


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import hamspine
        from hamspine import kan
        from hamspine.ddp import DataParallel
        hamspine.set_compute_dtype("f32")
        f, lab, x, w, b = _rank_data()
        rows = slice(rank * RANK_ROWS, (rank + 1) * RANK_ROWS)
        res = {}
        # the function on this rank's rows
        fr = f[rows].cuda().requires_grad_(True)
        loss = kan.supcon_loss(fr, lab[rows].cuda(), 0.07, group="world")
        loss.backward()
        res["loss"], res["grad"] = loss.detach().cpu().reshape(1).numpy(), fr.grad.cpu().numpy()
        fs = f[rows].cuda().requires_grad_(True)
        kan.supcon_loss(fs, lab[rows].cuda(), 0.07, group=dist.group.WORLD, average_across_ranks=False).backward()
        res["grad_sum"] = fs.grad.cpu().numpy()
        # unequal local batches: ValueError on every rank, and nobody is left waiting in the gather
        n = RANK_ROWS - rank
        try:
            kan.supcon_loss(f[:n].cuda(), lab[:n].cuda(), 0.07, group="world")
            res["unequal"] = "accepted"
        except ValueError as e:
            res["unequal"] = "ValueError: " + str(e)
        # through DataParallel: a projection without BatchNorm (per-rank batch statistics would legitimately differ)
        net = _projection(w, b)
        ddp = DataParallel(net)
        lp = kan.supcon_loss(net(x[rows].cuda()), lab[rows].cuda(), 0.07, group="world")
        lp.backward()
        ddp.finish()
        torch.cuda.synchronize()
        res["dw"], res["db"] = net.weight.grad.float().cpu().numpy(), net.bias.grad.float().cpu().numpy()
        res["loss_ddp"] = lp.detach().cpu().reshape(1).numpy()
        out.put((rank, "ok", res))
    except Exception as e:  # noqa: BLE001
        import traceback
        out.put((rank, "error: " + repr(e) + traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in procs:
            r = out.get(timeout=300)
            res[r[0]] = r
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for r in res.values():
        assert r[1] == "ok", r[1]
    return {k: {n: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for n, v in r[2].items()} for k, r in res.items()}


def test_two_ranks_return_the_global_loss_and_their_rows_of_its_gradient(two_ranks):
    f, lab, _, _, _ = _rank_data()
    loss, grad = _py(f, lab, tiled=True)                           # one process, the 74 concatenated rows
    for r in range(2):
        rows = slice(r * RANK_ROWS, (r + 1) * RANK_ROWS)
        assert kr.bits_equal(two_ranks[r]["loss"], loss), f"rank {r}: not the loss of the concatenated batch"
        assert kr.bits_equal(two_ranks[r]["grad"], 2.0 * grad[rows]), f"rank {r}: gradient is not 2 x its slice"
        assert kr.bits_equal(two_ranks[r]["grad_sum"], grad[rows]), f"rank {r}: average_across_ranks=False is not the slice"
    assert kr.bits_equal(two_ranks[0]["loss"], two_ranks[1]["loss"])
    # and it is not the mean of the rank losses
    local = [_py(f[r * RANK_ROWS:(r + 1) * RANK_ROWS], lab[r * RANK_ROWS:(r + 1) * RANK_ROWS], tiled=True)[0] for r in range(2)]
    assert abs(0.5 * (local[0] + local[1]).item() - loss.item()) > 1e-3 * abs(loss.item())


def test_unequal_local_batches_raise_on_every_rank(two_ranks):
    for r in range(2):
        assert two_ranks[r]["unequal"].startswith("ValueError"), two_ranks[r]["unequal"]


def test_data_parallel_holds_the_gradient_of_the_global_loss(two_ranks):
    import hamspine
    from hamspine import kan
    f, lab, x, w, b = _rank_data()
    for k in ("dw", "db", "loss_ddp"):
        assert kr.bits_equal(two_ranks[0][k], two_ranks[1][k]), f"{k} differs across the ranks"
    # float64: the concatenated batch through the same projection
    xd, wd, bd = x.double(), w.double(), b.double()
    ref = hr.supcon_ref64(xd @ wd.T + bd, lab, 0.07)
    want = {"dw": ref["dfeat"].T @ xd, "db": ref["dfeat"].sum(0)}
    hamspine.set_compute_dtype("f32")
    try:
        net = _projection(w, b)
        kan.supcon_loss(net(x.cuda()), lab.cuda(), 0.07, tiled=True).backward()
        single = {"dw": net.weight.grad.float().cpu(), "db": net.bias.grad.float().cpu()}
    finally:
        hamspine.set_compute_dtype("bf16")
    for k in ("dw", "db"):
        e1, e2 = kr.maxrel(single[k], want[k]), kr.maxrel(two_ranks[0][k], want[k])
        print(f"DataParallel {k}: two ranks {e2:.3e}, one process {e1:.3e}")
        assert e2 == e2 and e2 <= max(2.0 * e1, kr.F32_NOISE), f"{k}: two ranks {e2:.3e} vs one process {e1:.3e}"
