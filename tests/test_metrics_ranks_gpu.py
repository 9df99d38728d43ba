"""MulticlassMeter.compute(group=...) over two ranks that share the one card (gloo carries the exchange through host memory), as
tests/test_supcon_global_gpu.py runs its ranks: every rank returns the metrics of the union of all rows, bit for bit what one
process computes from all rows, with either AUROC route; local state stays; failures reach every rank.

Every wait is bounded: the process group has a timeout, the results are awaited with a timeout, the workers joined with one and
terminated (and the test failed) if still alive."""
import datetime
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import metrics_ranked_ref as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, N = 7, 101
SPLITS = {"37+64": (slice(0, 37), slice(37, 101)), "0+101": (slice(0, 0), slice(0, 101))}
ROUTES = ("pairs", "ranked")
LOGGED = ("val_Accuracy", "val_F1_macro", "val_AUROC", "val_Precision_macro", "val_Recall_macro")


def _data():
    return RR.meter_inputs(N, C, 41)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _feed(meter, logits, labels, rows):
    """rows in batches of 16 (none: no update at all)"""
    lg, lb = logits[rows], labels[rows]
    for at in range(0, len(lb), 16):
        meter.update(torch.from_numpy(lg[at:at + 16]).cuda(), torch.from_numpy(lb[at:at + 16]).cuda())
    return meter


def _pack(res, meter):
    return dict(res, auroc_counts=meter.auroc_counts())


def _pl_model(tmp):
    """the Lightning module as tests/test_pl_model_gpu.py builds it: its smallest towers, procedural weights"""
    import golden_cases as gc
    from ConNexT.models.pl_model_MOE2 import Model4AAAI_MoE
    from oracle.procedural import load_procedural
    dirs = (gc.save_bert_dir(gc.MIBF_BERT, os.path.join(tmp, "bert768")), gc.save_convnext_dir(gc.CONNEXT_CFG, os.path.join(tmp, "convnext")))
    cfg = {"model": {"num_classes": 5, "moe": {"balance_weight": 0.01}, "pretrained_path": dirs[1], "bert_path": dirs[0]}, "train": {}}
    m = Model4AAAI_MoE(config=cfg)
    load_procedural(m.net.net, gc.SEED + 310)
    return m.to("cuda").eval()


def _pl_batches():
    import golden_cases as gc
    from oracle.procedural import synthetic_batch
    out = []
    for inputs in (gc.connext_inputs(), synthetic_batch(3, 64, 16, gc.MIBF_BERT["vocab_size"], 5, seed=312, min_len=3)):
        images, ids, mask, labels = [t.to("cuda") for t in inputs]
        out.append({"imgs": images, "texts": {"input_ids": ids, "attention_mask": mask}, "labels": labels})
    return out


def _pl_logged(m, batches):
    with torch.no_grad():
        for i, b in enumerate(batches):
            m.validation_step(b, i)
    m.on_validation_epoch_end()
    return {k: m.logged[k] for k in LOGGED}


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, os.path.join(ROOT, "multimodal-diagnosis-ham-spine_amd"))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        import hamspine
        from hamspine import metrics as M
        from hamspine._lib import HamspineError
        hamspine.set_compute_dtype("f32")
        logits, labels = _data()
        res = {}
        for name, split in SPLITS.items():
            for route in ROUTES:
                meter = _feed(M.MulticlassMeter(C, capacity=16, auroc=route), logits, labels, split[rank])
                n, cm = meter.n, meter.cm.clone()
                stored = meter.scores[:, :n].clone()
                first = _pack(meter.compute(group="world"), meter)
                again = _pack(meter.compute(group=dist.group.WORLD), meter)
                res[name, route] = first
                res[name, route, "again"] = all(np.array_equal(again[k], v, equal_nan=True) for k, v in first.items())
                res[name, route, "state"] = (meter.n == n and torch.equal(meter.cm, cm) and int(meter.invalid) == 0
                                             and torch.equal(meter.scores[:, :n], stored))
                res[name, route, "local_rows"] = int(meter.compute()["support"].sum())     # no group: this rank's shard
        # shards of shard_indices, the group given to the constructor
        rows = np.array(M.shard_indices(N, rank, world), dtype=np.int64)
        meter = _feed(M.MulticlassMeter(C, capacity=16, auroc="ranked", group="world"), logits, labels, rows)
        res["sharded"] = _pack(meter.compute(), meter)
        res["sharded_rows"] = rows
        # a label out of range on rank 1 only; then num_classes differing between the ranks: HamspineError on both, no hang
        bad = labels.copy()
        if rank == 1:
            bad[50] = C
        for what, make in (("bad_label", lambda: _feed(M.MulticlassMeter(C, capacity=16), logits, bad, SPLITS["37+64"][rank])),
                           ("classes", lambda: M.MulticlassMeter(C - rank, capacity=16)),
                           ("keep_scores", lambda: M.MulticlassMeter(C, capacity=16, keep_scores=rank == 0))):
            try:
                make().compute(group="world")
                res[what] = "accepted"
            except HamspineError as e:
                res[what] = "HamspineError: " + str(e)
        # and the ranks still talk to each other afterwards
        meter = _feed(M.MulticlassMeter(C, capacity=16), logits, labels, SPLITS["37+64"][rank])
        res["after"] = _pack(meter.compute(group="world"), meter)
        # the Lightning module: each rank validates one of the two batches
        with tempfile.TemporaryDirectory() as tmp:
            m = _pl_model(tmp)
            res["pl"] = _pl_logged(m, [_pl_batches()[rank]])
            res["pl_group"] = m.val_auroc.group
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
    res, stuck = {}, []
    try:
        for _ in procs:
            r = out.get(timeout=300)
            res[r[0]] = r
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                stuck.append(p.pid)
                p.terminate()
                p.join(timeout=10)
    assert not stuck, f"workers {stuck} were still alive and were terminated"
    for r in res.values():
        assert r[1] == "ok", r[1]
    return {k: r[2] for k, r in res.items()}


@pytest.fixture(scope="module")
def single():
    """one process, one meter fed all rows, per route"""
    import hamspine  # noqa: F401
    from hamspine import metrics as M
    logits, labels = _data()
    out = {}
    for route in ROUTES:
        meter = _feed(M.MulticlassMeter(C, capacity=16, auroc=route), logits, labels, slice(0, N))
        out[route] = _pack(meter.compute(), meter)
    return out


def _same(got, want, what):
    assert set(got) == set(want), what
    for k, v in want.items():
        a, b = np.atleast_1d(np.asarray(got[k])), np.atleast_1d(np.asarray(v))
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: {k}"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("split", list(SPLITS))
def test_every_rank_returns_the_metrics_of_all_rows(two_ranks, single, split, route):
    assert {"confusion_matrix", "auroc_counts", "auroc_macro"} <= set(single[route])
    assert int(single[route]["confusion_matrix"].sum()) == N and not np.isnan(single[route]["auroc"]).any()
    _same(single["ranked"], single["pairs"], "one process, the two routes")
    for r in range(2):
        _same(two_ranks[r][split, route], single[route], f"rank {r}, shards {split}, {route}")
        assert two_ranks[r][split, route, "again"], f"rank {r}: a second compute(group=...) differs"
        assert two_ranks[r][split, route, "state"], f"rank {r}: compute(group=...) changed n, cm or the stored rows"
    _same(two_ranks[0][split, route], two_ranks[1][split, route], "rank 0 against rank 1")
    rows = [s.stop - s.start for s in SPLITS[split]]
    assert [two_ranks[r][split, route, "local_rows"] for r in range(2)] == rows, "compute(group=None) is not the local shard"


def test_shard_indices_shards_cover_every_row_once(two_ranks, single):
    rows = np.concatenate([two_ranks[r]["sharded_rows"] for r in range(2)])
    assert np.array_equal(np.sort(rows), np.arange(N))
    for r in range(2):
        _same(two_ranks[r]["sharded"], single["ranked"], f"rank {r}, strided shards")


def test_failures_reach_every_rank_and_nobody_hangs(two_ranks, single):
    for r in range(2):
        assert two_ranks[r]["bad_label"].startswith("HamspineError") and "1 rows" in two_ranks[r]["bad_label"], two_ranks[r]["bad_label"]
        assert two_ranks[r]["classes"].startswith("HamspineError") and "num_classes" in two_ranks[r]["classes"], two_ranks[r]["classes"]
        assert two_ranks[r]["keep_scores"].startswith("HamspineError"), two_ranks[r]["keep_scores"]
        _same(two_ranks[r]["after"], single["pairs"], f"rank {r}, after the failures")


def test_lightning_module_logs_the_global_metrics_on_every_rank(two_ranks):
    import hamspine
    hamspine.set_compute_dtype("f32")
    try:
        with tempfile.TemporaryDirectory() as tmp:
            m = _pl_model(tmp)
            want = _pl_logged(m, _pl_batches())
            assert m.val_auroc.group is None                      # one process: the meter as it was
    finally:
        hamspine.set_compute_dtype("bf16")
    assert not np.isnan(want["val_AUROC"])
    for r in range(2):
        assert two_ranks[r]["pl_group"] == "world"
        for k in LOGGED:
            assert isinstance(two_ranks[r]["pl"][k], float) and two_ranks[r]["pl"][k] == want[k], (r, k, two_ranks[r]["pl"][k], want[k])
