"""The metric definitions of csrc/metrics.hip, without a GPU: tests/metrics_ref.py (the numpy restatement the GPU tests hold the
kernels against) is pinned on scikit-learn, and the Lightning shim under ConNexT/models/pl_model_MOE2.py is exercised on a small
plain module.  Tolerance 1e-12: both sides divide the same integers in f64 (observed differences are a few 1e-16)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import sklearn.metrics as sk

import metrics_ref as R

CASES = [(37, 3), (257, 7), (1000, 6)]
TOL = 1e-12


def _inputs(N, C, seed=0):
    """labels with every class present (the first C are 0..C-1), logits rounded to quarters so rows and scores tie"""
    rng = np.random.default_rng(1000 * C + N + seed)
    labels = rng.integers(0, C, N)
    labels[:C] = np.arange(C)
    logits = rng.normal(size=(N, C))
    logits[np.arange(N), labels] += 0.8                      # better than chance, far from perfect
    logits = np.round(logits * 4) / 4
    k = max(N // 8, 2)
    logits[N // 2:N // 2 + k] = logits[:k]                    # repeated rows under other labels: scores tie exactly
    return logits, labels


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"N{c[0]}_C{c[1]}")
def case(request):
    N, C = request.param
    logits, labels = _inputs(N, C)
    assert (logits.max(1, keepdims=True) == logits).sum(1).max() > 1, "no tied rows: the arg-max rule is not exercised"
    return N, C, logits, labels, R.argmax_rows(logits), R.softmax64(logits), R.metrics(logits, labels, C)


def test_confusion_matrix_and_per_class_values_match_sklearn(case):
    N, C, logits, labels, preds, probs, res = case
    assert np.array_equal(res["confusion_matrix"], sk.confusion_matrix(labels, preds, labels=list(range(C))))
    p, r, f, s = sk.precision_recall_fscore_support(labels, preds, average=None, labels=list(range(C)), zero_division=0)
    for key, want in (("precision", p), ("recall", r), ("f1", f), ("accuracy_per_class", r)):
        print(key, np.abs(res[key] - want).max())
        assert np.abs(res[key] - want).max() <= TOL, key
    assert np.array_equal(res["support"], s)
    assert abs(res["accuracy"] - sk.accuracy_score(labels, preds)) <= TOL
    cm = res["confusion_matrix"]
    assert np.abs(res["accuracy_per_class"] - cm.diagonal() / cm.sum(1)).max() <= TOL     # ConNexT/models/test.py:128-130


def test_macro_and_weighted_averages_match_sklearn_with_a_class_never_predicted(case):
    N, C, logits, labels, preds, probs, _ = case
    preds = np.where(preds == C - 1, 0, preds)               # class C-1 is never predicted: its precision is 0 / 0 -> 0
    res = R.finalize(R.confusion(labels, preds, C)[0])
    assert res["confusion_matrix"][:, C - 1].sum() == 0 and res["precision"][C - 1] == 0.0
    for avg in ("macro", "weighted"):
        p, r, f, _ = sk.precision_recall_fscore_support(labels, preds, average=avg, labels=list(range(C)), zero_division=0)
        for key, want in ((f"precision_{avg}", p), (f"recall_{avg}", r), (f"f1_{avg}", f)):
            print(key, abs(res[key] - want))
            assert abs(res[key] - want) <= TOL, key


def test_auroc_matches_sklearn_one_vs_rest(case):
    N, C, logits, labels, preds, probs, res = case
    counts = R.pair_counts(probs, labels, C)
    assert counts[:, 1].sum() > 0, "no tied scores: the eq column is not exercised"
    for c in range(C):
        want = sk.roc_auc_score((labels == c).astype(int), probs[:, c])
        print(c, abs(res["auroc"][c] - want))
        assert abs(res["auroc"][c] - want) <= TOL
    if C == 2:
        want = sk.roc_auc_score(labels, probs[:, 1])
    else:
        want = sk.roc_auc_score(labels, probs, multi_class="ovr", average="macro", labels=list(range(C)))
    assert abs(res["auroc_macro"] - want) <= TOL


def test_class_without_positives_is_nan_and_left_out_of_the_auroc_mean():
    logits, labels = _inputs(120, 5, seed=1)
    labels = np.where(labels == 3, 1, labels)
    res = R.metrics(logits, labels, 5)
    assert np.isnan(res["auroc"][3]) and not np.isnan(np.delete(res["auroc"], 3)).any()
    probs = R.softmax64(logits)
    want = np.mean([sk.roc_auc_score((labels == c).astype(int), probs[:, c]) for c in (0, 1, 2, 4)])
    assert abs(res["auroc_macro"] - want) <= TOL
    # one class alone: no class has both positives and negatives
    res = R.metrics(logits, np.zeros(120, dtype=np.int64), 5)
    assert np.isnan(res["auroc"]).all() and np.isnan(res["auroc_macro"])


def test_class_neither_present_nor_predicted_is_left_out_of_macro():
    logits, labels = _inputs(120, 5, seed=2)
    labels = np.where(labels == 3, 1, labels)
    preds = R.argmax_rows(logits)
    preds = np.where(preds == 3, 2, preds)
    res = R.finalize(R.confusion(labels, preds, 5)[0])
    assert res["support"][3] == 0 and res["confusion_matrix"][:, 3].sum() == 0
    for avg in ("macro", "weighted"):                        # scikit-learn's default labels=None: the classes that occur
        p, r, f, _ = sk.precision_recall_fscore_support(labels, preds, average=avg, zero_division=0)
        for key, want in ((f"precision_{avg}", p), (f"recall_{avg}", r), (f"f1_{avg}", f)):
            assert abs(res[key] - want) <= TOL, key
    # and differs from the mean over all five classes, which counts the absent class as 0
    assert abs(res["f1_macro"] - res["f1"].mean()) > 1e-3
    empty = R.finalize(np.zeros((4, 4), dtype=np.int64))
    assert empty["accuracy"] == 0.0 and empty["f1_macro"] == 0.0 and empty["recall_weighted"] == 0.0


def test_out_of_range_labels_are_counted_and_left_out():
    logits, labels = _inputs(50, 4, seed=3)
    bad = labels.copy()
    bad[[5, 17]] = (4, -1)
    keep = np.ones(50, dtype=bool)
    keep[[5, 17]] = False
    res, want = R.metrics(logits, bad, 4), R.metrics(logits[keep], labels[keep], 4)
    assert res["invalid"] == 2 and np.array_equal(res["confusion_matrix"], want["confusion_matrix"])
    assert np.array_equal(res["auroc"], want["auroc"])


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_constants_and_entry_points_of_the_meter():
    import hamspine._lib as L
    from hamspine import metrics as M
    assert M.ABI_CONSTANTS == (M.MAX_CLASSES, M.N_SCALARS, M.N_PER_CLASS) == (64, 8, 5)
    assert len(M.SCALAR_KEYS) == 8 and len(M.PER_CLASS_KEYS) == 5
    protos = L.parse_header(open(L.HEADER_PATH).read()).prototypes
    assert len(protos["hs_metrics_update"][1]) == 13 and len(protos["hs_metrics_auroc"][1]) == 7
    assert len(protos["hs_metrics_finalize"][1]) == 5 and len(protos["hs_metrics_update_preds"][1]) == 7
    with pytest.raises(L.HamspineError):                      # no CPU fallback
        M.MulticlassMeter(3, device="cpu")
    with pytest.raises(L.HamspineError):
        M.MulticlassMeter(65)


# ----------------------------------------------------------------------------------------------------------- the shim
def _shim_module():
    from hamspine.lightning_shim import LightningModule

    class Tiny(LightningModule):
        def __init__(self, learning_rate=1e-4, config=None):
            super().__init__()
            self.save_hyperparameters()
            self.fc = nn.Linear(config["model"]["width"], 3)
            self.register_buffer("class_weights", torch.tensor(config["train"]["class_weights"]))

    return Tiny


def test_shim_hyperparameters_and_log_storage():
    Tiny = _shim_module()
    cfg = {"model": {"width": 4}, "train": {"class_weights": [1.0, 2.0, 0.5]}}
    m = Tiny(learning_rate=3e-4, config=cfg)
    assert m.hparams.learning_rate == 3e-4 and m.hparams.config is cfg and dict(m.hparams).keys() == {"learning_rate", "config"}
    assert Tiny(config=cfg).hparams.learning_rate == 1e-4
    t = torch.tensor(2.0, requires_grad=True)
    m.log("a", t * 1.0, prog_bar=True)
    m.log("b", 0.25)
    assert torch.is_tensor(m.logged["a"]) and not m.logged["a"].requires_grad and m.logged["b"] == 0.25
    for v, bs in ((1.0, None), (2.0, None), (6.0, None)):
        m.log("val_loss", torch.tensor(v), on_step=False, on_epoch=True)
    assert torch.is_tensor(m.logged["val_loss"]) and float(m.logged["val_loss"]) == 3.0 and "val_loss_step" not in m.logged
    m.log("train_loss", torch.tensor(1.0), on_step=True, on_epoch=True, batch_size=3)
    m.log("train_loss", torch.tensor(5.0), on_step=True, on_epoch=True, batch_size=1)
    assert float(m.logged["train_loss"]) == 2.0 and float(m.logged["train_loss_step"]) == 5.0
    m.reset_logged()
    assert m.logged == {}
    m.log("val_loss", torch.tensor(4.0), on_epoch=True)
    assert float(m.logged["val_loss"]) == 4.0


def test_shim_checkpoint_round_trip_and_tolerant_loader(tmp_path):
    from hamspine.checkpoint import load_checkpoint
    Tiny = _shim_module()
    cfg = {"model": {"width": 4}, "train": {"class_weights": [1.0, 2.0, 0.5]}}
    torch.manual_seed(0)
    m = Tiny(learning_rate=3e-4, config=cfg)
    m.current_epoch, m.global_step = 7, 123
    path = m.save_checkpoint(str(tmp_path / "epoch=7-val_Accuracy=0.9.ckpt"))
    ckpt = torch.load(path, weights_only=True)
    assert set(ckpt) == {"state_dict", "hyper_parameters", "epoch", "global_step", "pytorch-lightning_version"}
    assert ckpt["hyper_parameters"] == {"learning_rate": 3e-4, "config": cfg} and (ckpt["epoch"], ckpt["global_step"]) == (7, 123)
    cfg2 = {"model": {"width": 4}, "train": {"class_weights": [9.0, 9.0, 9.0]}}
    back = Tiny.load_from_checkpoint(path, map_location="cpu")
    over = Tiny.load_from_checkpoint(path, map_location="cpu", config=cfg2)
    assert back.hparams.config == cfg and over.hparams.config == cfg2 and over.hparams.learning_rate == 3e-4
    for other in (back, over):
        assert (other.current_epoch, other.global_step) == (7, 123)
        assert all(torch.equal(v, other.state_dict()[k]) for k, v in m.state_dict().items())
    # hamspine.checkpoint.load_checkpoint unwraps the same file
    torch.manual_seed(1)
    fresh = Tiny(config=cfg2)
    missing, unexpected = load_checkpoint(fresh, path, verbose=False)
    assert missing == [] and unexpected == []
    assert all(torch.equal(v, fresh.state_dict()[k]) for k, v in m.state_dict().items())
    with pytest.raises(RuntimeError):
        Tiny.load_from_checkpoint(path, config={"model": {"width": 5}, "train": {"class_weights": [1.0, 1.0, 1.0]}})


def test_drop_in_imports_and_derives_from_the_shim_without_lightning():
    from ConNexT.models import pl_model_MOE2 as P
    try:
        import pytorch_lightning as pl
        base = pl.LightningModule
    except ImportError:
        from hamspine.lightning_shim import LightningModule as base
    assert issubclass(P.Model4AAAI_MoE, base)
    for name in ("ConvNeXtEncoder", "BaseLineConvNeXt_KAN_mamba", "SimpleFusion", "Model4AAAI_MoE"):
        assert hasattr(P, name)
    f = P.SimpleFusion(8, 16, 4, proj_dim=6)
    assert sorted(f.state_dict()) == ["hidden_proj.bias", "hidden_proj.weight", "img_proj.bias", "img_proj.weight",
                                      "text_proj.bias", "text_proj.weight"]
    assert f.hidden_proj.weight.shape == (6, 8)
