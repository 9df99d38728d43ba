"""ConNexT/models/pl_model_MOE2.py on the GPU: the Lightning module around OurClassfierConvnextV2 against the golden vectors of
the reference model (tests/golden/e2e_connext.npz), its validation metrics against tests/metrics_ref.py, its checkpoint.

Built as tests/test_convnext_gpu.py::_build_connext builds the bare model: tiny towers saved as local directories, named through
config['model'], and the same procedural weights loaded into `net.net`.  Tolerances are that file's: 1e-4 on logits and loss,
5e-3 on gradient norms (f32 mode)."""
import numpy as np
import pytest
import torch

import golden_cases as gc
import metrics_ref as R

pytestmark = pytest.mark.gpu

import hamspine  # noqa: E402
from oracle.procedural import load_procedural, synthetic_batch  # noqa: E402

DEV = "cuda"
NAMES = ["akiec", "bcc", "bkl", "df", "mel"]


@pytest.fixture(autouse=True)
def _f32_mode():
    hamspine.set_compute_dtype("f32")
    yield
    hamspine.set_compute_dtype("bf16")


def _close(a, b, what, rtol, atol=2e-6):
    a, b = a.detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    scale = max(b.abs().max().item(), 1e-6)
    err = (a - b).abs().max().item()
    assert err <= rtol * scale + atol, f"{what}: max err {err:.3e} (scale {scale:.3e}, rtol {rtol})"


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("connext_pl")
    return (gc.save_bert_dir(gc.MIBF_BERT, str(root / "bert768")), gc.save_convnext_dir(gc.CONNEXT_CFG, str(root / "convnext")))


def _config(dirs, class_weights=None, **data):
    cfg = {"model": {"num_classes": 5, "moe": {"balance_weight": 0.01}, "pretrained_path": dirs[1], "bert_path": dirs[0]},
           "train": {}}
    if class_weights:
        cfg["train"]["class_weights"] = class_weights
    if data:
        cfg["data"] = data
    return cfg


def _build(cfg, lr=1e-4):
    from ConNexT.models.pl_model_MOE2 import Model4AAAI_MoE
    m = Model4AAAI_MoE(learning_rate=lr, config=cfg)
    assert m.net.net._use_hf
    load_procedural(m.net.net, gc.SEED + 310)
    return m.to(DEV)


def _batch(inputs):
    images, ids, mask, labels = [t.to(DEV) for t in inputs]
    return {"imgs": images, "texts": {"input_ids": ids, "attention_mask": mask}, "labels": labels}


def test_forward_training_step_optimizer_and_checkpoint(dirs, tmp_path):
    from hamspine.optim import FusedAdam
    fx = gc.load("e2e_connext")
    cfg = _config(dirs)
    m = _build(cfg, lr=3e-4).train()
    batch = _batch(gc.connext_inputs())
    assert m.hparams.learning_rate == 3e-4 and m.hparams.config is cfg and m.class_names == [f"class_{i}" for i in range(5)]
    assert all(k.startswith("net.net.") for k in m.state_dict())
    assert {k[len("net.net."):] for k in m.state_dict()} == set(m.net.net.state_dict())
    # forward: the bare model's logits, bit for bit, and the reference's
    logits = m(batch)
    direct = m.net.net({"input_ids": batch["texts"]["input_ids"], "attention_mask": batch["texts"]["attention_mask"],
                        "transformed_image": batch["imgs"]})
    assert torch.equal(logits, direct)
    _close(logits, fx["logits"], "logits", 1e-4)
    pred, balance = m.net(batch)
    assert balance.shape == () and float(balance) == 0.0
    # training step: the fixture's loss, the gradient norms of the existing end-to-end test
    loss = m.training_step(batch, 0)
    _close(loss, fx["loss"], "training_step loss", 1e-4)
    assert set(m.logged) == {"train_loss", "train_loss_step", "train_acc", "train_acc_step"}
    assert all(torch.is_tensor(v) and v.is_cuda and not v.requires_grad for v in m.logged.values())
    _close(m.logged["train_loss"], fx["loss"], "logged train_loss", 1e-4)
    want_acc = (fx["logits"].argmax(1) == gc.connext_inputs()[3]).float().mean()
    assert float(m.logged["train_acc"]) == float(want_acc)
    loss.backward()
    params = dict(m.net.net.named_parameters())
    for k, n in fx["gnorm"].items():
        _close(params[k].grad.norm(), n, f"|grad {k}|", 5e-3, 1e-7)
    # the optimizer pair, and one step
    opts, scheds = m.configure_optimizers()
    assert len(opts) == 1 and isinstance(opts[0], FusedAdam) and len(scheds) == 1
    g = opts[0].param_groups[0]
    assert g["lr"] == 3e-4 and g["weight_decay"] == 1e-5 and len(g["params"]) == len(list(m.parameters()))
    s = scheds[0]
    assert (s["interval"], s["frequency"]) == ("epoch", 1) and set(s) == {"scheduler", "interval", "frequency"}
    assert isinstance(s["scheduler"], torch.optim.lr_scheduler.CosineAnnealingLR)
    assert (s["scheduler"].T_max, s["scheduler"].eta_min) == (10, 1e-6) and s["scheduler"].optimizer is opts[0]
    before = m.net.net.fc.weight.detach().clone()
    opts[0].step()
    s["scheduler"].step()
    after = m.net.net.fc.weight.detach()
    assert torch.isfinite(after).all() and not torch.equal(after, before)
    assert (after - before).abs().max().item() <= 3e-4 * 1.001 + 1e-5 * before.abs().max().item()   # Adam's first step: lr
    assert opts[0].param_groups[0]["lr"] < 3e-4
    # checkpoint round trip
    m.eval()
    with torch.no_grad():
        want = m(batch)
    m.current_epoch, m.global_step = 3, 41
    path = m.save_checkpoint(str(tmp_path / "epoch=3-val_Accuracy=0.5.ckpt"))
    back = type(m).load_from_checkpoint(path, config=cfg, map_location=DEV).eval()
    assert back.hparams.learning_rate == 3e-4 and (back.current_epoch, back.global_step) == (3, 41)
    with torch.no_grad():
        assert torch.equal(back(batch), want)
    from hamspine.checkpoint import load_checkpoint
    assert load_checkpoint(back, path, map_location=DEV, strict=True, verbose=False) == ([], [])


def test_validation_epoch_logs_the_references_keys_with_the_restated_values(dirs):
    cfg = _config(dirs, class_names=NAMES)
    m = _build(cfg).eval()
    seen = []
    m.net.register_forward_hook(lambda mod, args, out: seen.append(out[0].detach().float().cpu().numpy()))
    b1 = _batch(gc.connext_inputs())
    b2 = _batch(synthetic_batch(3, 64, 16, gc.MIBF_BERT["vocab_size"], 5, seed=312, min_len=3))
    with torch.no_grad():
        l1 = m.validation_step(b1, 0)
        l2 = m.validation_step(b2, 1)
    assert m.validation_macro_metrics is m.val_auroc is m.validation_per_class_metrics and m.val_auroc.n == 6
    m.on_validation_epoch_end()
    assert m.val_auroc.n == 0 and int(m.val_auroc.cm.sum()) == 0            # reset
    logits = np.concatenate(seen)
    labels = torch.cat([b1["labels"], b2["labels"]]).cpu().numpy()
    ref = R.metrics(logits, labels, 5)
    want = {"val_loss": None, "val_Accuracy": ref["accuracy"], "val_Precision_macro": ref["precision_macro"],
            "val_Recall_macro": ref["recall_macro"], "val_F1_macro": ref["f1_macro"], "val_AUROC": ref["auroc_macro"]}
    for metric, key in (("Accuracy", "accuracy_per_class"), ("Precision", "precision"), ("Recall", "recall"), ("F1_score", "f1")):
        for i, name in enumerate(NAMES):
            want[f"per_class/{metric}_{name}"] = float(ref[key][i])
    assert set(m.logged) == set(want)
    for k, v in want.items():
        if k == "val_loss":
            continue
        assert isinstance(m.logged[k], float), k
        assert np.isclose(m.logged[k], v, rtol=0, atol=1e-12, equal_nan=True), (k, m.logged[k], v)
    assert not np.isnan(ref["auroc_macro"]) and np.isnan(ref["auroc"]).any()  # 6 rows, 5 classes: some class has no positive
    assert torch.is_tensor(m.logged["val_loss"]) and m.logged["val_loss"].is_cuda
    _close(m.logged["val_loss"], (l1 + l2) / 2, "val_loss epoch mean", 1e-6)
    t = torch.from_numpy(logits)
    _close(m.logged["val_loss"], torch.nn.functional.cross_entropy(t, torch.from_numpy(labels)), "val_loss", 1e-4)
    with pytest.raises(ValueError, match="class_names"):
        type(m)(config=_config(dirs, class_names=NAMES[:4]))


def test_class_weights_add_their_two_keys_and_weigh_the_loss(dirs):
    w = [1.0, 2.0, 0.5, 3.0, 1.5]
    m = _build(_config(dirs, class_weights=w)).train()
    keys = set(m.state_dict())
    assert {"class_weights", "loss.weight"} <= keys and all(k.startswith("net.net.") for k in keys - {"class_weights", "loss.weight"})
    assert m.class_weights.is_cuda and torch.equal(m.loss.weight.cpu(), torch.tensor(w))
    batch = _batch(gc.connext_inputs())
    loss = m.training_step(batch, 0)
    fx = gc.load("e2e_connext")
    want = torch.nn.functional.cross_entropy(fx["logits"], gc.connext_inputs()[3], weight=torch.tensor(w))
    _close(loss, want, "weighted loss", 1e-4)


def test_convnext_large_encoder_shape():
    """in the bf16 compute mode: the f32 LayerNorm kernel takes rows of up to 1024 channels, the last stage here has 1536"""
    from ConNexT.models.pl_model_MOE2 import ConvNeXtEncoder
    hamspine.set_compute_dtype("bf16")
    with torch.device(DEV):
        enc = ConvNeXtEncoder(pretrained=False).eval()
    assert enc.output_dim == 1536 and len(enc.features) == 8 and [len(enc.features[i]) for i in (1, 3, 5, 7)] == [3, 3, 27, 3]
    assert enc.features[7][0].block[0].weight.shape == (1536, 1, 7, 7) and enc.features[0][0].weight.shape == (192, 3, 4, 4)
    with torch.no_grad():
        out = enc(torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(DEV))
    assert out.shape == (1, 1536, 4) and torch.isfinite(out.float()).all()
