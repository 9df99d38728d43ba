"""The ConNeXT family's Lightning module (reference ConNexT/models/pl_model_MOE2.py:29-202): same class names, constructor
signatures, attribute names and state-dict keys (`net.net.*`, plus `class_weights` and `loss.weight` with class weights), so
that ConNexT/predict.py and ConNexT/models/test.py -- both `Model4AAAI_MoE.load_from_checkpoint(...)` -- run on this tree.

What differs from the reference:
  * `Model4AAAI_MoE` derives from `pytorch_lightning.LightningModule` when that package imports, else from
    `hamspine.lightning_shim.LightningModule` (hyper-parameters, `log`, `.ckpt` save / load; no Trainer).
  * the three torchmetrics collections are ONE `hamspine.metrics.MulticlassMeter`: `validation_step` makes one kernel launch
    and never synchronises, `on_validation_epoch_end` reads the device once.  With torch.distributed initialised over more
    than one rank the meter is made with group="world": every rank then logs the metrics of all ranks' rows.  The attributes `validation_macro_metrics`,
    `val_auroc` and `validation_per_class_metrics` all name that meter; like the reference's metric objects it adds no
    state-dict keys.  A class without positives has AUROC NaN and is left out of `val_AUROC` (torchmetrics: 0 with a warning).
  * the loss is `hamspine.functional.cross_entropy`, the optimizer `hamspine.optim.FusedAdam` (Adam with L2 weight decay, as
    torch.optim.Adam).  With `gradient_clip_val` in config['train'] it clips the global gradient norm inside its step
    (`FusedAdam(max_grad_norm=...)`: .grad stays unscaled; pass no `gradient_clip_val` to the Trainer as well).
"""
import torch
import torch.nn as nn

from hamspine import functional as F
from hamspine.metrics import MulticlassMeter
from hamspine.nn import Linear
from hamspine.nn.convnext import convnext_large_features
from hamspine.optim import FusedAdam

from .ourmodel import OurClassfierConvnextV2

try:
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except ImportError:
    from hamspine.lightning_shim import LightningModule as _Base


class ConvNeXtEncoder(nn.Module):
    """torchvision `convnext_large().features` followed by flatten(2): (B, 3, H, W) -> (B, 1536, H/32 * W/32) in the compute
    dtype.  ImageNet weights cannot be fetched here, so `pretrained` is accepted and the initialisation is the one of
    `weights=None` either way; load a state dict into `.features` (torchvision's keys) for trained weights.  The 1536-channel
    last stage is wider than the f32 LayerNorm kernel's rows (1024), so the tower runs in the bf16 compute mode (the default);
    in the f32 parity mode its LayerNorm raises.  Nothing in this file instantiates the encoder, as in the reference."""

    def __init__(self, pretrained=True):
        super().__init__()
        self.features = convnext_large_features()
        self.output_dim = 1536

    def forward(self, x):
        return self.features(x).flatten(2)


class BaseLineConvNeXt_KAN_mamba(nn.Module):
    """OurClassfierConvnextV2 behind the batch keys of the Lightning loaders; returns (logits, balance_loss = 0).

    One addition to the reference, which hard-codes both directories: they are read from
    `config['model'].get('pretrained_path', "/data/QLI/ConNexT/convnext-base-224")` and
    `config['model'].get('bert_path', "/data/QLI/BERT_pretain")`, so a tree without /data can point elsewhere.  A config
    without these keys behaves as the reference does."""

    def __init__(self, config):
        super().__init__()
        num_classes = config['model']['num_classes']
        self.net = OurClassfierConvnextV2(
            num_labels=num_classes,
            pretrained=True,
            pretrained_path=config['model'].get('pretrained_path', "/data/QLI/ConNexT/convnext-base-224"),
            bert_path=config['model'].get('bert_path', "/data/QLI/BERT_pretain"),
        )

    def forward(self, x):
        batch = {
            "transformed_image": x["imgs"],
            "input_ids": x["texts"]["input_ids"],
            "attention_mask": x["texts"]["attention_mask"],
        }
        logits = self.net(batch)
        balance_loss = torch.zeros((), device=logits.device)
        return logits, balance_loss


class SimpleFusion(nn.Module):
    def __init__(self, text_dim, img_dim, hidden_dim, proj_dim=256):
        super().__init__()
        self.text_proj = Linear(text_dim, proj_dim)
        self.img_proj = Linear(img_dim, proj_dim)
        self.hidden_proj = Linear(hidden_dim * 2, proj_dim)

    def forward(self, text_embedding, image_embedding, first_hidden, last_hidden):
        img_global = F.mean_tokens(image_embedding.transpose(1, 2).contiguous())       # mean over dim 2 of (B, C, N)
        text_token = self.text_proj(text_embedding)
        img_token = self.img_proj(img_global)
        hidden_token = self.hidden_proj(torch.cat([first_hidden, last_hidden], dim=1))
        return torch.stack([text_token, img_token, hidden_token], dim=1)


class _CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(weight=...) on the fused kernel; `weight` is a buffer, as there (state-dict key `loss.weight`)"""

    def __init__(self, weight=None):
        super().__init__()
        self.register_buffer("weight", weight)

    def forward(self, logits, labels):
        return F.cross_entropy(logits.float(), labels, weight=self.weight)


class Model4AAAI_MoE(_Base):
    def __init__(self, learning_rate=1e-4, config=None):
        super().__init__()
        self.save_hyperparameters()

        class_weights_list = config['train'].get('class_weights', None)
        if class_weights_list:
            print("使用加权交叉熵损失...")
            weights = torch.tensor(class_weights_list, dtype=torch.float)
            self.register_buffer('class_weights', weights)
            self.loss = _CrossEntropyLoss(weight=self.class_weights.clone())
        else:
            print("使用标准交叉熵损失...")
            self.loss = _CrossEntropyLoss()

        self.net = BaseLineConvNeXt_KAN_mamba(config)

        self.config = config
        self.balance_weight = config['model']['moe'].get('balance_weight', 0.01)

        num_classes = config['model']['num_classes']
        self.num_classes = num_classes
        self._meter = None            # made on the first validation batch, on its device; holds no module state

        self.class_names = config.get('data', {}).get('class_names', [f'class_{i}' for i in range(num_classes)])
        if len(self.class_names) != num_classes:
            raise ValueError("The number of class_names provided does not match num_classes.")

    # the reference's three metric objects are one device-side meter
    @property
    def validation_macro_metrics(self):
        return self._meter

    val_auroc = validation_per_class_metrics = validation_macro_metrics

    def _meter_on(self, device):
        if self._meter is None or self._meter.device != device:
            # under data parallelism every rank validates its own shard (hamspine.metrics.shard_indices) and logs the metrics
            # of all ranks' rows; one process: the meter as it was
            import torch.distributed as dist
            many = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
            self._meter = MulticlassMeter(self.num_classes, device=device, group="world" if many else None)
        return self._meter

    def forward(self, x):
        return self.net(x)[0]

    def training_step(self, batch, batch_idx):
        pred, balance_loss = self.net(batch)
        cls_loss = self.loss(pred, batch["labels"])
        total_loss = cls_loss + self.balance_weight * balance_loss

        accuracy = (pred.argmax(dim=-1) == batch["labels"]).float().mean()

        self.log('train_loss', total_loss, on_step=True, on_epoch=True, prog_bar=True)
        self.log('train_acc', accuracy, on_step=True, on_epoch=True, prog_bar=True)

        return total_loss

    def validation_step(self, batch, batch_idx):
        pred, _ = self.net(batch)
        loss = self.loss(pred, batch["labels"])
        # arg-max, softmax, confusion matrix and the stored scores of all three reference collections: one launch, no sync
        self._meter_on(pred.device).update(pred, batch["labels"])

        self.log("val_loss", loss, on_step=False, on_epoch=True, prog_bar=True)
        return loss

    def on_validation_epoch_end(self):
        if self._meter is None:
            return
        res = self._meter.compute()

        self.log('val_Accuracy', res['accuracy'], prog_bar=True)
        self.log('val_Precision_macro', res['precision_macro'], prog_bar=False)
        self.log('val_Recall_macro', res['recall_macro'], prog_bar=False)
        self.log('val_F1_macro', res['f1_macro'], prog_bar=True)
        self.log('val_AUROC', res['auroc_macro'], prog_bar=False)

        for base_metric_name, key in (('Accuracy', 'accuracy_per_class'), ('Precision', 'precision'), ('Recall', 'recall'),
                                      ('F1_score', 'f1')):
            for i, value in enumerate(res[key]):
                class_name = self.class_names[i]
                log_tag = f"per_class/{base_metric_name}_{class_name}"
                self.log(log_tag, float(value), prog_bar=False)

        self._meter.reset()

    def configure_optimizers(self):
        # config['train']['gradient_clip_val'] (the stock Trainer argument, given here in the config): global gradient-norm
        # clipping inside the fused step, no host sync; absent: the optimizer as it was
        optimizer = FusedAdam(self.parameters(), lr=self.hparams.learning_rate, weight_decay=1e-5,
                              max_grad_norm=self.hparams.config['train'].get('gradient_clip_val'))
        scheduler = {
            "scheduler": torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=10, eta_min=1e-6),
            "interval": "epoch",
            "frequency": 1,
        }
        return [optimizer], [scheduler]
