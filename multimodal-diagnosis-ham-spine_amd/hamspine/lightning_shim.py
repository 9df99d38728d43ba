"""The part of `pytorch_lightning.LightningModule` that ConNexT/models/pl_model_MOE2.py uses, for trees without Lightning.

`LightningModule` below is a plain `nn.Module` with `save_hyperparameters()`, `log()`, `load_from_checkpoint()` and
`save_checkpoint()`.  When `pytorch_lightning` imports, the drop-in derives from the real class and this module is unused.

Logging never synchronises: `log(name, value)` keeps the value as it is (a device tensor stays a device tensor, `.item()` is
never called) in `self.logged[name]`.  With `on_epoch=True` the values are averaged on the device, weighted by `batch_size`
(default 1): `logged[name]` is the running mean as a device tensor, and with `on_step=True` as well the latest value is kept under
`name + "_step"`.  `reset_logged()` starts a new epoch.

Checkpoints have the layout of Lightning's `.ckpt` files: one `torch.save`d dict with `state_dict`, `hyper_parameters`,
`epoch`, `global_step` and `pytorch-lightning_version`.  Lightning is not installed where this project is built and tested, so
the layout is taken from its documentation and is NOT pinned against a file that Lightning wrote.
"""
import inspect

import torch
import torch.nn as nn

VERSION = "hamspine-shim"


class AttributeDict(dict):
    """dict whose keys read as attributes: `hparams.learning_rate`"""

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key) from None

    def __setattr__(self, key, value):
        self[key] = value


class LightningModule(nn.Module):
    def __init__(self):
        super().__init__()
        self.hparams = AttributeDict()
        self.logged = {}
        self._epoch_sums = {}                  # name -> [weighted sum (device tensor or float), weight]
        self.current_epoch = 0
        self.global_step = 0

    # ------------------------------------------------------------------------------------------------- hyper-parameters
    def save_hyperparameters(self):
        """record the arguments of the calling `__init__` (its own parameters, `self` left out) in `self.hparams`"""
        frame = inspect.currentframe().f_back
        code = frame.f_code
        names = code.co_varnames[1:code.co_argcount + code.co_kwonlyargcount]
        self.hparams.update({k: frame.f_locals[k] for k in names if k in frame.f_locals})

    # -------------------------------------------------------------------------------------------------------- logging
    def log(self, name, value, on_step=None, on_epoch=None, batch_size=None, **unused):
        if torch.is_tensor(value):
            value = value.detach()
        if not on_epoch:
            self.logged[name] = value
            return
        w = 1 if batch_size is None else int(batch_size)
        acc = self._epoch_sums.get(name)
        if acc is None:
            acc = self._epoch_sums[name] = [value * w, w]
        else:
            acc[0] = acc[0] + value * w
            acc[1] += w
        self.logged[name] = acc[0] / acc[1]
        if on_step:
            self.logged[name + "_step"] = value

    def reset_logged(self):
        self.logged = {}
        self._epoch_sums = {}

    # ---------------------------------------------------------------------------------------------------- checkpoints
    def save_checkpoint(self, path):
        torch.save({"epoch": int(self.current_epoch), "global_step": int(self.global_step),
                    "pytorch-lightning_version": VERSION, "state_dict": self.state_dict(),
                    "hyper_parameters": dict(self.hparams)}, path)
        return path

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, strict=True, **kwargs):
        """build the module from the checkpoint's `hyper_parameters` (keyword arguments override them) and load its
        `state_dict`.  The file is read with torch.load(weights_only=True): tensors and plain containers."""
        ckpt = torch.load(checkpoint_path, map_location=map_location, weights_only=True)
        hparams = dict(ckpt.get("hyper_parameters") or {})
        hparams.update(kwargs)
        params = inspect.signature(cls.__init__).parameters
        if not any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values()):
            hparams = {k: v for k, v in hparams.items() if k in params}
        model = cls(**hparams)
        model.load_state_dict(ckpt["state_dict"], strict=strict)
        model.current_epoch = int(ckpt.get("epoch", 0))
        model.global_step = int(ckpt.get("global_step", 0))
        if map_location is not None and not isinstance(map_location, dict) and not callable(map_location):
            model = model.to(map_location)
        return model
