"""Writes tests/golden/mambavision_model.npz and tests/golden/mambavision_variants.json from the reference's own MambaVision
(ConNexT/models/block/mamba_vision.py in the reference tree).

    python tests/gen_mambavision_model_golden.py <path of the reference tree>

Same scheme as tests/gen_mambavision_golden.py, whose stand-ins for timm / mamba_ssm it reuses: the reference's classes run on the
CPU in float64 and the scan is the yardstick's loop on both sides.  No test imports this file; the tests read the fixtures.

mambavision_model.npz: MambaVision(dim=8, in_dim=8, depths=[1,2,2,2], num_heads=[1,1,2,2], window_size=[8,8,4,2], mlp_ratio=2,
drop_path_rate=0., num_classes=5, layer_scale=0.5, layer_scale_conv=0.5) in train mode on a seeded (2, 3, 96, 80) input (maps
24x20 -> 12x10 -> 6x5 -> 3x3: stage 3 pads to 4 windows, stage 4 pads, both stride-2 convs of the levels see an odd extent).  It
holds the f32 state dict (constants perturbed, running statistics too), the float64 logits, forward_features_mamba_fusion
output, the input gradient for a fixed cotangent of the logits, the BatchNorm buffers after the step and the eval-mode logits.

mambavision_variants.json: per factory, built on the meta device: number of state-dict keys, number of parameters, SHA-256 of the
"key:shape" lines; and the encoder's output shape for the variants T and S at 224 pixels."""
import hashlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_mambavision_golden as base  # noqa: E402

SMALL_KW = dict(dim=8, in_dim=8, depths=[1, 2, 2, 2], num_heads=[1, 1, 2, 2], window_size=[8, 8, 4, 2], mlp_ratio=2,
                drop_path_rate=0., num_classes=5, layer_scale=0.5, layer_scale_conv=0.5)
FACTORIES = ["mamba_vision_T", "mamba_vision_T2", "mamba_vision_S", "mamba_vision_B", "mamba_vision_B_21k", "mamba_vision_L",
             "mamba_vision_L_21k", "mamba_vision_L2", "mamba_vision_L2_512_21k", "mamba_vision_L3_256_21k", "mamba_vision_L3_512_21k"]


class _DropPath(torch.nn.Module):
    """the factories build with stochastic depth; the fixtures never run it"""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        assert self.drop_prob == 0.0 or not self.training
        return x


class _Cfg(dict):
    def to_dict(self):
        return dict(self)


def _load_reference(reference_root):
    base._register_stand_ins()
    builder = sys.modules["timm.models._builder"]
    sys.modules["timm.models.layers"].DropPath = _DropPath
    builder.resolve_pretrained_cfg = lambda name, **kw: _Cfg(url="")
    builder._update_default_model_kwargs = lambda *a, **k: None
    sys.modules["timm.models"]._update_default_kwargs = lambda *a, **k: None
    try:
        import einops  # noqa: F401
    except ImportError:
        m = types.ModuleType("einops")
        m.rearrange = m.repeat = None
        sys.modules["einops"] = m
    path = os.path.join(reference_root, "ConNexT", "models", "block", "mamba_vision.py")
    spec = importlib.util.spec_from_file_location("reference_mamba_vision", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def signature(model):
    sd = model.state_dict()
    lines = "\n".join(f"{k}:{tuple(v.shape)}" for k, v in sd.items())
    return {"keys": len(sd), "parameters": sum(p.numel() for p in model.parameters()),
            "sha256": hashlib.sha256(lines.encode()).hexdigest()}


def small_model_fixture(ref):
    torch.manual_seed(30)
    model = ref.MambaVision(**SMALL_KW).train()
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():      # generic values where the initialisers give constants; A_log and dt_proj.bias stay as initialised
        for n, p in model.named_parameters():
            if "dt_proj" not in n and (n.endswith((".D", ".bias", "gamma_1", "gamma_2", "gamma")) or "norm" in n
                                       or "conv_down.1." in n or "conv_down.4." in n):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
        for n, b in model.named_buffers():
            if n.endswith("running_mean"):
                b.add_(0.1 * torch.randn(b.shape, generator=g))
            elif n.endswith("running_var"):
                b.mul_(1 + 0.2 * torch.rand(b.shape, generator=g))
    sd32 = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.double()
    x32 = torch.randn(2, 3, 96, 80, generator=g)
    w32 = torch.randn(2, 5, generator=g)
    x = x32.double().requires_grad_(True)
    fusion = model.forward_features_mamba_fusion(x).detach()    # updates the running statistics once ...
    model.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd32.items()})   # ... so put them back
    logits = model(x)
    (logits * w32.double()).sum().backward()
    after = {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    with torch.no_grad():
        eval_logits = model.eval()(x.detach())
    arrays = {"x": x32.numpy(), "cotangent": w32.numpy(), "logits": logits.detach().numpy(), "fusion": fusion.numpy(),
              "dx": x.grad.numpy(), "eval_logits": eval_logits.numpy()}
    arrays.update({"sd." + k: v.numpy() for k, v in sd32.items()})
    arrays.update({"after." + k: v.numpy() for k, v in after.items()})
    dst = os.path.join(HERE, "golden", "mambavision_model.npz")
    np.savez_compressed(dst, **arrays)
    print(f"wrote {dst}: {os.path.getsize(dst)} bytes, {len(arrays)} arrays; fusion {tuple(fusion.shape)}")


def variants_fixture(ref):
    out = {"factories": {}, "encoder": {}}
    linspace = torch.linspace
    torch.linspace = lambda *a, **k: linspace(*a, **{**k, "device": "cpu"})     # the drop-path rates are read with .item()
    try:
        for name in FACTORIES:
            with torch.device("meta"):
                model = getattr(ref, name)(pretrained=False)
            out["factories"][name] = signature(model)
            if name in ("mamba_vision_T", "mamba_vision_S"):
                feat = model.head.in_features
                side = 224 // 32
                out["encoder"][name[-1]] = {"num_features": feat, "map": [feat, side, side], "tokens": [1568, feat * side * side // 1568]}
    finally:
        torch.linspace = linspace
    dst = os.path.join(HERE, "golden", "mambavision_variants.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {dst}")


def main(reference_root):
    ref = _load_reference(reference_root)
    small_model_fixture(ref)
    variants_fixture(ref)


if __name__ == "__main__":
    main(sys.argv[1])
