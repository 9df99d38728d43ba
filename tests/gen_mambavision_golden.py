"""Writes tests/golden/mambavision_layer.npz from the reference's own MambaVisionLayer (ConNexT/models/block/mamba_vision.py in
the reference tree): a seeded (2, 32, 5, 5) input, the state dict (both f32 values, run in float64), the float64 output and
input gradient for a fixed cotangent of MambaVisionLayer(dim=32, depth=2, num_heads=2, window_size=3, conv=False, downsample=False,
transformer_blocks=[1], layer_scale=0.5).

    python tests/gen_mambavision_golden.py <path of the reference tree>

Runs on the CPU.  No test imports this file; the tests read the .npz.  The reference module imports timm and mamba_ssm, which
need not be installed: small stand-ins are registered in sys.modules before it is imported.  The timm stand-ins restate the
few pieces the stage uses (Mlp: fc1, erf-GELU, fc2; DropPath at rate 0; the registry decorator).  The stand-in for
mamba_ssm's selective_scan_fn is the yardstick's own gate-less loop (tests/mambavision_ref.scan_core), so the fixture pins
everything of the stage to the reference's code - projections, the two convs, the split and concatenation, attention, LayerNorm,
MLP, layer scale, padding, window partition, reverse and crop - except the arithmetic of the scan itself, which comes from our
loop on both sides."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mambavision_ref as mr  # noqa: E402


class _Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _DropPath(nn.Module):
    def __init__(self, drop_prob=0.0):
        super().__init__()
        assert drop_prob == 0.0, "the fixture is generated without stochastic depth"

    def forward(self, x):
        return x


def _selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, return_last_state=False):
    """mamba_ssm's layout - u, delta (b, d, l); A (d, n); B, C (b, n, l) - on the yardstick's loop"""
    assert z is None and delta_softplus and not return_last_state and D is not None and delta_bias is not None
    t = lambda v: v.transpose(1, 2)
    return t(mr.scan_core(t(u), t(delta), delta_bias, A, t(B), t(C), D))


def _register_stand_ins():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    passthrough = lambda fn=None, **kw: fn
    mod("timm")
    mod("timm.models", _update_default_kwargs=passthrough)
    mod("timm.models.registry", register_model=lambda fn: fn)
    mod("timm.models.layers", trunc_normal_=nn.init.trunc_normal_, DropPath=_DropPath, LayerNorm2d=nn.LayerNorm)
    mod("timm.models._builder", resolve_pretrained_cfg=passthrough, _update_default_model_kwargs=passthrough)
    mod("timm.models.vision_transformer", Mlp=_Mlp, PatchEmbed=nn.Identity)
    mod("mamba_ssm")
    mod("mamba_ssm.ops")
    mod("mamba_ssm.ops.selective_scan_interface", selective_scan_fn=_selective_scan_fn)


def main(reference_root):
    _register_stand_ins()
    path = os.path.join(reference_root, "ConNexT", "models", "block", "mamba_vision.py")
    spec = importlib.util.spec_from_file_location("reference_mamba_vision", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.manual_seed(20)
    layer = ref.MambaVisionLayer(dim=32, depth=2, num_heads=2, window_size=3, conv=False, downsample=False,
                                 transformer_blocks=[1], layer_scale=0.5)
    with torch.no_grad():      # generic values where the initialisers give constants; A_log and dt_proj.bias stay as initialised
        for n, p in layer.named_parameters():
            if "dt_proj" not in n and (n.endswith((".D", ".bias", "gamma_1", "gamma_2")) or ".norm" in n):
                p.add_(0.2 * torch.randn_like(p))
    sd32 = {k: v.clone() for k, v in layer.state_dict().items()}      # f32 values: stored as f32, exact in float64
    layer = layer.double()
    g = torch.Generator().manual_seed(21)
    x32 = torch.randn(2, 32, 5, 5, generator=g)
    w32 = torch.randn(2, 32, 5, 5, generator=g)
    x = x32.double().requires_grad_(True)
    w = w32.double()
    out = layer(x)
    (out * w).sum().backward()
    arrays = {"x": x32.numpy(), "cotangent": w32.numpy(), "out": out.detach().numpy(), "dx": x.grad.numpy()}
    arrays.update({"sd." + k: v.numpy() for k, v in sd32.items()})
    dst = os.path.join(HERE, "golden", "mambavision_layer.npz")
    np.savez_compressed(dst, **arrays)
    print(f"wrote {dst}: {os.path.getsize(dst)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main(sys.argv[1])
