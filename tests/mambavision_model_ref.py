"""Plain-torch restatement of the convolutional half of MambaVision and of the whole model (reference
ConNexT/models/block/mamba_vision.py:1434-1524,1809-1951), built on tests/mambavision_ref.py for the token stages.  The yardstick
of the MambaVision model tests: float64 by default; its autograd gives the gradient references.  `params` is a dict with the
state-dict keys of the module under test.

With `compute_dtype=torch.bfloat16` the functions follow the dtype policy of the module under test: the image is rounded once,
every activation between PatchEmbed and the last window reverse is bfloat16, convolutions take bfloat16 operands (the filter
rounded once) and accumulate wide, BatchNorm statistics, its affine map, tanh-GELU, layer scale and the residual are evaluated
in f32 from f32 parameters and rounded once; the pooled features and the head are f32."""
import torch
import torch.nn.functional as TF

import mambavision_ref as mr
from mambavision_ref import _sub, _wide


def conv3x3_ref(x, weight, bias=None, stride=1):
    """nn.Conv2d(C, Kout, 3, stride, 1): operands in the dtype of x, sum and bias in the wide type, one rounding"""
    xw = _wide(x)
    w = weight.to(x.dtype).to(xw.dtype)
    return TF.conv2d(xw, w, None if bias is None else bias.to(xw.dtype), stride, 1).to(x.dtype)


def batchnorm_ref(x, params, name, eps, training, momentum=0.1, new_stats=None):
    """BatchNorm2d over (B, C, H, W) -> the normalised, scaled and shifted map in the WIDE type (the caller applies the epilogue
    and rounds).  training: batch statistics (biased variance), and new_stats[name + '.running_*'] receive the updated running
    statistics (unbiased variance); eval: the running statistics in `params`."""
    xw = _wide(x)
    g, b = params[name + ".weight"].to(xw.dtype), params[name + ".bias"].to(xw.dtype)
    if training:
        mean, var = xw.mean((0, 2, 3)), xw.var((0, 2, 3), unbiased=False)
        if new_stats is not None:
            n = xw.numel() // xw.shape[1]
            rm, rv = params[name + ".running_mean"].to(xw.dtype), params[name + ".running_var"].to(xw.dtype)
            new_stats[name + ".running_mean"] = ((1 - momentum) * rm + momentum * mean).detach()
            new_stats[name + ".running_var"] = ((1 - momentum) * rv + momentum * var * n / max(n - 1, 1)).detach()
    else:
        mean, var = params[name + ".running_mean"].to(xw.dtype), params[name + ".running_var"].to(xw.dtype)
    inv = torch.rsqrt(var + eps)
    return (xw - mean[None, :, None, None]) * (inv * g)[None, :, None, None] + b[None, :, None, None]


def bn_gelu_tanh_ref(x, params, name, eps, training, new_stats=None):
    return TF.gelu(batchnorm_ref(x, params, name, eps, training, new_stats=new_stats), approximate="tanh").to(x.dtype)


def bn_scale_residual_ref(x, params, name, eps, training, res, ls_gamma=None, rowscale=None, new_stats=None):
    """res + ls_gamma[c] * rowscale[sample] * bn(x)"""
    z = batchnorm_ref(x, params, name, eps, training, new_stats=new_stats)
    if ls_gamma is not None:
        z = z * ls_gamma.to(z.dtype)[None, :, None, None]
    if rowscale is not None:
        z = z * rowscale.to(z.dtype)[:, None, None, None]
    return (_wide(res) + z).to(x.dtype)


def patch_embed_ref(x, params, training=True, new_stats=None):
    """mamba_vision.py:1464-1490; x in the compute dtype"""
    for conv, bn in (("conv_down.0", "conv_down.1"), ("conv_down.3", "conv_down.4")):
        x = conv3x3_ref(x, params[conv + ".weight"], None, 2)
        x = torch.relu(batchnorm_ref(x, params, bn, 1e-4, training, new_stats=new_stats)).to(x.dtype)
    return x


def conv_block_ref(x, params, training=True, rowscale=None, new_stats=None):
    """mamba_vision.py:1493-1524"""
    h = conv3x3_ref(x, params["conv1.weight"], params["conv1.bias"], 1)
    h = bn_gelu_tanh_ref(h, params, "norm1", 1e-5, training, new_stats)
    h = conv3x3_ref(h, params["conv2.weight"], params["conv2.bias"], 1)
    return bn_scale_residual_ref(h, params, "norm2", 1e-5, training, x, params.get("gamma"), rowscale, new_stats)


def downsample_ref(x, params):
    return conv3x3_ref(x, params["reduction.0.weight"], None, 2)


def _prefixed(stats, prefix):
    return None if stats is None else _Prefixed(stats, prefix)


class _Prefixed:
    """writes new_stats entries under a prefix"""

    def __init__(self, target, prefix):
        self.target, self.prefix = target, prefix

    def __setitem__(self, k, v):
        self.target[self.prefix + k] = v


def _depth(params, prefix):
    return 1 + max(int(k[len(prefix):].split(".")[0]) for k in params if k.startswith(prefix))


def levels_ref(x, params, num_heads, window_size, compute_dtype=None, state_dtype=None, training=True, new_stats=None):
    """patch_embed and every level: x (B, 3, H, W) -> the last level's map in the compute dtype (None: the dtype of x)"""
    if compute_dtype is not None:
        x = x.to(compute_dtype)
    x = patch_embed_ref(x, _sub(params, "patch_embed."), training, _prefixed(new_stats, "patch_embed."))
    n_levels = _depth(params, "levels.")
    for i in range(n_levels):
        lp = _sub(params, f"levels.{i}.")
        depth = _depth(lp, "blocks.")
        if "blocks.0.conv1.weight" in lp:
            for j in range(depth):
                x = conv_block_ref(x, _sub(lp, f"blocks.{j}."), training, None, _prefixed(new_stats, f"levels.{i}.blocks.{j}."))
        else:
            H, W = x.shape[2:]
            t = mr.window_partition_ref(x, window_size[i])
            for j in range(depth):
                t = mr.block_ref(t, _sub(lp, f"blocks.{j}."), num_heads[i], state_dtype=state_dtype)
            x = mr.window_reverse_ref(t, window_size[i], H, W)
        if "downsample.reduction.0.weight" in lp:
            x = downsample_ref(x, _sub(lp, "downsample."))
    return x


def model_ref(x, params, num_heads, window_size, compute_dtype=None, state_dtype=None, training=True, new_stats=None):
    """MambaVision.forward and forward_features_mamba_fusion: x (B, 3, H, W) f32 / f64 -> (logits, fusion map), both in the dtype
    of x"""
    m = levels_ref(x, params, num_heads, window_size, compute_dtype, state_dtype, training, new_stats)
    y = batchnorm_ref(m, params, "norm", 1e-5, training, new_stats=new_stats).to(m.dtype)
    pooled = y.to(x.dtype).mean((2, 3))
    logits = pooled @ params["head.weight"].to(x.dtype).T + params["head.bias"].to(x.dtype)
    return logits, m.to(x.dtype)
