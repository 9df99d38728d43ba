"""MambaVision (reference ConNexT/models/block/mamba_vision.py:1301-2472) with the reference's constructor signatures, defaults,
attribute names and state-dict keys, on the hamspine kernels: window_partition, window_reverse, _load_state_dict, _load_checkpoint,
Downsample, PatchEmbed, ConvBlock, MambaVisionMixer, Attention, Block, MambaVisionLayer, MambaVision, the eleven mamba_vision_*
factories, MambaVisionEncoder and create_mamba_vision_encoder.  The reference imports timm, einops and mamba_ssm; nothing here
does.  Nothing here downloads either: a factory called with pretrained=True and no file at model_path raises FileNotFoundError.

The levels of MambaVision are MambaVisionStage, not MambaVisionLayer.  MambaVisionLayer is the token stage on its own
((B, C, H, W) f32 in and out) and keeps refusing conv=True and downsample=True; MambaVisionStage has the reference
MambaVisionLayer's signature, attributes (conv, transformer_block, blocks, downsample, do_gt, window_size) and state-dict keys and
builds either ConvBlocks or the hybrid Blocks, plus the optional Downsample, so a reference checkpoint loads key for key.

What runs where.  in_proj, x_proj, dt_proj, out_proj, qkv, proj, fc1, fc2 and head are hamspine GEMMs; the two centred depthwise
convs + SiLU, the 8-state gate-less scan and the window partition / reverse are the kernels of hamspine.mambavision_ops; the
attention is hamspine.functional.MHAFn with qkv.weight as the packed projection (its rows are ordered q | k | v with the heads
inside each, as nn.MultiheadAttention.in_proj_weight); LayerNorm, the erf-GELU MLP (functional.mlp_gelu) and layer scale +
residual + stochastic depth (convnext_ops.layer_scale_residual with one keep/drop draw per window row) are the existing nodes.
The conv of the z half writes straight into the right half of the buffer out_proj reads and the scan into the left half, so
the reference's torch.cat([y, z]) is no launch.  The 3x3 convolutions of PatchEmbed, ConvBlock and Downsample, BatchNorm with
ConvBlock's tanh-GELU and layer scale + stochastic depth + residual epilogues, the image packing and the window partition /
reverse of an NHWC map are the nodes of hamspine.mambavision_conv_ops (csrc/mvconv.hip; hs_gemm's convolution core where C and
Kout are multiples of 64, i.e. the B and L3 variants).  Where one window covers the whole map (every 224-pixel factory) the
partition and the reverse between the stages are views.

Dtype policy.  The image enters as (B, 3, H, W) f32 and is packed to NHWC rows of 8 channels in the compute dtype
(hamspine.set_compute_dtype).  Every activation between PatchEmbed and the last window reverse, the residual streams included,
is in the compute dtype: conv-stage maps are (B, C, H, W)-shaped over NHWC memory with the channel pitch ceil8(C) and zero pad
lanes (only C = 196 and the image are padded), token stages hold (windows, tokens, C).  Parameters stay f32: the GEMMs and the
convolutions read compute-dtype copies of their weights, the depthwise convs, the scan (A_log, D, dt_proj.bias), LayerNorm,
BatchNorm and layer scale read f32 parameters.  BatchNorm statistics, the scan's state and every sum (conv taps, state sum,
normalisation statistics, softmax, GEMM and convolution accumulators) are f32.  The model's outputs are f32: the logits, the
pooled features, and the map of forward_features_mamba_fusion, which is NCHW-contiguous (MambaVisionEncoder's reshape reads
that memory).  MambaVisionLayer takes and returns (B, C, H, W) f32: its window partition casts to the compute dtype and its
window reverse casts back.  PatchEmbed, ConvBlock, Downsample and MambaVisionStage called on their own return compute-dtype
maps; MambaVisionMixer, Attention and Block called on their own run in the dtype of their input."""
import math
from pathlib import Path

import torch
import torch.nn as nn

import hamspine
from hamspine import functional as F
from hamspine import mambavision_conv_ops as cops
from hamspine import mambavision_ops as ops
from hamspine import ssm
from hamspine.convnext_ops import layer_scale_residual
from hamspine.nn.convnext import _drop_path_scale
from hamspine.nn.layers import Dropout, LayerNorm, Linear
from hamspine.nn.mamba import low_rank_weights
from hamspine.nn.resnet import BatchNormParams


def window_partition(x, window_size):
    """x (B, C, H, W) f32 -> (num_windows * B, window_size * window_size, C) f32.  Unlike the reference's, H and W need not be
    multiples of the window: the right and bottom are filled with zeros up to the next multiple."""
    return ops.window_partition(x, window_size, torch.float32)


def window_reverse(windows, window_size, H, W):
    """windows (num_windows * B, window_size * window_size, C) -> (B, C, H, W) f32; where H or W is no multiple of the window,
    the tokens of the padded positions are dropped."""
    return ops.window_reverse(windows, window_size, H, W)


class _ConvParams(nn.Conv1d):
    """parameter holder: the (d, 1, k) depthwise weight with torch's Conv1d initialisation"""

    def forward(self, x):
        raise RuntimeError("executed by the parent module")


class MambaVisionMixer(nn.Module):
    def __init__(self, d_model, d_state=16, d_conv=4, expand=2, dt_rank="auto", dt_min=0.001, dt_max=0.1, dt_init="random",
                 dt_scale=1.0, dt_init_floor=1e-4, conv_bias=True, bias=False, use_fast_path=True, layer_idx=None, device=None,
                 dtype=None):
        factory_kwargs = {"device": device, "dtype": dtype}
        super().__init__()
        if d_state != ops.D_STATE or d_conv != ops.D_CONV:
            raise NotImplementedError(f"MambaVisionMixer: d_state {d_state}, d_conv {d_conv} is not implemented (the kernels take "
                                      f"d_state {ops.D_STATE} and d_conv {ops.D_CONV}, what Block builds)")
        self.d_model = d_model
        self.d_state = d_state
        self.d_conv = d_conv
        self.expand = expand
        self.d_inner = int(self.expand * self.d_model)
        self.dt_rank = math.ceil(self.d_model / 16) if dt_rank == "auto" else dt_rank
        self.use_fast_path = use_fast_path
        self.layer_idx = layer_idx
        d = self.d_inner // 2
        self.in_proj = Linear(self.d_model, self.d_inner, bias=bias, **factory_kwargs)
        self.x_proj = Linear(d, self.dt_rank + self.d_state * 2, bias=False, **factory_kwargs)
        self.dt_proj = Linear(self.dt_rank, d, bias=True, **factory_kwargs)
        dt_init_std = self.dt_rank ** -0.5 * dt_scale
        if dt_init == "constant":
            nn.init.constant_(self.dt_proj.weight, dt_init_std)
        elif dt_init == "random":
            nn.init.uniform_(self.dt_proj.weight, -dt_init_std, dt_init_std)
        else:
            raise NotImplementedError
        # dt_proj.bias = softplus^-1(dt), dt log-uniform in [dt_min, dt_max]
        dt = torch.exp(torch.rand(d, **factory_kwargs) * (math.log(dt_max) - math.log(dt_min)) + math.log(dt_min))
        dt = dt.clamp(min=dt_init_floor)
        with torch.no_grad():
            self.dt_proj.bias.copy_(dt + torch.log(-torch.expm1(-dt)))
        self.dt_proj.bias._no_reinit = True
        A = torch.arange(1, self.d_state + 1, dtype=torch.float32, device=device).repeat(d, 1).contiguous()
        self.A_log = nn.Parameter(torch.log(A))
        self.A_log._no_weight_decay = True
        self.D = nn.Parameter(torch.ones(d, device=device))
        self.D._no_weight_decay = True
        self.out_proj = Linear(self.d_inner, self.d_model, bias=bias, **factory_kwargs)
        # bias=conv_bias // 2 as in the reference: True // 2 is 0, so with the default the two convs have no bias parameter
        self.conv1d_x = _ConvParams(d, d, d_conv, groups=d, bias=conv_bias // 2, **factory_kwargs)
        self.conv1d_z = _ConvParams(d, d, d_conv, groups=d, bias=conv_bias // 2, **factory_kwargs)

    def forward(self, hidden_states):
        """hidden_states (B, L, d_model) -> (B, L, d_model) in the same dtype"""
        d = self.d_inner // 2
        xz = F.linear(hidden_states, self.in_proj.weight, self.in_proj.bias)            # (B, L, 2d) = [x | z]
        xs, z = ssm.split_views(xz, d)
        yz = torch.empty_like(xz)                                                       # [scan output | conv(z)]: out_proj's input
        u = ops.conv1d_same_silu(xs, self.conv1d_x.weight, self.conv1d_x.bias)
        zc = ops.conv1d_same_silu(z, self.conv1d_z.weight, self.conv1d_z.bias, out=yz[..., d:])
        Rp, wx, wdt = low_rank_weights(self.x_proj.weight, self.dt_proj.weight, self.dt_rank)
        dt_r, bc = ssm.split_copy(F.linear(u, wx), Rp)                                  # (B, L, Rp), (B, L, 16) = [Bm | Cm]
        # the reference applies dt_proj with its bias (1619) and passes the bias to the scan as delta_bias too (1629), so
        # delta = softplus(W dt + 2 b); checkpoints were trained that way.  Once in the GEMM epilogue, once inside the scan.
        dt = F.linear(dt_r, wdt, self.dt_proj.bias)
        y = ops.selective_scan_nogate(u, dt, self.dt_proj.bias, self.A_log, bc, self.D, out=yz[..., :d])
        return F.linear(ops.join_halves(y, zc, yz), self.out_proj.weight, self.out_proj.bias)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_norm=False, attn_drop=0., proj_drop=0., norm_layer=nn.LayerNorm):
        super().__init__()
        assert dim % num_heads == 0
        if qk_norm:
            raise NotImplementedError("Attention: qk_norm is not implemented (no factory of the reference sets it)")
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.fused_attn = True
        self.qkv = Linear(dim, dim * 3, bias=qkv_bias)
        self.q_norm = nn.Identity()
        self.k_norm = nn.Identity()
        self.attn_drop = nn.Dropout(attn_drop)          # holds p; the dropout runs inside the attention node
        self.proj = Linear(dim, dim)
        self.proj_drop = Dropout(proj_drop)

    def forward(self, x):
        meta = {"heads": self.num_heads, "dropout": float(self.attn_drop.p) if self.training else 0.0, "self_attn": True}
        y = F.MHAFn.apply(x, None, None, None, meta, self.qkv.weight, self.qkv.bias, None, None, None, self.proj.weight,
                          self.proj.bias)
        return self.proj_drop(y)


class Mlp(nn.Module):
    """timm.models.vision_transformer.Mlp as Block uses it (the default of its Mlp_block argument): fc1, erf-GELU, dropout,
    fc2, dropout; the state dict is fc1.* and fc2.*"""

    def __init__(self, in_features, hidden_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        if act_layer is not nn.GELU:
            raise NotImplementedError("Mlp: only nn.GELU (erf) is implemented")
        hidden_features = hidden_features or in_features
        self.fc1 = Linear(in_features, hidden_features)
        self.fc2 = Linear(hidden_features, in_features)
        self.drop = float(drop)

    def forward(self, x):
        if self.training and self.drop > 0:
            return self.fc2(self.fc1(x, act="gelu", dropout_p=self.drop), dropout_p=self.drop)
        return F.mlp_gelu(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias)


class Block(nn.Module):
    def __init__(self, dim, num_heads, counter, transformer_blocks, mlp_ratio=4., qkv_bias=False, qk_scale=False, drop=0.,
                 attn_drop=0., drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, Mlp_block=Mlp, layer_scale=None):
        super().__init__()
        if norm_layer is not nn.LayerNorm or Mlp_block is not Mlp:
            raise NotImplementedError("Block: only nn.LayerNorm and the default Mlp are implemented (the reference builds no "
                                      "other)")
        self.norm1 = LayerNorm(dim)
        if counter in transformer_blocks:
            self.mixer = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_norm=qk_scale, attn_drop=attn_drop,
                                   proj_drop=drop, norm_layer=norm_layer)
        else:
            self.mixer = MambaVisionMixer(d_model=dim, d_state=8, d_conv=3, expand=1)
        self.drop_path = nn.Identity()                  # the reference's attribute; the rate is applied in forward
        self.drop_path_rate = float(drop_path)
        self.norm2 = LayerNorm(dim)
        self.mlp = Mlp_block(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        if layer_scale is not None and type(layer_scale) in [int, float]:
            self.gamma_1 = nn.Parameter(layer_scale * torch.ones(dim))
            self.gamma_2 = nn.Parameter(layer_scale * torch.ones(dim))
        else:
            self.gamma_1 = self.gamma_2 = 1
            self.register_buffer("_unit_scale", torch.ones(dim), persistent=False)

    def forward(self, x):
        """x (windows, tokens, dim) -> the same; stochastic depth draws once per window row and branch"""
        g1, g2 = (self.gamma_1, self.gamma_2) if isinstance(self.gamma_1, nn.Parameter) else (self._unit_scale, self._unit_scale)
        x = layer_scale_residual(self.mixer(self.norm1(x)), g1, x, _drop_path_scale(x, self.drop_path_rate, self.training))
        return layer_scale_residual(self.mlp(self.norm2(x)), g2, x, _drop_path_scale(x, self.drop_path_rate, self.training))


class MambaVisionLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size, conv=False, downsample=True, mlp_ratio=4., qkv_bias=True,
                 qk_scale=None, drop=0., attn_drop=0., drop_path=0., layer_scale=None, layer_scale_conv=None,
                 transformer_blocks=[]):
        super().__init__()
        if conv:
            raise NotImplementedError("MambaVisionLayer: conv=True (the ConvBlock stages 1 and 2) is not implemented yet; it is "
                                      "the follow-up with PatchEmbed, Downsample and the MambaVision wrappers")
        if downsample:
            raise NotImplementedError("MambaVisionLayer: downsample=True (the 3x3 stride-2 Downsample) is not implemented yet; it "
                                      "is the follow-up with PatchEmbed, ConvBlock and the MambaVision wrappers")
        self.conv = conv
        self.transformer_block = True
        self.blocks = nn.ModuleList([Block(dim=dim, counter=i, transformer_blocks=transformer_blocks, num_heads=num_heads,
                                           mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop,
                                           attn_drop=attn_drop,
                                           drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path,
                                           layer_scale=layer_scale) for i in range(depth)])
        self.downsample = None
        self.do_gt = False
        self.window_size = window_size

    def forward(self, x):
        """x (B, C, H, W) f32 -> (B, C, H, W) f32"""
        _, _, H, W = x.shape
        if x.dtype != torch.float32:
            x = x.float()
        x = ops.window_partition(x, self.window_size, hamspine.compute_dtype())
        for blk in self.blocks:
            x = blk(x)
        return ops.window_reverse(x, self.window_size, H, W)


# --------------------------------------------------------------------------------------------------------------------------------
# the convolutional half, the full model, the factories and the encoder (reference lines 1333-1524, 1833-2472)
# --------------------------------------------------------------------------------------------------------------------------------
class _Conv2dParams(nn.Conv2d):
    """parameter holder: the (Kout, C, 3, 3) weight and optional bias in nn.Conv2d's layout and initialisation"""

    def forward(self, x):
        raise RuntimeError("executed by the parent module")


class _BatchNormParams(BatchNormParams):
    """BatchNorm2d parameter / buffer holder with its own eps; num_batches_tracked is counted as BatchNormParams does"""

    def __init__(self, c, eps=1e-5):
        super().__init__(c)
        self.eps = eps


def _bn(x, bn, training, relu=False):
    if training:
        bn.bump()
    return cops.batch_norm(x, bn, training, relu)


def _as_map(x):
    """whatever reaches a conv module on its own -> the compute dtype (a map of it passes through)"""
    dt = hamspine.compute_dtype()
    return x if x.dtype == dt else x.to(dt)


def _load_state_dict(module, state_dict, strict=False, logger=None):
    """module.load_state_dict that reports a mismatch (print, or logger.warning) instead of raising unless `strict`; missing
    num_batches_tracked entries are not counted"""
    result = module.load_state_dict(state_dict, strict=False)
    missing = [k for k in result.missing_keys if "num_batches_tracked" not in k]
    err_msg = []
    if result.unexpected_keys:
        err_msg.append("unexpected key in source state_dict: " + ", ".join(result.unexpected_keys) + "\n")
    if missing:
        err_msg.append("missing keys in source state_dict: " + ", ".join(missing) + "\n")
    if err_msg:
        err_msg = "\n".join(["The model and loaded state dict do not match exactly\n"] + err_msg)
        if strict:
            raise RuntimeError(err_msg)
        if logger is not None:
            logger.warning(err_msg)
        else:
            print(err_msg)


def _load_checkpoint(model, filename, map_location="cpu", strict=False, logger=None):
    """loads a local checkpoint file: the `state_dict` / `model` wrappers and the `module.` / `encoder.` prefixes are accepted"""
    checkpoint = torch.load(filename, map_location=map_location, weights_only=False)
    if not isinstance(checkpoint, dict):
        raise RuntimeError(f"No state_dict found in checkpoint file {filename}")
    if "state_dict" in checkpoint:
        state_dict = checkpoint["state_dict"]
    elif "model" in checkpoint:
        state_dict = checkpoint["model"]
    else:
        state_dict = checkpoint
    if list(state_dict.keys())[0].startswith("module."):
        state_dict = {k[7:]: v for k, v in state_dict.items()}
    if sorted(state_dict.keys())[0].startswith("encoder"):
        state_dict = {k.replace("encoder.", ""): v for k, v in state_dict.items() if k.startswith("encoder.")}
    _load_state_dict(model, state_dict, strict, logger)
    return checkpoint


class Downsample(nn.Module):
    def __init__(self, dim, keep_dim=False):
        super().__init__()
        dim_out = dim if keep_dim else 2 * dim
        self.reduction = nn.Sequential(_Conv2dParams(dim, dim_out, 3, 2, 1, bias=False))

    def forward(self, x):
        """x (B, dim, H, W) -> (B, dim_out, ceil(H / 2), ceil(W / 2)), a map of the compute dtype"""
        return cops.conv3x3(_as_map(x), self.reduction[0].weight, None, stride=2)


class PatchEmbed(nn.Module):
    def __init__(self, in_chans=3, in_dim=64, dim=96):
        super().__init__()
        self.proj = nn.Identity()
        self.conv_down = nn.Sequential(_Conv2dParams(in_chans, in_dim, 3, 2, 1, bias=False), _BatchNormParams(in_dim, eps=1e-4),
                                       nn.ReLU(), _Conv2dParams(in_dim, dim, 3, 2, 1, bias=False),
                                       _BatchNormParams(dim, eps=1e-4), nn.ReLU())

    def forward(self, x):
        """x (B, in_chans, H, W) f32 -> (B, dim, H / 4, W / 4), a map of the compute dtype"""
        cd = self.conv_down
        x = cops.pack_image(x, hamspine.compute_dtype())
        x = _bn(cops.conv3x3(x, cd[0].weight, None, stride=2), cd[1], self.training, relu=True)
        return _bn(cops.conv3x3(x, cd[3].weight, None, stride=2), cd[4], self.training, relu=True)


class ConvBlock(nn.Module):
    def __init__(self, dim, drop_path=0., layer_scale=None, kernel_size=3):
        super().__init__()
        if kernel_size != 3:
            raise NotImplementedError("ConvBlock: only kernel_size 3 is implemented (the reference builds no other)")
        self.conv1 = _Conv2dParams(dim, dim, kernel_size=kernel_size, stride=1, padding=1)
        self.norm1 = _BatchNormParams(dim, eps=1e-5)
        self.act1 = nn.GELU(approximate="tanh")         # runs inside norm1's apply pass
        self.conv2 = _Conv2dParams(dim, dim, kernel_size=kernel_size, stride=1, padding=1)
        self.norm2 = _BatchNormParams(dim, eps=1e-5)
        self.layer_scale = layer_scale
        if layer_scale is not None and type(layer_scale) in [int, float]:
            self.gamma = nn.Parameter(layer_scale * torch.ones(dim))
            self.layer_scale = True
        else:
            self.layer_scale = False
        self.drop_path = nn.Identity()                  # the reference's attribute; the rate is applied in forward
        self.drop_path_rate = float(drop_path)

    def forward(self, x):
        """x (B, dim, H, W) -> the same, a map of the compute dtype; stochastic depth draws once per sample"""
        x = _as_map(x)
        tr = self.training
        if tr:
            self.norm1.bump()
            self.norm2.bump()
        h = cops.batch_norm_gelu_tanh(cops.conv3x3(x, self.conv1.weight, self.conv1.bias), self.norm1, tr)
        h = cops.conv3x3(h, self.conv2.weight, self.conv2.bias)
        return cops.batch_norm_scale_residual(h, self.norm2, tr, x, self.gamma if self.layer_scale else None,
                                              _drop_path_scale(x, self.drop_path_rate, tr))


class MambaVisionStage(nn.Module):
    """One level of MambaVision: the reference's MambaVisionLayer with every option - ConvBlocks (conv=True) or the hybrid Blocks
    over windows, and an optional Downsample - under the reference's attribute names and state-dict keys.  A class of its own
    because MambaVisionLayer's constructor keeps refusing conv=True and downsample=True."""

    def __init__(self, dim, depth, num_heads, window_size, conv=False, downsample=True, mlp_ratio=4., qkv_bias=True,
                 qk_scale=None, drop=0., attn_drop=0., drop_path=0., layer_scale=None, layer_scale_conv=None,
                 transformer_blocks=[]):
        super().__init__()
        self.conv = conv
        rate = lambda i: drop_path[i] if isinstance(drop_path, list) else drop_path
        if conv:
            self.blocks = nn.ModuleList([ConvBlock(dim=dim, drop_path=rate(i), layer_scale=layer_scale_conv) for i in range(depth)])
            self.transformer_block = False
        else:
            self.blocks = nn.ModuleList([Block(dim=dim, counter=i, transformer_blocks=transformer_blocks, num_heads=num_heads,
                                               mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop,
                                               attn_drop=attn_drop, drop_path=rate(i), layer_scale=layer_scale)
                                         for i in range(depth)])
            self.transformer_block = True
        self.downsample = None if not downsample else Downsample(dim=dim)
        self.do_gt = False
        self.window_size = window_size

    def forward(self, x, as_map=False):
        """x (B, C, H, W) -> a map of the compute dtype; a token stage without Downsample returns (B, C, H, W) f32 in NCHW memory
        unless as_map"""
        x = _as_map(x)
        _, _, H, W = x.shape
        if self.transformer_block:
            x = cops.window_partition_nhwc(x, self.window_size)
        for blk in self.blocks:
            x = blk(x)
        if self.transformer_block:
            if self.downsample is None and not as_map:
                return ops.window_reverse(x, self.window_size, H, W)
            x = cops.window_reverse_nhwc(x, self.window_size, H, W)
        return x if self.downsample is None else self.downsample(x)


class MambaVision(nn.Module):
    def __init__(self, dim, in_dim, depths, window_size, mlp_ratio, num_heads, drop_path_rate=0.2, in_chans=3, num_classes=1000,
                 qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., layer_scale=None, layer_scale_conv=None, **kwargs):
        super().__init__()
        num_features = int(dim * 2 ** (len(depths) - 1))
        self.num_classes = num_classes
        self.patch_embed = PatchEmbed(in_chans=in_chans, in_dim=in_dim, dim=dim)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths), device="cpu")]
        self.levels = nn.ModuleList()
        for i in range(len(depths)):
            conv = i == 0 or i == 1
            half = depths[i] // 2
            self.levels.append(MambaVisionStage(
                dim=int(dim * 2 ** i), depth=depths[i], num_heads=num_heads[i], window_size=window_size[i], mlp_ratio=mlp_ratio,
                qkv_bias=qkv_bias, qk_scale=qk_scale, conv=conv, drop=drop_rate, attn_drop=attn_drop_rate,
                drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], downsample=(i < 3), layer_scale=layer_scale,
                layer_scale_conv=layer_scale_conv,
                transformer_blocks=list(range(half + 1, depths[i])) if depths[i] % 2 != 0 else list(range(half, depths[i]))))
        self.norm = _BatchNormParams(num_features)
        self.avgpool = nn.AdaptiveAvgPool2d(1)          # runs as the token mean behind norm
        self.head = Linear(num_features, num_classes) if num_classes > 0 else nn.Identity()
        self.apply(self._init_weights)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)

    @torch.jit.ignore
    def no_weight_decay_keywords(self):
        return {"rpb"}

    def _levels(self, x, as_map):
        x = self.patch_embed(x)
        for i, level in enumerate(self.levels):
            x = level(x, as_map=as_map or i + 1 < len(self.levels))
        return x

    def forward_features(self, x):
        """x (B, in_chans, H, W) f32 -> (B, num_features) pooled features"""
        m = _bn(self._levels(x, True), self.norm, self.training)
        B, C, H, W = m.shape
        tokens = m.permute(0, 2, 3, 1).reshape(B, H * W, C)     # a view: the memory is NHWC
        # a class count that is no multiple of 8 cannot be a bf16 leading dimension: such a head runs in f32
        wide = isinstance(self.head, nn.Identity) or self.head.out_features % 8 != 0
        return F.mean_tokens(tokens, out_f32=wide)

    def forward_features_mamba_fusion(self, x):
        """x (B, in_chans, H, W) f32 -> the last level's map (B, num_features, H / 32, W / 32) f32 in NCHW memory"""
        x = self._levels(x, False)
        return x if x.dtype == torch.float32 and x.is_contiguous() else x.float().contiguous()

    def forward(self, x):
        x = self.forward_features(x)
        if isinstance(self.head, nn.Identity):
            return x
        return self.head(x, out_dtype=torch.float32)

    def _load_state_dict(self, pretrained, strict: bool = False):
        _load_checkpoint(self, pretrained, strict=strict)


def _pretrained_cfg(resolution, crop_pct, crop_mode):
    return {"url": "", "num_classes": 1000, "input_size": (3, resolution, resolution), "pool_size": None, "crop_pct": crop_pct,
            "interpolation": "bicubic", "fixed_input_size": True, "mean": (0.485, 0.456, 0.406), "std": (0.229, 0.224, 0.225),
            "crop_mode": crop_mode}


# name -> (depths, num_heads, window_size, dim, in_dim, resolution, drop_path_rate, layer_scale or None, crop_pct, crop_mode)
_VARIANTS = {
    "mamba_vision_T": ([1, 3, 8, 4], [2, 4, 8, 16], [8, 8, 14, 7], 80, 32, 224, 0.2, None, 1.0, "center"),
    "mamba_vision_T2": ([1, 3, 11, 4], [2, 4, 8, 16], [8, 8, 14, 7], 80, 32, 224, 0.2, None, 0.98, "center"),
    "mamba_vision_S": ([3, 3, 7, 5], [2, 4, 8, 16], [8, 8, 14, 7], 96, 64, 224, 0.2, None, 0.93, "center"),
    "mamba_vision_B": ([3, 3, 10, 5], [2, 4, 8, 16], [8, 8, 14, 7], 128, 64, 224, 0.3, 1e-5, 1.0, "center"),
    "mamba_vision_B_21k": ([3, 3, 10, 5], [2, 4, 8, 16], [8, 8, 14, 7], 128, 64, 224, 0.3, 1e-5, 1.0, "center"),
    "mamba_vision_L": ([3, 3, 10, 5], [4, 8, 16, 32], [8, 8, 14, 7], 196, 64, 224, 0.3, 1e-5, 1.0, "center"),
    "mamba_vision_L_21k": ([3, 3, 10, 5], [4, 8, 16, 32], [8, 8, 14, 7], 196, 64, 224, 0.3, 1e-5, 1.0, "center"),
    "mamba_vision_L2": ([3, 3, 12, 5], [4, 8, 16, 32], [8, 8, 14, 7], 196, 64, 224, 0.3, 1e-5, 1.0, "center"),
    "mamba_vision_L2_512_21k": ([3, 3, 12, 5], [4, 8, 16, 32], [8, 8, 32, 16], 196, 64, 512, 0.3, 1e-5, 0.93, "squash"),
    "mamba_vision_L3_256_21k": ([3, 3, 20, 10], [4, 8, 16, 32], [8, 8, 16, 8], 256, 64, 256, 0.5, 1e-5, 1.0, "center"),
    "mamba_vision_L3_512_21k": ([3, 3, 20, 10], [4, 8, 16, 32], [8, 8, 32, 16], 256, 64, 512, 0.5, 1e-5, 0.93, "squash"),
}


def _build_variant(name, pretrained, kwargs):
    depths, num_heads, window_size, dim, in_dim, resolution, dpr, layer_scale, crop_pct, crop_mode = _VARIANTS[name]
    model_path = kwargs.pop("model_path", f"/tmp/{name}.pth.tar")
    cfg = dict(depths=kwargs.pop("depths", list(depths)), num_heads=kwargs.pop("num_heads", list(num_heads)),
               window_size=kwargs.pop("window_size", list(window_size)), dim=kwargs.pop("dim", dim),
               in_dim=kwargs.pop("in_dim", in_dim), mlp_ratio=kwargs.pop("mlp_ratio", 4),
               resolution=kwargs.pop("resolution", resolution), drop_path_rate=kwargs.pop("drop_path_rate", dpr))
    if layer_scale is not None:                          # B and larger: layer scale on the token stages, none on the conv stages
        cfg["layer_scale"] = kwargs.pop("layer_scale", layer_scale)
        cfg["layer_scale_conv"] = None
    if pretrained and not Path(model_path).is_file():
        # the reference fetches the weights here; this package never downloads
        raise FileNotFoundError(f"{name}(pretrained=True): no checkpoint at {model_path}; place the weights there or pass model_path")
    model = MambaVision(**cfg, **kwargs)
    model.pretrained_cfg = _pretrained_cfg(resolution, crop_pct, crop_mode)
    model.default_cfg = model.pretrained_cfg
    if pretrained:
        model._load_state_dict(model_path)
    return model


def mamba_vision_T(pretrained=False, **kwargs):
    return _build_variant("mamba_vision_T", pretrained, kwargs)


def mamba_vision_T2(pretrained=False, **kwargs):
    return _build_variant("mamba_vision_T2", pretrained, kwargs)


def mamba_vision_S(pretrained=False, **kwargs):
    return _build_variant("mamba_vision_S", pretrained, kwargs)


def mamba_vision_B(pretrained=False, **kwargs):
    return _build_variant("mamba_vision_B", pretrained, kwargs)


def mamba_vision_B_21k(pretrained=False, **kwargs):
    return _build_variant("mamba_vision_B_21k", pretrained, kwargs)


def mamba_vision_L(pretrained=False, **kwargs):
    return _build_variant("mamba_vision_L", pretrained, kwargs)


def mamba_vision_L_21k(pretrained=False, **kwargs):
    return _build_variant("mamba_vision_L_21k", pretrained, kwargs)


def mamba_vision_L2(pretrained=False, **kwargs):
    return _build_variant("mamba_vision_L2", pretrained, kwargs)


def mamba_vision_L2_512_21k(pretrained=False, **kwargs):
    return _build_variant("mamba_vision_L2_512_21k", pretrained, kwargs)


def mamba_vision_L3_256_21k(pretrained=False, **kwargs):
    return _build_variant("mamba_vision_L3_256_21k", pretrained, kwargs)


def mamba_vision_L3_512_21k(pretrained=False, **kwargs):
    return _build_variant("mamba_vision_L3_512_21k", pretrained, kwargs)


class MambaVisionEncoder(nn.Module):
    """The image encoder of the Mamba fusion: a MambaVision without its classification head whose last feature map leaves as
    (B, 1568, -1), the reshape of the reference (the map's NCHW memory read in rows of C H W / 1568).  `projection` is kept,
    unused, for the state dict."""

    _PATHS = {"S": ("mamba_vision_S", "/tmp/mamba_vision_S.pth.tar"), "T": ("mamba_vision_T", "/tmp/mamba_vision_T.pth.tar"),
              "L3-512-21K": ("mamba_vision_L3_512_21k", "/tmp/mamba_vision_L3_512_21K.pth.tar"),
              "L2": ("mamba_vision_L2", "/data/sb/aaa_final_isic/MambaVision-L2-512-21K/mamba_vision_L2_512_21k.pth.tar")}

    def __init__(self, output_dim=768, pretrained=True, model_variant="L2"):
        super().__init__()
        if model_variant not in self._PATHS:
            raise ValueError(f"Unsupported MambaVision variant: {model_variant}")
        name, path = self._PATHS[model_variant]
        self.mamba_vision = _build_variant(name, pretrained, {"model_path": path})
        feature_dim = self.mamba_vision.head.in_features
        self.mamba_vision.head = nn.Identity()
        self.projection = nn.Linear(feature_dim, output_dim)

    def forward(self, x):
        features = self.mamba_vision.forward_features_mamba_fusion(x)
        return features.reshape(features.shape[0], 1568, -1)


def create_mamba_vision_encoder(output_dim=512, pretrained=True, model_variant="L2", model_paths=None):
    """MambaVisionEncoder for `model_variant`; as in the reference, variants the encoder does not name raise ValueError there"""
    names = ("T", "T2", "S", "B", "B_21k", "L", "L_21k", "L2", "L2_512_21k", "L3_256_21k", "L3_512_21k")
    default_paths = {n: f"/tmp/mamba_vision_{n}.pth.tar" for n in names}
    model_path = model_paths.get(model_variant, default_paths.get(model_variant)) if model_paths else default_paths.get(model_variant)
    if not model_path:
        raise ValueError(f"Unsupported model variant: {model_variant}")
    return MambaVisionEncoder(output_dim=output_dim, pretrained=pretrained, model_variant=model_variant)
