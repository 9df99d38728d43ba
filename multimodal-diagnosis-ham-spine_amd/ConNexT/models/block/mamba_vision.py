"""MambaVisionMixer, Attention, Block, MambaVisionLayer, window_partition and window_reverse (reference
ConNexT/models/block/mamba_vision.py:1301-1330,1527-1830: stages 3 and 4 of MambaVision, windows of tokens through blocks that
alternate the Mamba mixer and self-attention) with the reference's constructor signatures, defaults, attribute names and
state-dict keys, on the hamspine kernels.  The reference imports timm, einops and mamba_ssm; nothing here does.

Not here yet (the follow-up): the convolutional half of the tower (PatchEmbed, ConvBlock, Downsample), the MambaVision /
MambaVisionEncoder wrappers and the mamba_vision_* factories.  MambaVisionLayer(conv=True) and (downsample=True) say so.

What runs where.  in_proj, x_proj, dt_proj, out_proj, qkv, proj, fc1 and fc2 are hamspine GEMMs; the two centred depthwise
convs + SiLU, the 8-state gate-less scan and the window partition / reverse are the kernels of hamspine.mambavision_ops; the
attention is hamspine.functional.MHAFn with qkv.weight as the packed projection (its rows are ordered q | k | v with the heads
inside each, as nn.MultiheadAttention.in_proj_weight); LayerNorm, the erf-GELU MLP (functional.mlp_gelu) and layer scale +
residual + stochastic depth (convnext_ops.layer_scale_residual with one keep/drop draw per window row) are the existing nodes.
The conv of the z half writes straight into the right half of the buffer out_proj reads and the scan into the left half, so
the reference's torch.cat([y, z]) is no launch.

Dtype policy.  MambaVisionLayer takes and returns (B, C, H, W) f32.  The window partition casts to the compute dtype
(hamspine.set_compute_dtype) and the window reverse casts back to f32; between the two every activation, the residual stream
included, is in the compute dtype.  Parameters stay f32: the GEMMs read bf16 copies of their weights in bf16 mode, the convs,
the scan (A_log, D, dt_proj.bias), LayerNorm and layer scale read f32 parameters.  The scan's state and every sum (conv taps,
state sum, LayerNorm statistics, softmax, GEMM accumulators) are f32.  MambaVisionMixer, Attention and Block called on their own
run in the dtype of their input."""
import math

import torch
import torch.nn as nn

import hamspine
from hamspine import functional as F
from hamspine import mambavision_ops as ops
from hamspine import ssm
from hamspine.convnext_ops import layer_scale_residual
from hamspine.nn.convnext import _drop_path_scale
from hamspine.nn.layers import Dropout, LayerNorm, Linear
from hamspine.nn.mamba import low_rank_weights


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
