"""Mamba(d_model, d_state=16, d_conv=4, expand=2, dt_rank="auto", ...) with mamba_ssm's signature, defaults (dt_rank
ceil(d_model / 16), conv bias, no linear biases), parameter names and initialisation (reference modules/fusion_blocks.py:264-292
with the defaults; ConNexT/models/block/len4mamba.py:74-79,138-143 with d_state 128).  The projections are hamspine GEMMs, the
conv and the scan the kernels of hamspine.ssm, which take d_conv 4 and d_state in ssm.D_STATES."""
import math

import torch
import torch.nn as nn

from .. import functional as F
from .. import ssm
from .layers import Linear


def low_rank_weights(wx, wdt, R):
    """x_proj / dt_proj weights with the dt rank R padded to a multiple of 8 by zero rows / columns: the bf16 GEMM moves
    16-byte chunks, so a K or a row pitch of 3 (d_model 40) would not be accepted.  The zero rows of x_proj make the
    padding columns of its output exact zeros, which is the zero padding the dt_proj GEMM's K tail needs."""
    Rp = -(-R // 8) * 8
    if Rp != R:
        wx = torch.cat([wx[:R], wx.new_zeros(Rp - R, wx.shape[1]), wx[R:]], dim=0)
        wdt = torch.nn.functional.pad(wdt, (0, Rp - R))
    return Rp, wx, wdt


class Mamba(nn.Module):
    def __init__(self, d_model, d_state=ssm.D_STATE, d_conv=ssm.D_CONV, expand=2, dt_rank="auto", dt_min=1e-3, dt_max=1e-1,
                 dt_init_floor=1e-4):
        super().__init__()
        if d_conv != ssm.D_CONV:
            raise NotImplementedError(f"Mamba: d_conv {d_conv} is not implemented (the conv1d kernel has {ssm.D_CONV} taps)")
        if d_state not in ssm.D_STATES:
            raise NotImplementedError(f"Mamba: d_state {d_state} is not implemented (the scan kernels take {ssm.D_STATES})")
        self.d_model = d_model
        self.d_state, self.d_conv, self.expand = d_state, d_conv, expand
        self.d_inner = d = int(self.expand * d_model)
        self.dt_rank = R = math.ceil(d_model / 16) if dt_rank == "auto" else int(dt_rank)
        self.in_proj = Linear(d_model, 2 * d, bias=False)
        # parameter holder: (d, 1, 4) weight and (d,) bias with torch's Conv1d initialisation
        self.conv1d = nn.Conv1d(d, d, self.d_conv, groups=d, padding=self.d_conv - 1, bias=True)
        self.x_proj = Linear(d, R + 2 * self.d_state, bias=False)
        self.dt_proj = Linear(R, d, bias=True)
        nn.init.uniform_(self.dt_proj.weight, -R ** -0.5, R ** -0.5)
        # dt_proj.bias = softplus^-1(dt), dt log-uniform in [dt_min, dt_max]
        dt = torch.exp(torch.rand(d) * (math.log(dt_max) - math.log(dt_min)) + math.log(dt_min)).clamp(min=dt_init_floor)
        with torch.no_grad():
            self.dt_proj.bias.copy_(dt + torch.log(-torch.expm1(-dt)))
        self.A_log = nn.Parameter(torch.log(torch.arange(1, self.d_state + 1, dtype=torch.float32)).repeat(d, 1).contiguous())
        self.A_log._no_weight_decay = True
        self.D = nn.Parameter(torch.ones(d))
        self.D._no_weight_decay = True
        self.out_proj = Linear(d, d_model, bias=False)

    def _low_rank_weights(self):
        return low_rank_weights(self.x_proj.weight, self.dt_proj.weight, self.dt_rank)

    def forward(self, x, mean_tokens=False, residual=None, out_dtype=None):
        """x (B, L, d_model) in the compute dtype -> (B, L, d_model); with mean_tokens the f32 mean over L, (B, d_model),
        taken before out_proj (which has no bias, so the two commute): one (B, d_inner) GEMM instead of (B L, d_inner).
        `residual` (B, L, d_model) is added in out_proj's epilogue and `out_dtype` (f32 for a bf16 block at a boundary)
        is the dtype that GEMM writes; neither combines with mean_tokens, whose result is already f32 and has no token axis."""
        if mean_tokens and (residual is not None or out_dtype is not None):
            raise ValueError("Mamba.forward: residual / out_dtype do not combine with mean_tokens")
        d = self.d_inner
        xz = F.linear(x, self.in_proj.weight)                               # (B, L, 2d) = [xs | z]
        xs, z = ssm.split_views(xz, d)
        u = ssm.causal_conv1d(xs, self.conv1d.weight, self.conv1d.bias)
        Rp, wx, wdt = self._low_rank_weights()
        dt_r, bc = ssm.split_copy(F.linear(u, wx), Rp)                      # (B, L, Rp), (B, L, 2N) = [Bm | Cm]
        dt = F.linear(dt_r, wdt)                                            # dt_proj.bias is added inside the scan
        y = ssm.selective_scan(u, dt, self.dt_proj.bias, self.A_log, bc, self.D, z)
        if mean_tokens:
            return F.linear(F.mean_tokens(y, out_f32=True), self.out_proj.weight)
        return F.linear(y, self.out_proj.weight, residual=residual, out_dtype=out_dtype)
