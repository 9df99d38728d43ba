"""Plain-torch restatement of stages 3 and 4 of MambaVision (reference ConNexT/models/block/mamba_vision.py:1301-1330,1527-1830):
the mixer with its two centred depthwise convs and the gate-less scan, the windowed self-attention, the Block with layer scale
and stochastic depth, and the MambaVisionLayer with its zero padding, window partition, reverse and crop.  The yardstick of the
MambaVision tests: a sequential loop over time that works in any dtype on the CPU; its float64 autograd gives the gradient
references.  `params` is a dict with the state-dict keys of the module under test.

With `compute_dtype=torch.bfloat16` the functions follow the dtype policy of the module under test: activations, the residual
stream and the GEMM operands are bfloat16; LayerNorm, the conv taps, SiLU, GELU, softmax, layer scale and the scan are evaluated
in f32 from f32 parameters and rounded once; the scan's state is f32.  With None everything runs in the dtype of the input."""
import torch
import torch.nn.functional as TF


def _wide(x):
    """what a kernel computes in: f32 for a bfloat16 activation, otherwise the dtype of x"""
    return x.float() if x.dtype == torch.bfloat16 else x


def _lin(x, w, b=None):
    """a GEMM of the module: operands in the dtype of x, bias added in the wide type, one rounding"""
    y = x @ w.to(x.dtype).T
    return y if b is None else (_wide(y) + b.to(_wide(y).dtype)).to(x.dtype)


def conv_same_ref(x, weight, bias=None):
    """silu(depthwise conv1d(x, k = 3, padding='same') [+ bias]); x (B, L, d), weight (d, 1, 3), bias (d,) or None"""
    L = x.shape[1]
    xw = _wide(x)
    xp = TF.pad(xw, (0, 0, 1, 1))
    acc = torch.zeros_like(xw) if bias is None else bias.to(xw.dtype).expand_as(xw)
    for j in range(3):
        acc = acc + xp[:, j:j + L, :] * weight[:, 0, j].to(xw.dtype)
    return TF.silu(acc).to(x.dtype)


def scan_core(u, delta_raw, dt_bias, A, Bm, Cm, D, state_dtype=None):
    """the gate-less selective scan: delta = softplus(delta_raw + dt_bias), h_t = exp(delta_t A) h_{t-1} + delta_t Bm_t u_t,
    y_t = <h_t, Cm_t> + D u_t.  u, delta_raw (B, L, d); Bm, Cm (B, L, N); A (d, N) (negative); D, dt_bias (d,).  The state and
    every sum are kept in state_dtype (default: the dtype of u) -> (B, L, d) in the dtype of u."""
    sd = state_dtype or u.dtype
    N = A.shape[-1]
    dt = TF.softplus(delta_raw.to(sd) + dt_bias.to(sd))
    A = A.to(sd)
    Bsz, L, d = u.shape
    h = torch.zeros((Bsz, d, N), dtype=sd, device=u.device)
    ys = []
    for t in range(L):
        dtt, ut = dt[:, t, :, None], u[:, t, :, None].to(sd)
        h = torch.exp(dtt * A) * h + dtt * Bm[:, t, None, :].to(sd) * ut
        ys.append((h * Cm[:, t, None, :].to(sd)).sum(-1) + D.to(sd) * u[:, t].to(sd))
    return torch.stack(ys, dim=1).to(u.dtype)


def scan_ref(u, dt_raw, dt_bias, A_log, Bm, Cm, D, state_dtype=None):
    """scan_core with A = -exp(A_log), A_log (d, N)"""
    sd = state_dtype or u.dtype
    return scan_core(u, dt_raw, dt_bias, -torch.exp(A_log.to(sd)), Bm, Cm, D, state_dtype)


def _sub(params, prefix):
    return {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix)}


def mixer_ref(x, params, state_dtype=None):
    """mamba_vision.py:1605-1636; x (B, L, H) -> (B, L, H) in the dtype of x"""
    d, N = params["A_log"].shape
    R = params["dt_proj.weight"].shape[1]
    xz = _lin(x, params["in_proj.weight"], params.get("in_proj.bias"))
    xs = conv_same_ref(xz[..., :d], params["conv1d_x.weight"], params.get("conv1d_x.bias"))
    z = conv_same_ref(xz[..., d:], params["conv1d_z.weight"], params.get("conv1d_z.bias"))
    xdbl = _lin(xs, params["x_proj.weight"])
    dt_r, Bm, Cm = xdbl[..., :R], xdbl[..., R:R + N], xdbl[..., R + N:]
    # the reference calls the whole dt_proj module (1619) and hands dt_proj.bias to the scan as delta_bias as well (1629):
    # delta = softplus(W dt + 2 b).  Pretrained weights were trained with it, so it is kept.
    dt_raw = _lin(dt_r, params["dt_proj.weight"], params["dt_proj.bias"])
    y = scan_ref(xs, dt_raw, params["dt_proj.bias"], params["A_log"], Bm, Cm, params["D"], state_dtype)
    return _lin(torch.cat([y, z], dim=-1), params["out_proj.weight"], params.get("out_proj.bias"))


def attention_ref(x, params, num_heads):
    """mamba_vision.py:1665-1686 without dropout: qkv rows are q | k | v with the heads inside each"""
    B, L, D = x.shape
    hd = D // num_heads
    qkv = _lin(x, params["qkv.weight"], params.get("qkv.bias")).reshape(B, L, 3, num_heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    att = torch.softmax(_wide(q) @ _wide(k).transpose(-2, -1) * hd ** -0.5, dim=-1).to(x.dtype)
    out = (att @ v).transpose(1, 2).reshape(B, L, D)
    return _lin(out, params["proj.weight"], params["proj.bias"])


def mlp_ref(x, params):
    h = TF.gelu(_wide(_lin(x, params["fc1.weight"], params["fc1.bias"]))).to(x.dtype)
    return _lin(h, params["fc2.weight"], params["fc2.bias"])


def _norm(x, params, name):
    xw = _wide(x)
    return TF.layer_norm(xw, xw.shape[-1:], params[name + ".weight"].to(xw.dtype), params[name + ".bias"].to(xw.dtype)).to(x.dtype)


def _residual(x, branch, gamma, rowscale):
    """x + rowscale[row] * gamma * branch: layer scale, stochastic depth per first-dimension row, residual"""
    bw = _wide(branch)
    if gamma is not None:
        bw = bw * gamma.to(bw.dtype)
    if rowscale is not None:
        bw = bw * rowscale.to(bw.dtype)[:, None, None]
    return (_wide(x) + bw).to(x.dtype)


def block_ref(x, params, num_heads, rowscale1=None, rowscale2=None, state_dtype=None):
    """mamba_vision.py:1733-1736; x (windows, tokens, dim).  rowscale*: per-row keep / (1 - p) factors of the two DropPath
    draws, or None.  The mixer is the attention when the parameters hold mixer.qkv.weight."""
    mp = _sub(params, "mixer.")
    h = _norm(x, params, "norm1")
    m = attention_ref(h, mp, num_heads) if "qkv.weight" in mp else mixer_ref(h, mp, state_dtype)
    x = _residual(x, m, params.get("gamma_1"), rowscale1)
    return _residual(x, mlp_ref(_norm(x, params, "norm2"), _sub(params, "mlp.")), params.get("gamma_2"), rowscale2)


def window_partition_ref(x, ws):
    """mamba_vision.py:1813-1820: zero padding to the right and bottom, then (B, C, H, W) -> (B nW, ws ws, C)"""
    B, C, H, W = x.shape
    x = TF.pad(x, (0, (ws - W % ws) % ws, 0, (ws - H % ws) % ws))
    Hp, Wp = x.shape[2:]
    return x.reshape(B, C, Hp // ws, ws, Wp // ws, ws).permute(0, 2, 4, 3, 5, 1).reshape(-1, ws * ws, C)


def window_reverse_ref(windows, ws, H, W):
    """mamba_vision.py:1825-1827: (B nW, ws ws, C) -> (B, C, H, W), the padded positions cropped"""
    nh, nw = -(-H // ws), -(-W // ws)
    B = windows.shape[0] // (nh * nw)
    x = windows.reshape(B, nh, nw, ws, ws, -1).permute(0, 5, 1, 3, 2, 4).reshape(B, -1, nh * ws, nw * ws)
    return x[:, :, :H, :W]


def layer_ref(x, params, num_heads, window_size, compute_dtype=None, state_dtype=None):
    """mamba_vision.py:1809-1830 with conv=False, downsample=False; x (B, C, H, W) -> (B, C, H, W) in the dtype of x.  The
    blocks run in compute_dtype (None: the dtype of x): the cast sits after the partition and before the reverse."""
    H, W = x.shape[2:]
    t = window_partition_ref(x, window_size)
    if compute_dtype is not None:
        t = t.to(compute_dtype)
    depth = 1 + max(int(k.split(".")[1]) for k in params if k.startswith("blocks."))
    for i in range(depth):
        t = block_ref(t, _sub(params, f"blocks.{i}."), num_heads, state_dtype=state_dtype)
    return window_reverse_ref(t.to(x.dtype), window_size, H, W)
