"""Plain-torch restatement of mamba_ssm.Mamba(d_model, d_state=N, d_conv=4, expand=2) for any d_state, and of the two
multimodal blocks of the reference's ConNexT/models/block/len4mamba.py composed from it: the yardstick of the general-d_state
Mamba tests.  A sequential loop over time that works in any dtype on the CPU; its float64 autograd gives the gradient
references.  d_state is read from A_log.  `params` is a dict with the state-dict keys of the module under test; the KAN
projections of the attention are oracle.models.OKAN1 called functionally on those entries."""
import torch
import torch.nn.functional as TF
from torch.func import functional_call

from oracle.models import OKAN1


def conv_ref(xs, weight, bias):
    """silu(causal depthwise conv1d(xs, k = 4, left pad 3) + bias); xs (B, L, d), weight (d, 1, 4), bias (d,)"""
    L = xs.shape[1]
    xp = TF.pad(xs, (0, 0, 3, 0))
    acc = bias.to(xs.dtype).expand_as(xs)
    for j in range(4):
        acc = acc + xp[:, j:j + L, :] * weight[:, 0, j].to(xs.dtype)
    return TF.silu(acc)


def scan_ref(u, dt_raw, dt_bias, A_log, Bm, Cm, D, z, state_dtype=None):
    """u, dt_raw, z (B, L, d); Bm, Cm (B, L, N); A_log (d, N); D, dt_bias (d,).  The state and every sum are kept in
    state_dtype (default: the dtype of u) -> (B, L, d) in the dtype of u."""
    sd = state_dtype or u.dtype
    N = A_log.shape[-1]
    dt = TF.softplus(dt_raw.to(sd) + dt_bias.to(sd))
    A = -torch.exp(A_log.to(sd))
    Bsz, L, d = u.shape
    h = torch.zeros((Bsz, d, N), dtype=sd, device=u.device)
    ys = []
    for t in range(L):
        dtt, ut = dt[:, t, :, None], u[:, t, :, None].to(sd)
        h = torch.exp(dtt * A) * h + dtt * Bm[:, t, None, :].to(sd) * ut
        ys.append((h * Cm[:, t, None, :].to(sd)).sum(-1) + D.to(sd) * u[:, t].to(sd))
    y = torch.stack(ys, dim=1)
    zz = z.to(sd)
    return (y * zz * torch.sigmoid(zz)).to(u.dtype)


def mamba_ref(x, params, state_dtype=None):
    """x (B, L, H) -> (B, L, H) in the dtype of x; A_log, D and dt_proj.bias are used as given (f32 or f64)"""
    d, N = params["A_log"].shape
    R = params["dt_proj.weight"].shape[1]
    dtp = x.dtype
    w = {k: v.to(dtp) for k, v in params.items() if k not in ("A_log", "D", "dt_proj.bias")}
    xz = x @ w["in_proj.weight"].T
    xs, z = xz[..., :d], xz[..., d:]
    u = conv_ref(xs, w["conv1d.weight"], w["conv1d.bias"])
    xdbl = u @ w["x_proj.weight"].T
    dt_r, Bm, Cm = xdbl[..., :R], xdbl[..., R:R + N], xdbl[..., R + N:]
    dt_raw = dt_r @ w["dt_proj.weight"].T
    y = scan_ref(u, dt_raw, params["dt_proj.bias"], params["A_log"], Bm, Cm, params["D"], z, state_dtype)
    return y @ w["out_proj.weight"].T


def sinusoid_table(max_len, d_model):
    """(1, max_len, d_model) float64: sin(t / 10000^(2i / d_model)) in column 2i, the cosine in column 2i + 1, row t.  An
    independent evaluation of the table the blocks build in f32 (len4mamba.py:117-123); the block references below take the
    module's own table as data."""
    t = torch.arange(max_len, dtype=torch.float64)[:, None]
    angle = t / torch.pow(torch.tensor(10000.0, dtype=torch.float64), torch.arange(0, d_model, 2, dtype=torch.float64) / d_model)
    return torch.stack([torch.sin(angle), torch.cos(angle)], dim=-1).reshape(1, max_len, d_model)


def _sub(params, prefix):
    return {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix)}


def _lin(x, params, name):
    return x @ params[name + ".weight"].T + params[name + ".bias"]


def sequence_ref(text, img, first, last, params, pe):
    """len4mamba.py:86-106: the four projections, the concatenation and the positional encoding `pe` (1, max_len, D), the
    module's attribute -> (B, P + 3, D)"""
    seq = torch.cat([_lin(text, params, "proj_text").unsqueeze(1), _lin(img.permute(0, 2, 1), params, "proj_img"),
                     _lin(first, params, "proj_first").unsqueeze(1), _lin(last, params, "proj_last").unsqueeze(1)], dim=1)
    return seq + pe[:, :seq.shape[1], :].to(seq.dtype)


def kan_attention_ref(x, params, num_heads):
    """len4mamba.py:37-62 with p = 0 dropout; params holds {q,k,v}_proj.layers.0.* and out_proj.*"""
    B, L, D = x.shape
    hd = D // num_heads
    kan = OKAN1([D, D]).to(x.dtype)
    q, k, v = (functional_call(kan, _sub(params, n + "_proj."), (x,)).view(B, L, num_heads, hd).transpose(1, 2)
               for n in ("q", "k", "v"))
    att = torch.softmax((q @ k.transpose(-2, -1)) / (hd ** 0.5), dim=-1)
    out = (att @ v).transpose(1, 2).contiguous().view(B, L, D)
    return _lin(out, params, "out_proj")


def _mamba_in(x, params, mamba_dtype, state_dtype):
    """the Mamba block in mamba_dtype (None: the dtype of x) with the state in state_dtype, result back in the dtype of x"""
    mp = _sub(params, "mamba.")
    if mamba_dtype is None or mamba_dtype == x.dtype:
        return mamba_ref(x, mp, state_dtype)
    return mamba_ref(x.to(mamba_dtype), mp, state_dtype).to(x.dtype)


def multimodal_mamba_ref(text, img, first, last, params, pe, mamba_dtype=None, state_dtype=None):
    """len4mamba.py:147-176"""
    seq = sequence_ref(text, img, first, last, params, pe)
    return _mamba_in(seq, params, mamba_dtype, state_dtype) + seq


def multimodal_mamba_kan_attention_ref(text, img, first, last, params, pe, num_heads, mamba_dtype=None, state_dtype=None):
    """len4mamba.py:86-116"""
    seq = sequence_ref(text, img, first, last, params, pe)
    D = seq.shape[-1]
    a = kan_attention_ref(seq, _sub(params, "attn."), num_heads) + seq
    a = TF.layer_norm(a, (D,), params["norm1.weight"], params["norm1.bias"])
    m = _mamba_in(a, params, mamba_dtype, state_dtype) + a
    return TF.layer_norm(m, (D,), params["norm2.weight"], params["norm2.bias"])
