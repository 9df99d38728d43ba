"""Plain-torch restatement of mamba_ssm.Mamba(d_model) with the package defaults (d_state 16, d_conv 4, expand 2,
dt_rank ceil(d_model / 16), conv bias, no linear biases): the yardstick of the SSM tests.  A sequential loop over time that
works in any dtype on any device; its float64 autograd gives the gradient references.  `params` is a dict with the
state-dict keys of the block (A_log, D, in_proj.weight, conv1d.weight, conv1d.bias, x_proj.weight, dt_proj.weight,
dt_proj.bias, out_proj.weight)."""
import torch
import torch.nn.functional as TF

N_STATE = 16


def conv_ref(xs, weight, bias):
    """silu(causal depthwise conv1d(xs, k = 4, left pad 3) + bias); xs (B, L, d), weight (d, 1, 4), bias (d,)"""
    L = xs.shape[1]
    xp = TF.pad(xs, (0, 0, 3, 0))
    acc = bias.to(xs.dtype).expand_as(xs)
    for j in range(4):
        acc = acc + xp[:, j:j + L, :] * weight[:, 0, j].to(xs.dtype)
    return TF.silu(acc)


def scan_ref(u, dt_raw, dt_bias, A_log, Bm, Cm, D, z, state_dtype=None):
    """u, dt_raw, z (B, L, d); Bm, Cm (B, L, 16); A_log (d, 16); D, dt_bias (d,).  The state is kept in state_dtype
    (default: the dtype of u) -> (B, L, d) in the dtype of u."""
    sd = state_dtype or u.dtype
    dt = TF.softplus(dt_raw.to(sd) + dt_bias.to(sd))
    A = -torch.exp(A_log.to(sd))
    Bsz, L, d = u.shape
    h = torch.zeros((Bsz, d, N_STATE), dtype=sd, device=u.device)
    ys = []
    for t in range(L):
        dtt, ut = dt[:, t, :, None], u[:, t, :, None].to(sd)
        h = torch.exp(dtt * A) * h + dtt * Bm[:, t, None, :].to(sd) * ut
        ys.append((h * Cm[:, t, None, :].to(sd)).sum(-1) + D.to(sd) * u[:, t].to(sd))
    y = torch.stack(ys, dim=1)
    zz = z.to(sd)
    return (y * zz * torch.sigmoid(zz)).to(u.dtype)


def mamba_ref(x, params, state_dtype=None):
    """x (B, L, H) -> (B, L, H)"""
    d = params["D"].shape[0]
    R = params["dt_proj.weight"].shape[1]
    dtp = x.dtype
    w = {k: v.to(dtp) for k, v in params.items() if k not in ("A_log", "D", "dt_proj.bias")}
    xz = x @ w["in_proj.weight"].T
    xs, z = xz[..., :d], xz[..., d:]
    u = conv_ref(xs, w["conv1d.weight"], w["conv1d.bias"])
    xdbl = u @ w["x_proj.weight"].T
    dt_r, Bm, Cm = xdbl[..., :R], xdbl[..., R:R + N_STATE], xdbl[..., R + N_STATE:]
    dt_raw = dt_r @ w["dt_proj.weight"].T
    y = scan_ref(u, dt_raw, params["dt_proj.bias"], params["A_log"], Bm, Cm, params["D"], z, state_dtype)
    return y @ w["out_proj.weight"].T


def fusion_ref(image_tokens, text_tokens, txt_w, txt_b, params, text_pool="cls", state_dtype=None):
    """reference SSMFusionModule.forward: Mamba(img + txt_proj(pool(txt))) averaged over the tokens -> (B, H)"""
    txt = text_tokens.mean(dim=1) if text_pool == "mean" else text_tokens[:, 0, :]
    tokens = image_tokens + (txt @ txt_w.T + txt_b).unsqueeze(1)
    return mamba_ref(tokens, params, state_dtype).mean(dim=1)
