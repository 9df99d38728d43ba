"""Autograd nodes of the MambaVision mixer and stage (reference ConNexT/models/block/mamba_vision.py:1301-1330,1527-1636,
1809-1830): the centred depthwise conv1d + SiLU, the gate-less selective scan with 8 states and the window partition / reverse
(hs_conv1d_same_silu_*, hs_selective_scan_* with z = NULL, hs_window_*; csrc/ssm.hip).

The conv and the scan can write into a column slice of a wider buffer (`out=`): the mixer hands them the two halves of the
(B, L, d_inner) tensor out_proj reads, so the reference's torch.cat([y, z]) is no launch.  `join_halves` ties that buffer to
the two nodes for autograd and hands each its half of the gradient as a view; the backward kernels read it through its row
pitch."""
import torch
from torch.autograd import Function

from . import _lib as L
from . import rt
from .ssm import _pitched

D_STATE, D_CONV = 8, 3                  # what Block builds the mixer with (mamba_vision.py:1719-1723)


def _pitched_as(g, dtype):
    """gradient (B, L, d), possibly a column slice -> (tensor of `dtype`, row pitch)"""
    if g.dtype != dtype:
        g = g.to(dtype)
    return _pitched(g)


def _out_slice(out, like, who):
    """checks a caller-provided output slice: shape and dtype of `like`, rows evenly spaced; -> its row pitch"""
    if out.shape != like.shape or out.dtype != like.dtype or out.device != like.device:
        raise L.HamspineError(f"{who}: out must have the shape, dtype and device of the input")
    o, ld = _pitched(out)
    if o is not out:
        raise L.HamspineError(f"{who}: out must be a column slice of a contiguous (B, L, width) tensor")
    return ld


class Conv1dSameSiluFn(Function):
    """silu(depthwise conv1d(x, padding='same') [+ bias]): x (B, L, d), possibly a column slice; weight (d, 1, 3) f32, bias (d,)
    f32 or None; `out`: optional (B, L, d) column slice to write"""

    @staticmethod
    def forward(ctx, x, weight, bias, out):
        rt.need_gpu(x, weight, bias, out)
        x, ldx = _pitched(x)
        B, Lt, d = x.shape
        weight = weight.contiguous()
        bias = bias.contiguous() if bias is not None else None
        if out is None:
            y, ldy = torch.empty((B, Lt, d), dtype=x.dtype, device=x.device), d
        else:
            y, ldy = out, _out_slice(out, x, "conv1d_same_silu")
        L.check(L.lib().hs_conv1d_same_silu_fwd(rt.hs_dtype(x), rt.p(x), ldx, rt.p(weight), rt.p(bias), rt.p(y), ldy, B, Lt, d,
                                                weight.shape[-1], rt.stream()), "hs_conv1d_same_silu_fwd")
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x, weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        x, ldx = _pitched(x)
        B, Lt, d = x.shape
        dy, lddy = _pitched_as(dy, x.dtype)
        dx = torch.empty((B, Lt, d), dtype=x.dtype, device=x.device)
        dw = rt.grad_buffer_like(weight)
        db = rt.grad_buffer_like(bias) if bias is not None else None
        ws = rt.workspace(L.lib().hs_conv1d_same_silu_ws_bytes(B, d), x.device)
        L.check(L.lib().hs_conv1d_same_silu_bwd(rt.hs_dtype(x), rt.p(dy), lddy, rt.p(x), ldx, rt.p(weight), rt.p(bias), rt.p(dx), d,
                                                rt.p(dw), rt.p(db), rt.p(ws), ws.numel(), B, Lt, d, weight.shape[-1], rt.stream()),
                "hs_conv1d_same_silu_bwd")
        return dx, dw, db, None


class SelectiveScanNoGateFn(Function):
    """out = scan(u, softplus(dt + dt_bias), -exp(A_log), Bm, Cm) + D u, d_state 8 (the sibling of ssm.SelectiveScanFn without
    z).  u, dt: (B, L, d); bc: (B, L, 16) = [Bm | Cm]; A_log (d, 8), D, dt_bias (d,) f32; `out`: optional (B, L, d) column slice
    to write.  Saved for the backward: the inputs and the state after every chunk, (B, (L-1)//chunk, d, 8) f32."""

    @staticmethod
    def forward(ctx, u, dt, dt_bias, A_log, bc, D, out):
        rt.need_gpu(u, dt, dt_bias, A_log, bc, D, out)
        lib = L.lib()
        u, ldu = _pitched(u)
        dt, lddt = _pitched(dt)
        bc, ldbc = _pitched(bc)
        B, Lt, d = u.shape
        N = A_log.shape[-1]
        if dt.shape != u.shape or bc.shape != (B, Lt, 2 * N) or not (u.dtype == dt.dtype == bc.dtype):
            raise L.HamspineError("selective_scan: u, dt (B, L, d) and bc (B, L, 2 * d_state) must agree in shape and dtype")
        dt_bias, A_log, D = dt_bias.contiguous(), A_log.contiguous(), D.contiguous()
        esz = u.element_size()
        if out is None:
            y, ldo = torch.empty((B, Lt, d), dtype=u.dtype, device=u.device), d
        else:
            y, ldo = out, _out_slice(out, u, "selective_scan")
        need = any(ctx.needs_input_grad)
        hck = None
        chunk = lib.hs_selective_scan_chunk_len_nogate(N)
        if need and Lt > 0 and chunk > 0:      # an unsupported d_state is refused by the call below
            nck = (Lt - 1) // chunk
            hck = torch.empty((B, nck, d, N), dtype=torch.float32, device=u.device) if nck > 0 else None
        L.check(lib.hs_selective_scan_fwd(rt.hs_dtype(u), rt.p(u), ldu, rt.p(dt), lddt, rt.p(dt_bias), rt.p(A_log), rt.p(bc),
                                          rt.p(bc, N * esz), ldbc, rt.p(D), None, 0, rt.p(y), ldo, rt.p(hck), B, Lt, d, N,
                                          rt.stream()), "hs_selective_scan_fwd")
        if need:
            ctx.save_for_backward(u, dt, dt_bias, A_log, bc, D, hck)
        return y

    @staticmethod
    def backward(ctx, dout):
        u, dt, dt_bias, A_log, bc, D, hck = ctx.saved_tensors
        lib = L.lib()
        u, ldu = _pitched(u)
        dt, lddt = _pitched(dt)
        bc, ldbc = _pitched(bc)
        B, Lt, d = u.shape
        N = A_log.shape[-1]
        T = u.dtype
        esz = u.element_size()
        dout, lddo = _pitched_as(dout, T)
        du = torch.empty((B, Lt, d), dtype=T, device=u.device)
        ddt = torch.empty_like(du)
        dbc = torch.empty((B, Lt, 2 * N), dtype=T, device=u.device)
        dA = rt.grad_buffer_like(A_log)
        dD = rt.grad_buffer_like(D)
        dbias = rt.grad_buffer_like(dt_bias)
        ws = rt.workspace(lib.hs_selective_scan_ws_bytes_nogate(B, Lt, d, N), u.device)
        L.check(lib.hs_selective_scan_bwd(rt.hs_dtype(T), rt.p(dout), lddo, rt.p(u), ldu, rt.p(dt), lddt, rt.p(dt_bias),
                                          rt.p(A_log), rt.p(bc), rt.p(bc, N * esz), ldbc, rt.p(D), None, 0, rt.p(hck), rt.p(du), d,
                                          rt.p(ddt), d, rt.p(dbc), rt.p(dbc, N * esz), 2 * N, None, 0, rt.p(dA), rt.p(dD),
                                          rt.p(dbias), rt.p(ws), ws.numel(), B, Lt, d, N, rt.stream()), "hs_selective_scan_bwd")
        return du, ddt, dbias, dA, dbc, dD, None


class JoinHalvesFn(Function):
    """(a, b, buf) -> buf, where a and b are buf[..., :w] and buf[..., w:] already written by their nodes: torch.cat([a, b], -1)
    without a launch.  The backward hands each node its half of the gradient as a view."""

    @staticmethod
    def forward(ctx, a, b, buf):
        w, es = a.shape[-1], buf.element_size()
        ok = (buf.is_contiguous() and a.shape[:-1] == b.shape[:-1] == buf.shape[:-1] and w + b.shape[-1] == buf.shape[-1]
              and a.data_ptr() == buf.data_ptr() and b.data_ptr() == buf.data_ptr() + w * es
              and a.stride() == buf.stride() and b.stride() == buf.stride())
        if not ok:
            raise L.HamspineError("join_halves: a and b must be the two column slices of buf")
        ctx.meta = w
        return buf

    @staticmethod
    def backward(ctx, g):
        w = ctx.meta
        return g[..., :w], g[..., w:], None


class WindowPartitionFn(Function):
    """map (B, C, H, W) f32 -> tokens (B nWh nWw, ws ws, C) of `dtype`, zero-filled to the right and bottom up to a multiple
    of ws; the backward is the window reverse with the crop"""

    @staticmethod
    def forward(ctx, x, ws, dtype):
        rt.need_gpu(x)
        if x.dtype != torch.float32:
            raise L.HamspineError(f"window_partition expects an f32 map, got {x.dtype}")
        B, Cc, H, W = x.shape
        ctx.meta = (B, Cc, H, W, ws)
        return _partition(x.contiguous(), ws, dtype)

    @staticmethod
    def backward(ctx, g):
        B, Cc, H, W, ws = ctx.meta
        return _reverse(g.contiguous(), B, Cc, H, W, ws), None, None


class WindowReverseFn(Function):
    """tokens (B nWh nWw, ws ws, C) -> map (B, C, H, W) f32 without the padded positions; the backward is the window partition
    of the gradient (zeros for the padded tokens)"""

    @staticmethod
    def forward(ctx, tokens, ws, H, W):
        rt.need_gpu(tokens)
        nwin = -(-H // ws) * -(-W // ws)
        nWB, P, Cc = tokens.shape
        if P != ws * ws or nWB % nwin:
            raise L.HamspineError(f"window_reverse: {tuple(tokens.shape)} tokens do not tile a {H} x {W} map with window {ws}")
        ctx.meta = (ws, tokens.dtype)
        return _reverse(tokens.contiguous(), nWB // nwin, Cc, H, W, ws)

    @staticmethod
    def backward(ctx, g):
        ws, dtype = ctx.meta
        if g.dtype != torch.float32:
            g = g.float()
        return _partition(g.contiguous(), ws, dtype), None, None, None


def _partition(x, ws, dtype):
    B, Cc, H, W = x.shape
    tok = torch.empty((B * -(-H // ws) * -(-W // ws), ws * ws, Cc), dtype=dtype, device=x.device)
    L.check(L.lib().hs_window_partition(rt.hs_dtype(dtype), rt.p(x), rt.p(tok), B, Cc, H, W, ws, rt.stream()),
            "hs_window_partition")
    return tok


def _reverse(tok, B, Cc, H, W, ws):
    x = torch.empty((B, Cc, H, W), dtype=torch.float32, device=tok.device)
    L.check(L.lib().hs_window_reverse(rt.hs_dtype(tok), rt.p(tok), rt.p(x), B, Cc, H, W, ws, rt.stream()), "hs_window_reverse")
    return x


def conv1d_same_silu(x, weight, bias=None, out=None):
    return Conv1dSameSiluFn.apply(x, weight, bias, out)


def selective_scan_nogate(u, dt, dt_bias, A_log, bc, D, out=None):
    return SelectiveScanNoGateFn.apply(u, dt, dt_bias, A_log, bc, D, out)


def join_halves(a, b, buf):
    return JoinHalvesFn.apply(a, b, buf)


def window_partition(x, window_size, dtype=torch.float32):
    return WindowPartitionFn.apply(x, int(window_size), dtype)


def window_reverse(tokens, window_size, H, W):
    return WindowReverseFn.apply(tokens, int(window_size), int(H), int(W))
