"""Mamba block of the SSM fusion (reference modules/fusion_blocks.py:264-292 -> mamba_ssm.Mamba, d_state 16, d_conv 4) and of
the multimodal Mamba blocks (reference ConNexT/models/block/len4mamba.py:74-79,138-143, d_state 128); the scan takes d_state
in D_STATES.  The four projections run through hamspine.functional.linear; the causal depthwise conv1d + SiLU and the selective scan
are one C call per direction (hs_causal_conv1d_* / hs_selective_scan_*, csrc/ssm.hip).  Activations stay in the compute
dtype, the state and every sum are f32.  Column slices of the in_proj / x_proj outputs are read in place through their row
pitch; the two splits below hand autograd one gradient per GEMM output instead of zero-padded slices."""
import torch
from torch.autograd import Function

from . import _lib as L
from . import rt

D_STATE, D_CONV = 16, 4                 # the defaults of mamba_ssm.Mamba
D_STATES = (16, 32, 64, 128, 256)       # what hs_selective_scan_* takes


def _pitched(t):
    """(B, L, d) tensor whose rows are contiguous and evenly spaced -> (tensor, row pitch in elements)"""
    B, Lt, d = t.shape
    p = t.stride(1) if Lt > 1 else (t.stride(0) if B > 1 else d)
    ok = t.stride(2) == 1 and p >= d and (Lt == 1 or t.stride(1) == p) and (B == 1 or t.stride(0) == Lt * p)
    if not ok:
        t = t.contiguous()
        p = d
    return t, p


def _same(g, dtype):
    g = g.contiguous()
    return g if g.dtype == dtype else g.to(dtype)


class SplitViewFn(Function):
    """(..., a + b) -> views (..., a), (..., b) of one GEMM output; the backward joins the two gradients in one launch."""

    @staticmethod
    def forward(ctx, x, a):
        rt.need_gpu(x)
        ctx.meta = (a, x.shape[-1] - a)
        return x[..., :a], x[..., a:]

    @staticmethod
    def backward(ctx, ga, gb):
        a, b = ctx.meta
        dt = ga.dtype if ga is not None else gb.dtype
        lead = (ga if ga is not None else gb).shape[:-1]
        dev = (ga if ga is not None else gb).device
        ga = _same(ga, dt) if ga is not None else torch.zeros(lead + (a,), dtype=dt, device=dev)
        gb = _same(gb, dt) if gb is not None else torch.zeros(lead + (b,), dtype=dt, device=dev)
        g = torch.empty(lead + (a + b,), dtype=dt, device=dev)
        rows = g.numel() // (a + b)
        L.check(L.lib().hs_concat2_t(rt.hs_dtype(dt), rt.p(ga), a, rt.p(gb), b, rt.p(g), rows, rt.stream()), "hs_concat2_t")
        return g, None


class SplitCopyFn(Function):
    """(..., a + b) -> contiguous copies (..., a), (..., b) (a GEMM operand and the Bm | Cm pair of the x_proj output)."""

    @staticmethod
    def forward(ctx, x, a):
        rt.need_gpu(x)
        x = x.contiguous()
        b = x.shape[-1] - a
        lead = x.shape[:-1]
        xa = torch.empty(lead + (a,), dtype=x.dtype, device=x.device)
        xb = torch.empty(lead + (b,), dtype=x.dtype, device=x.device)
        rows = x.numel() // (a + b)
        L.check(L.lib().hs_split2_t(rt.hs_dtype(x), rt.p(x), rt.p(xa), a, rt.p(xb), b, rows, rt.stream()), "hs_split2_t")
        ctx.meta = (a, b)
        return xa, xb

    backward = staticmethod(SplitViewFn.backward)


class AddTokenBiasFn(Function):
    """tokens (B, L, H) in the compute dtype + feature (B, H) f32, broadcast over the tokens"""

    @staticmethod
    def forward(ctx, x, v):
        rt.need_gpu(x, v)
        x = x.contiguous()
        v = v.contiguous()
        if v.dtype != torch.float32:
            v = v.float()
        B, Lt, H = x.shape
        o = torch.empty_like(x)
        L.check(L.lib().hs_add_token_bias_fwd(rt.hs_dtype(x), rt.p(x), rt.p(v), rt.p(o), B, Lt, H, rt.stream()),
                "hs_add_token_bias_fwd")
        ctx.meta = x.dtype
        return o

    @staticmethod
    def backward(ctx, g):
        g = _same(g, ctx.meta)
        B, Lt, H = g.shape
        dv = None
        if ctx.needs_input_grad[1]:
            dv = torch.empty((B, H), dtype=torch.float32, device=g.device)
            L.check(L.lib().hs_add_token_bias_bwd(rt.hs_dtype(g), rt.p(g), rt.p(dv), B, Lt, H, rt.stream()),
                    "hs_add_token_bias_bwd")
        return (g if ctx.needs_input_grad[0] else None), dv


class CausalConv1dFn(Function):
    """silu(depthwise causal conv1d(x) + bias): x (B, L, d), possibly a column slice; weight (d, 1, 4), bias (d,) f32"""

    @staticmethod
    def forward(ctx, x, weight, bias):
        rt.need_gpu(x, weight, bias)
        x, ldx = _pitched(x)
        B, Lt, d = x.shape
        weight, bias = weight.contiguous(), bias.contiguous()
        y = torch.empty((B, Lt, d), dtype=x.dtype, device=x.device)
        L.check(L.lib().hs_causal_conv1d_fwd(rt.hs_dtype(x), rt.p(x), ldx, rt.p(weight), rt.p(bias), rt.p(y), d, B, Lt, d,
                                             weight.shape[-1], rt.stream()), "hs_causal_conv1d_fwd")
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x, weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        x, ldx = _pitched(x)
        B, Lt, d = x.shape
        dy = _same(dy, x.dtype)
        dx = torch.empty((B, Lt, d), dtype=x.dtype, device=x.device)
        dw = rt.grad_buffer_like(weight)
        db = rt.grad_buffer_like(bias)
        wsb = L.lib().hs_causal_conv1d_ws_bytes(B, d)
        ws = rt.workspace(wsb, x.device)
        L.check(L.lib().hs_causal_conv1d_bwd(rt.hs_dtype(x), rt.p(dy), d, rt.p(x), ldx, rt.p(weight), rt.p(bias), rt.p(dx), d,
                                             rt.p(dw), rt.p(db), rt.p(ws), ws.numel(), B, Lt, d, weight.shape[-1], rt.stream()),
                "hs_causal_conv1d_bwd")
        return dx, dw, db


class SelectiveScanFn(Function):
    """out = (scan(u, softplus(dt + dt_bias), -exp(A_log), Bm, Cm) + D u) * silu(z).
    u, dt, z: (B, L, d); bc: (B, L, 2N) = [Bm | Cm]; A_log (d, N), D, dt_bias (d,) f32, N = d_state.  u / dt / z / bc may be
    column slices.  Saved for the backward: the inputs and the state after every chunk, (B, (L-1)//chunk(N), d, N) f32."""

    @staticmethod
    def forward(ctx, u, dt, dt_bias, A_log, bc, D, z):
        rt.need_gpu(u, dt, dt_bias, A_log, bc, D, z)
        lib = L.lib()
        u, ldu = _pitched(u)
        dt, lddt = _pitched(dt)
        z, ldz = _pitched(z)
        bc, ldbc = _pitched(bc)
        B, Lt, d = u.shape
        N = A_log.shape[-1]
        if dt.shape != u.shape or z.shape != u.shape or bc.shape != (B, Lt, 2 * N) or not (u.dtype == dt.dtype == z.dtype == bc.dtype):
            raise L.HamspineError("selective_scan: u, dt, z (B, L, d) and bc (B, L, 2 * d_state) must agree in shape and dtype")
        dt_bias, A_log, D = dt_bias.contiguous(), A_log.contiguous(), D.contiguous()
        esz = u.element_size()
        out = torch.empty((B, Lt, d), dtype=u.dtype, device=u.device)
        need = any(ctx.needs_input_grad)
        hck = None
        chunk = lib.hs_selective_scan_chunk_len_n(N)
        if need and Lt > 0 and chunk > 0:      # an unsupported d_state is refused by the call below
            nck = (Lt - 1) // chunk
            hck = torch.empty((B, nck, d, N), dtype=torch.float32, device=u.device) if nck > 0 else None
        L.check(lib.hs_selective_scan_fwd(rt.hs_dtype(u), rt.p(u), ldu, rt.p(dt), lddt, rt.p(dt_bias), rt.p(A_log), rt.p(bc),
                                          rt.p(bc, N * esz), ldbc, rt.p(D), rt.p(z), ldz, rt.p(out), d, rt.p(hck), B, Lt, d, N,
                                          rt.stream()), "hs_selective_scan_fwd")
        if need:
            ctx.save_for_backward(u, dt, dt_bias, A_log, bc, D, z, hck)
        return out

    @staticmethod
    def backward(ctx, dout):
        u, dt, dt_bias, A_log, bc, D, z, hck = ctx.saved_tensors
        lib = L.lib()
        u, ldu = _pitched(u)
        dt, lddt = _pitched(dt)
        z, ldz = _pitched(z)
        bc, ldbc = _pitched(bc)
        B, Lt, d = u.shape
        N = A_log.shape[-1]
        T = u.dtype
        esz = u.element_size()
        dout = _same(dout, T)
        du = torch.empty((B, Lt, d), dtype=T, device=u.device)
        ddt = torch.empty_like(du)
        dz = torch.empty_like(du)
        dbc = torch.empty((B, Lt, 2 * N), dtype=T, device=u.device)
        dA = rt.grad_buffer_like(A_log)
        dD = rt.grad_buffer_like(D)
        dbias = rt.grad_buffer_like(dt_bias)
        wsb = lib.hs_selective_scan_ws_bytes_n(B, Lt, d, N)
        ws = rt.workspace(wsb, u.device)
        L.check(lib.hs_selective_scan_bwd(rt.hs_dtype(T), rt.p(dout), d, rt.p(u), ldu, rt.p(dt), lddt, rt.p(dt_bias), rt.p(A_log),
                                          rt.p(bc), rt.p(bc, N * esz), ldbc, rt.p(D), rt.p(z), ldz, rt.p(hck), rt.p(du), d,
                                          rt.p(ddt), d, rt.p(dbc), rt.p(dbc, N * esz), 2 * N, rt.p(dz), d, rt.p(dA), rt.p(dD),
                                          rt.p(dbias), rt.p(ws), ws.numel(), B, Lt, d, N, rt.stream()), "hs_selective_scan_bwd")
        return du, ddt, dbias, dA, dbc, dD, dz


class TransposeBatchedFn(Function):
    """(B, R, C) f32 -> (B, C, R) contiguous in one launch (the image feature (B, C, P) as (B, P, C) projection rows)"""

    @staticmethod
    def forward(ctx, x):
        rt.need_gpu(x)
        if x.dtype != torch.float32:
            raise L.HamspineError(f"transpose_batched expects an f32 tensor, got {x.dtype}")
        return TransposeBatchedFn._run(x.contiguous())

    @staticmethod
    def _run(x):
        B, R, Cc = x.shape
        o = torch.empty((B, Cc, R), dtype=torch.float32, device=x.device)
        L.check(L.lib().hs_transpose_batched_f32(rt.p(x), rt.p(o), B, R, Cc, rt.stream()), "hs_transpose_batched_f32")
        return o

    @staticmethod
    def backward(ctx, g):
        return TransposeBatchedFn._run(_same(g, torch.float32))


class TokenSeqAssembleFn(Function):
    """[text (B, H); img (B, P, H); first (B, H); last (B, H)] + pe[:P + 3] -> (B, P + 3, H), f32, one launch per direction"""

    @staticmethod
    def forward(ctx, text, img, first, last, pe):
        rt.need_gpu(text, img, first, last, pe)
        ts = [t.contiguous() for t in (text, img, first, last, pe)]
        if any(t.dtype != torch.float32 for t in ts):
            raise L.HamspineError("token_seq_assemble expects f32 tensors")
        text, img, first, last, pe = ts
        B, P, H = img.shape
        if text.shape != (B, H) or first.shape != (B, H) or last.shape != (B, H) or pe.shape[-1] != H or pe.numel() < (P + 3) * H:
            raise L.HamspineError("token_seq_assemble: text / first / last (B, H), img (B, P, H) and pe (>= P + 3, H) must agree")
        seq = torch.empty((B, P + 3, H), dtype=torch.float32, device=img.device)
        L.check(L.lib().hs_token_seq_assemble_fwd(rt.p(text), rt.p(img), rt.p(first), rt.p(last), rt.p(pe), rt.p(seq), B, P, H,
                                                  rt.stream()), "hs_token_seq_assemble_fwd")
        ctx.meta = (B, P, H)
        return seq

    @staticmethod
    def backward(ctx, g):
        B, P, H = ctx.meta
        g = _same(g, torch.float32)
        need = ctx.needs_input_grad
        outs = [torch.empty(shape, dtype=torch.float32, device=g.device) if n else None
                for n, shape in zip(need[:4], ((B, H), (B, P, H), (B, H), (B, H)))]
        if any(o is not None for o in outs):
            L.check(L.lib().hs_token_seq_assemble_bwd(rt.p(g), *[rt.p(o) for o in outs], B, P, H, rt.stream()),
                    "hs_token_seq_assemble_bwd")
        return (*outs, None)


def split_views(x, a):
    return SplitViewFn.apply(x, a)


def split_copy(x, a):
    return SplitCopyFn.apply(x, a)


def add_token_bias(x, v):
    return AddTokenBiasFn.apply(x, v)


def causal_conv1d(x, weight, bias):
    return CausalConv1dFn.apply(x, weight, bias)


def selective_scan(u, dt, dt_bias, A_log, bc, D, z):
    return SelectiveScanFn.apply(u, dt, dt_bias, A_log, bc, D, z)


def transpose_batched(x):
    return TransposeBatchedFn.apply(x)


def token_seq_assemble(text, img, first, last, pe):
    return TokenSeqAssembleFn.apply(text, img, first, last, pe)
