"""Autograd nodes of the convolutional half of MambaVision (reference ConNexT/models/block/mamba_vision.py:1434-1524,1809-1830,
1922-1951): the 3x3 convolutions of PatchEmbed, ConvBlock and Downsample, BatchNorm with ConvBlock's two epilogues, the window
partition / reverse of an NHWC map and the image packing (hs_conv3x3_*, hs_bn_*, hs_window_*_nhwc, hs_*_image_nhwc;
csrc/mvconv.hip), with hs_gemm's weight-gradient layout, hs_colsum and hs_batchnorm_fwd/bwd for what they already do.

A "map" is a (B, C, H, W)-shaped tensor of the compute dtype whose memory is NHWC rows with the channel pitch Cp = ceil8(C); the
lanes C .. Cp-1 hold zeros.  With C a multiple of 8 that is an ordinary channels_last tensor, so hooks and callers see
(B, C, H, W).  Every node takes and returns maps; a tensor of another layout is copied into one.

Dispatch of the convolution: where hs_gemm's implicit-GEMM core accepts the shape (C and Kout multiples of 64: the B and L3
variants) it runs, as before; every other shape runs on the 3x3 body of csrc/mvconv.hip."""
import torch
from torch.autograd import Function

from . import _lib as L
from . import raw
from . import rt


def ceil8(c):
    return (c + 7) // 8 * 8


def _rows(x, dtype=None):
    """map or any (B, C, H, W) tensor -> contiguous (B, H, W, Cp) rows of `dtype` (default: x's) with zero pad lanes; no copy when
    x already is a map of that dtype"""
    B, C, H, W = x.shape
    Cp = ceil8(C)
    if dtype is not None and x.dtype != dtype:
        x = x.to(dtype)
    want = (H * W * Cp, 1, W * Cp, Cp)
    if all(n == 1 or s == w for n, s, w in zip(x.shape, x.stride(), want)) and x.storage_offset() % 8 == 0 \
            and x.untyped_storage().nbytes() >= (x.storage_offset() + B * H * W * Cp) * x.element_size():
        return torch.as_strided(x, (B, H, W, Cp), (H * W * Cp, W * Cp, Cp, 1))
    rows = torch.zeros((B, H, W, Cp), dtype=x.dtype, device=x.device) if Cp != C else \
        torch.empty((B, H, W, Cp), dtype=x.dtype, device=x.device)
    rows[..., :C].copy_(x.permute(0, 2, 3, 1))
    return rows


def _map(rows, C):
    """(B, H, W, Cp) rows -> the (B, C, H, W) map over them"""
    return rows[..., :C].permute(0, 3, 1, 2)


def _padded(v, Cp, fill=0.0):
    """f32 per-channel vector -> length Cp (the BatchNorm kernels run over the pitch; pad channels see x = 0)"""
    v = v.detach()
    if v.numel() == Cp:
        return v.contiguous()
    out = torch.full((Cp,), fill, dtype=torch.float32, device=v.device)
    out[:v.numel()] = v
    return out


def uses_gemm_core(C, Kout):
    """True where hs_gemm's convolution core takes a 3x3 convolution in both compute dtypes, forward and data gradient"""
    return C % 64 == 0 and Kout % 64 == 0


class Conv3x3Fn(Function):
    """y = conv2d(x, weight, bias, stride, padding=1) for a 3x3 weight (Kout, C, 3, 3) f32; x and y are maps"""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, force_new):
        rt.need_gpu(x, weight, bias)
        lib = L.lib()
        B, C, H, W = x.shape
        Kout = weight.shape[0]
        if tuple(weight.shape) != (Kout, C, 3, 3):
            raise L.HamspineError(f"conv3x3: weight {tuple(weight.shape)} does not fit an input of {C} channels")
        xr = _rows(x)
        T, Cp, Kp = xr.dtype, ceil8(C), ceil8(Kout)
        P, Q = (H - 1) // stride + 1, (W - 1) // stride + 1
        core = uses_gemm_core(C, Kout) and not force_new
        w32 = weight.detach().contiguous()
        wf = torch.empty((Kout, 9 * Cp), dtype=T, device=x.device)
        L.check(lib.hs_conv3x3_pack_filter(rt.hs_dtype(T), rt.p(w32), rt.p(wf), None, Kout, C, Cp, Kp, rt.stream()),
                "hs_conv3x3_pack_filter")
        b32 = bias.detach().contiguous() if bias is not None else None
        yr = torch.empty((B, P, Q, Kp), dtype=T, device=x.device)
        if core:
            raw.gemm(xr, wf, yr, B * P * Q, Kout, 9 * C, a_kind=L.A_CONV, b_kind=L.B_KC, ldb=9 * C, ldd=Kout,
                     geom=raw.conv_geom(B, H, W, C, Kout, 3, 3, stride, 1), bias=b32)
        else:
            L.check(lib.hs_conv3x3_fwd(rt.hs_dtype(T), rt.p(xr), rt.p(wf), rt.p(b32), rt.p(yr), B, H, W, C, Cp, Kout, Kp, stride,
                                       rt.stream()), "hs_conv3x3_fwd")
        ctx.meta = (stride, core, bias is not None)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xr, w32, wf)
        return _map(yr, Kout)

    @staticmethod
    def backward(ctx, dy):
        xr, w32, wf = ctx.saved_tensors
        stride, core, has_bias = ctx.meta
        lib = L.lib()
        B, H, W, Cp = xr.shape
        Kout, C = w32.shape[:2]
        T, Kp = xr.dtype, ceil8(Kout)
        P, Q = (H - 1) // stride + 1, (W - 1) // stride + 1
        M = B * P * Q
        dyr = _rows(dy, T)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dxr = torch.empty_like(xr)
            if core:
                raw.gemm(dyr, wf, dxr, B * H * W, C, 9 * Kout, a_kind=L.A_DGRAD, b_kind=L.B_WDGRAD, ldd=C,
                         geom=raw.conv_geom(B, H, W, C, Kout, 3, 3, stride, 1))
            else:
                wt = torch.empty((C, 9 * Kp), dtype=T, device=xr.device)
                L.check(lib.hs_conv3x3_pack_filter(rt.hs_dtype(T), rt.p(w32), rt.p(wf), rt.p(wt), Kout, C, Cp, Kp, rt.stream()),
                        "hs_conv3x3_pack_filter")
                L.check(lib.hs_conv3x3_dgrad(rt.hs_dtype(T), rt.p(dyr), rt.p(wt), rt.p(dxr), B, H, W, C, Cp, Kout, Kp, stride,
                                             rt.stream()), "hs_conv3x3_dgrad")
            dx = _map(dxr, C)
        if ctx.needs_input_grad[1]:
            # dW[ko][(r, s, c)] = sum over pixels of dy[pixel][ko] * patch(x)[pixel][(r, s, c)]: hs_gemm's weight-gradient layout
            # over the padded channel count, then back to the parameter's (Kout, C, 3, 3)
            g = torch.empty((Kout, 9 * Cp), dtype=torch.float32, device=xr.device)
            raw.gemm(dyr, xr, g, Kout, 9 * Cp, M, a_kind=L.A_RC, b_kind=L.B_CONV, lda=Kp, ldd=9 * Cp,
                     geom=raw.conv_geom(B, H, W, Cp, Kout, 3, 3, stride, 1),
                     split_k=max(1, raw.suggest_split(Kout, 9 * Cp, M, rt.hs_dtype(T))))
            dw = rt.grad_buffer_like(w32)
            if not dw.is_contiguous():
                dw = torch.empty_like(w32)
            L.check(lib.hs_conv3x3_unpack_wgrad(rt.p(g), rt.p(dw), Kout, C, Cp, rt.stream()), "hs_conv3x3_unpack_wgrad")
        if has_bias and ctx.needs_input_grad[2]:
            db = torch.empty((Kout,), dtype=torch.float32, device=xr.device)
            ws = rt.workspace(lib.hs_colsum_ws_bytes(M, Kout), xr.device)
            L.check(lib.hs_colsum(rt.hs_dtype(T), rt.p(dyr), M, Kout, Kp, rt.p(db), rt.p(ws), ws.numel(), 0, rt.stream()),
                    "hs_colsum")
        return dx, dw, db, None, None


def _bn_stats(xr, M, C, gamma, beta, running_mean, running_var, eps, momentum, training, relu=0, yr=None):
    """hs_batchnorm_fwd over the [M][Cp] rows: statistics (train: batch, with the running update; eval: running), scale / shift and,
    with yr, its own apply pass (plain or ReLU) -> (gamma, beta, mean, invstd, scale, shift) of length Cp"""
    lib = L.lib()
    Cp = xr.shape[-1]
    dev = xr.device
    g, b = _padded(gamma, Cp), _padded(beta, Cp)
    track = running_mean is not None and running_var is not None
    rm = _padded(running_mean, Cp) if track else None
    rv = _padded(running_var, Cp, 1.0) if track else None
    mean, invstd, scale, shift = (torch.empty(Cp, dtype=torch.float32, device=dev) for _ in range(4))
    ws = rt.workspace(lib.hs_batchnorm_ws_bytes(M, Cp, rt.hs_dtype(xr)), dev)
    p = L.BnParams()
    p.dtype, p.C, p.M, p.training, p.relu = rt.hs_dtype(xr), Cp, M, 1 if training else 0, relu
    p.eps, p.momentum = eps, momentum
    p.x, p.y, p.gamma, p.beta = rt.p(xr), rt.p(yr), rt.p(g), rt.p(b)
    p.running_mean, p.running_var = rt.p(rm), rt.p(rv)
    p.save_mean, p.save_invstd, p.scale, p.shift = rt.p(mean), rt.p(invstd), rt.p(scale), rt.p(shift)
    p.ws, p.ws_bytes = rt.p(ws), ws.numel()
    L.check(lib.hs_batchnorm_fwd(p, rt.stream()), "hs_batchnorm_fwd")
    if training and track and Cp != C:
        running_mean.copy_(rm[:C])
        running_var.copy_(rv[:C])
    return g, b, mean, invstd, scale, shift


def _use_batch(training, running_mean):
    return bool(training or running_mean is None)


class BatchNormFn(Function):
    """BatchNorm2d over a map, plain or with a fused ReLU (hs_batchnorm_fwd / hs_batchnorm_bwd: PatchEmbed's conv_down.1 / .4 and
    the model's final norm).  cfg: eps, momentum, training, relu, running_mean, running_var"""

    @staticmethod
    def forward(ctx, x, weight, bias, cfg):
        rt.need_gpu(x, weight, bias)
        B, C, H, W = x.shape
        xr = _rows(x)
        M = B * H * W
        yr = torch.empty_like(xr)
        batch = _use_batch(cfg["training"], cfg["running_mean"])
        g, b, mean, invstd, scale, shift = _bn_stats(xr, M, C, weight, bias, cfg["running_mean"], cfg["running_var"], cfg["eps"],
                                                     cfg["momentum"], batch, 1 if cfg["relu"] else 0, yr)
        ctx.meta = (C, batch, bool(cfg["relu"]))
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xr, g, mean, invstd, scale, shift)
        return _map(yr, C)

    @staticmethod
    def backward(ctx, dy):
        xr, g, mean, invstd, scale, shift = ctx.saved_tensors
        C, batch, relu = ctx.meta
        lib = L.lib()
        Cp = xr.shape[-1]
        M = xr.numel() // Cp
        dyr = _rows(dy, xr.dtype)
        dxr = torch.empty_like(xr)
        dgamma, dbeta = (torch.empty(Cp, dtype=torch.float32, device=xr.device) for _ in range(2))
        ws = rt.workspace(lib.hs_batchnorm_ws_bytes(M, Cp, rt.hs_dtype(xr)), xr.device)
        p = L.BnBwdParams()
        p.dtype, p.C, p.M, p.training, p.relu = rt.hs_dtype(xr), Cp, M, 1 if batch else 0, 1 if relu else 0
        p.dy, p.x, p.gamma, p.save_mean, p.save_invstd = rt.p(dyr), rt.p(xr), rt.p(g), rt.p(mean), rt.p(invstd)
        p.dx, p.dgamma, p.dbeta = rt.p(dxr), rt.p(dgamma), rt.p(dbeta)
        p.ws, p.ws_bytes = rt.p(ws), ws.numel()
        if relu:
            p.scale, p.shift = rt.p(scale), rt.p(shift)
        L.check(lib.hs_batchnorm_bwd(p, rt.stream()), "hs_batchnorm_bwd")
        return _map(dxr, C), dgamma[:C], dbeta[:C], None


class BatchNormEpilogueFn(Function):
    """ConvBlock's two BatchNorms over a map.  mode 0: gelu_tanh(bn(x)) (norm1 + act1).  mode 1: res + ls_gamma * rowscale[sample]
    * bn(x) (norm2, layer scale, stochastic depth, residual); ls_gamma and rowscale may be None.  The statistics come from
    hs_batchnorm_fwd without an output, the apply passes and the whole backward from csrc/mvconv.hip."""

    @staticmethod
    def forward(ctx, x, weight, bias, res, ls_gamma, rowscale, mode, cfg):
        rt.need_gpu(x, weight, bias, res, ls_gamma, rowscale)
        lib = L.lib()
        B, C, H, W = x.shape
        xr = _rows(x)
        Cp = xr.shape[-1]
        M = B * H * W
        batch = _use_batch(cfg["training"], cfg["running_mean"])
        g, b, mean, invstd, scale, shift = _bn_stats(xr, M, C, weight, bias, cfg["running_mean"], cfg["running_var"], cfg["eps"],
                                                     cfg["momentum"], batch)
        yr = torch.empty_like(xr)
        ls = ls_gamma.detach().contiguous() if ls_gamma is not None else None
        rs = rowscale.detach().to(torch.float32).contiguous() if rowscale is not None else None
        if mode == 0:
            L.check(lib.hs_bn_gelu_tanh_fwd(rt.hs_dtype(xr), rt.p(xr), rt.p(scale), rt.p(shift), rt.p(yr), M, C, Cp, rt.stream()),
                    "hs_bn_gelu_tanh_fwd")
        else:
            if rs is not None and rs.numel() != B:
                raise L.HamspineError(f"bn_scale_residual: rowscale has {rs.numel()} entries for {B} samples")
            rr = _rows(res, xr.dtype)
            L.check(lib.hs_bn_scale_residual_fwd(rt.hs_dtype(xr), rt.p(xr), rt.p(scale), rt.p(shift), rt.p(rr), rt.p(ls), rt.p(rs),
                                                 rt.p(yr), M, C, Cp, H * W, rt.stream()), "hs_bn_scale_residual_fwd")
        ctx.meta = (C, batch, mode, H * W)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xr, g, b, mean, invstd, scale, shift, ls, rs)
        return _map(yr, C)

    @staticmethod
    def backward(ctx, dy):
        xr, g, b, mean, invstd, scale, shift, ls, rs = ctx.saved_tensors
        C, batch, mode, hw = ctx.meta
        lib = L.lib()
        Cp = xr.shape[-1]
        M = xr.numel() // Cp
        dyr = _rows(dy, xr.dtype)
        dxr = torch.empty_like(xr)
        dgamma, dbeta = (torch.empty(C, dtype=torch.float32, device=xr.device) for _ in range(2))
        dls = torch.empty(C, dtype=torch.float32, device=xr.device) if ls is not None else None
        ws = rt.workspace(lib.hs_bn_epilogue_ws_bytes(M, C), xr.device)
        L.check(lib.hs_bn_epilogue_bwd(rt.hs_dtype(xr), mode, rt.p(dyr), rt.p(xr), rt.p(scale), rt.p(shift), rt.p(mean), rt.p(invstd),
                                       rt.p(g), rt.p(b), rt.p(ls), rt.p(rs), rt.p(dxr), rt.p(dgamma), rt.p(dbeta), rt.p(dls),
                                       1 if batch else 0, M, C, Cp, hw, rt.p(ws), ws.numel(), rt.stream()), "hs_bn_epilogue_bwd")
        dres = _map(dyr, C) if mode == 1 and ctx.needs_input_grad[3] else None
        return _map(dxr, C), dgamma, dbeta, dres, dls, None, None, None


class PackImageFn(Function):
    """image (B, Cin, H, W) f32 -> map of `dtype` (Cin = 3: 8 stored channels); the backward unpacks the gradient to f32 NCHW"""

    @staticmethod
    def forward(ctx, x, dtype):
        rt.need_gpu(x)
        x = x.contiguous()
        if x.dtype != torch.float32:
            x = x.float()
        B, C, H, W = x.shape
        Cp = ceil8(C)
        rows = torch.empty((B, H, W, Cp), dtype=dtype, device=x.device)
        L.check(L.lib().hs_pack_image_nhwc(rt.hs_dtype(dtype), rt.p(x), rt.p(rows), B, C, H, W, Cp, rt.stream()), "hs_pack_image_nhwc")
        ctx.meta = (C, dtype)
        return _map(rows, C)

    @staticmethod
    def backward(ctx, g):
        C, dtype = ctx.meta
        gr = _rows(g, dtype)
        B, H, W, Cp = gr.shape
        dx = torch.empty((B, C, H, W), dtype=torch.float32, device=g.device)
        L.check(L.lib().hs_unpack_image_nhwc(rt.hs_dtype(dtype), rt.p(gr), rt.p(dx), B, C, H, W, Cp, rt.stream()),
                "hs_unpack_image_nhwc")
        return dx, None


def _partition_nhwc(rows, C, ws):
    B, H, W, Cp = rows.shape
    tok = torch.empty((B * -(-H // ws) * -(-W // ws), ws * ws, C), dtype=rows.dtype, device=rows.device)
    L.check(L.lib().hs_window_partition_nhwc(rt.hs_dtype(rows), rt.p(rows), rt.p(tok), B, C, Cp, H, W, ws, rt.stream()),
            "hs_window_partition_nhwc")
    return tok


def _reverse_nhwc(tok, B, H, W, ws):
    C = tok.shape[-1]
    rows = torch.empty((B, H, W, ceil8(C)), dtype=tok.dtype, device=tok.device)
    L.check(L.lib().hs_window_reverse_nhwc(rt.hs_dtype(tok), rt.p(tok), rt.p(rows), B, C, rows.shape[-1], H, W, ws, rt.stream()),
            "hs_window_reverse_nhwc")
    return rows


def _one_window(C, H, W, ws):
    """one window covers the whole map, nothing is padded and the rows have no pad lanes: tokens and map are the same memory"""
    return H == ws and W == ws and C % 8 == 0


class WindowPartitionNhwcFn(Function):
    """map -> tokens (B nWh nWw, ws ws, C) of the same dtype, zero-filled right and below up to a multiple of ws"""

    @staticmethod
    def forward(ctx, x, ws):
        rt.need_gpu(x)
        B, C, H, W = x.shape
        ctx.meta = (B, C, H, W, ws, x.dtype)
        return _partition_nhwc(_rows(x), C, ws)

    @staticmethod
    def backward(ctx, g):
        B, C, H, W, ws, dtype = ctx.meta
        if g.dtype != dtype:
            g = g.to(dtype)
        return _map(_reverse_nhwc(g.contiguous(), B, H, W, ws), C), None


class WindowReverseNhwcFn(Function):
    """tokens (B nWh nWw, ws ws, C) -> map (B, C, H, W) of the same dtype without the padded positions"""

    @staticmethod
    def forward(ctx, tokens, ws, H, W):
        rt.need_gpu(tokens)
        nwin = -(-H // ws) * -(-W // ws)
        nWB, P, C = tokens.shape
        if P != ws * ws or nWB % nwin:
            raise L.HamspineError(f"window_reverse_nhwc: {tuple(tokens.shape)} tokens do not tile a {H} x {W} map with window {ws}")
        ctx.meta = (C, ws, tokens.dtype)
        return _map(_reverse_nhwc(tokens.contiguous(), nWB // nwin, H, W, ws), C)

    @staticmethod
    def backward(ctx, g):
        C, ws, dtype = ctx.meta
        return _partition_nhwc(_rows(g, dtype), C, ws), None, None, None


def conv3x3(x, weight, bias=None, stride=1, force_new_body=False):
    return Conv3x3Fn.apply(x, weight, bias, int(stride), bool(force_new_body))


def _cfg(bn, training, relu=False):
    return {"eps": float(bn.eps), "momentum": float(bn.momentum if bn.momentum is not None else 0.1), "training": bool(training),
            "relu": relu, "running_mean": bn.running_mean, "running_var": bn.running_var}


def batch_norm(x, bn, training, relu=False):
    """bn: a BatchNorm2d parameter holder (weight, bias, running statistics, eps, momentum)"""
    return BatchNormFn.apply(x, bn.weight, bn.bias, _cfg(bn, training, relu))


def batch_norm_gelu_tanh(x, bn, training):
    return BatchNormEpilogueFn.apply(x, bn.weight, bn.bias, None, None, None, 0, _cfg(bn, training))


def batch_norm_scale_residual(x, bn, training, res, ls_gamma=None, rowscale=None):
    return BatchNormEpilogueFn.apply(x, bn.weight, bn.bias, res, ls_gamma, rowscale, 1, _cfg(bn, training))


def pack_image(x, dtype):
    return PackImageFn.apply(x, dtype)


def window_partition_nhwc(x, window_size):
    """map -> tokens; a view where one window covers the whole map"""
    B, C, H, W = x.shape
    ws = int(window_size)
    if _one_window(C, H, W, ws):
        return x.permute(0, 2, 3, 1).reshape(B, H * W, C)
    return WindowPartitionNhwcFn.apply(x, ws)


def window_reverse_nhwc(tokens, window_size, H, W):
    """tokens -> map; a view where one window covers the whole map"""
    ws = int(window_size)
    if _one_window(tokens.shape[-1], H, W, ws):
        return tokens.reshape(tokens.shape[0], H, W, tokens.shape[-1]).permute(0, 3, 1, 2)
    return WindowReverseNhwcFn.apply(tokens, ws, int(H), int(W))
