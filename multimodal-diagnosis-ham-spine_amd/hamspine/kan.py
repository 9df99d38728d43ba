"""KAN layer, mixture-of-experts gating and SupCon loss on the HIP kernels (csrc/kan_moe.hip + hs_gemm, f32; SupCon beyond 256
rows and over the gathered batch of a process group: csrc/supcon.hip).

reference: ConNexT/models/block/kan1.py:77-165 (KANLinear.forward / b_splines), moe.py:171-291 (MoE),
scripts/train.py:23-44 (SupConLoss); kan1.py:167-214 / :112-142 (update_grid / curve2coeff, csrc/kan_grid.hip).
"""
import ctypes as C

import torch
from torch.autograd import Function

from . import _lib as L
from . import raw, rt


def _f32c(t):
    rt.need_gpu(t)
    if t.dtype != torch.float32:
        raise L.HamspineError(f"expected f32, got {t.dtype}")
    return t.contiguous()


BASE_ACTS = {"silu": 0, "swish": 0, "gelu": 1, "relu": 2, "identity": 3}   # hs_kan_features_* base_act codes


class KANLinearFn(Function):
    @staticmethod
    def forward(ctx, x, grid, base_w, spline_w, scaler, grid_size, order, act=0):
        x, base_w, spline_w = _f32c(x), _f32c(base_w), _f32c(spline_w)
        grid = _f32c(grid)
        scaler = _f32c(scaler) if scaler is not None else None
        B, in_f = x.shape
        out_f = base_w.shape[0]
        nb = grid_size + order
        Kc = in_f * (1 + nb)
        dev = x.device
        lib = L.lib()
        feat = torch.empty((B, Kc), dtype=torch.float32, device=dev)
        wcat = torch.empty((out_f, Kc), dtype=torch.float32, device=dev)
        L.check(lib.hs_kan_features_fwd(rt.p(x), rt.p(grid), rt.p(feat), B, in_f, grid_size, order, act, rt.stream()),
                "kan_features")
        L.check(lib.hs_kan_pack_weight(rt.p(base_w), rt.p(spline_w), rt.p(scaler), rt.p(wcat), out_f, in_f, nb, rt.stream()),
                "kan_pack_weight")
        y = torch.empty((B, out_f), dtype=torch.float32, device=dev)
        raw.gemm(feat, wcat, y, B, out_f, Kc, lda=Kc, ldb=Kc)
        ctx.save_for_backward(x, grid, spline_w, scaler, feat, wcat)
        ctx.meta = (grid_size, order, base_w.shape, act)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, grid, spline_w, scaler, feat, wcat = ctx.saved_tensors
        grid_size, order, base_shape, act = ctx.meta
        dy = _f32c(dy)
        B, in_f = x.shape
        out_f = base_shape[0]
        nb = grid_size + order
        Kc = in_f * (1 + nb)
        dev = x.device
        lib = L.lib()
        need_w = any(ctx.needs_input_grad[2:5])
        d_base = d_spline = d_scaler = None
        if need_w:
            dwcat = torch.empty((out_f, Kc), dtype=torch.float32, device=dev)
            split = raw.suggest_split(out_f, Kc, B, L.HS_F32)
            raw.gemm(dy, feat, dwcat, out_f, Kc, B, a_kind=L.A_RC, b_kind=L.B_RC, lda=out_f, ldb=Kc, split_k=split)
            d_base = torch.empty(base_shape, dtype=torch.float32, device=dev)
            d_spline = torch.empty_like(spline_w)
            d_scaler = torch.empty_like(scaler) if scaler is not None else None
            L.check(lib.hs_kan_unpack_wgrad(rt.p(dwcat), rt.p(spline_w), rt.p(scaler), rt.p(d_base), rt.p(d_spline),
                                            rt.p(d_scaler), out_f, in_f, nb, rt.stream()), "kan_unpack_wgrad")
        dx = None
        if ctx.needs_input_grad[0]:
            dfeat = torch.empty((B, Kc), dtype=torch.float32, device=dev)
            raw.gemm(dy, wcat, dfeat, B, Kc, out_f, a_kind=L.A_KC, b_kind=L.B_RC, lda=out_f, ldb=Kc)
            dx = torch.empty_like(x)
            L.check(lib.hs_kan_features_bwd(rt.p(x), rt.p(grid), rt.p(dfeat), rt.p(dx), B, in_f, grid_size, order, act,
                                            rt.stream()), "kan_features_bwd")
        return dx, None, d_base, d_spline, d_scaler, None, None, None


def kan_linear(x, grid, base_weight, spline_weight, spline_scaler, grid_size, spline_order, base_act="silu"):
    return KANLinearFn.apply(x, grid, base_weight, spline_weight, spline_scaler, int(grid_size), int(spline_order),
                             BASE_ACTS[base_act])


def _refit(x, grid_new, grid_old, y, spline_weight, spline_scaler, out, grid_size, order):
    lib = L.lib()
    B, in_f = x.shape
    out_f = out.shape[0]
    nbytes = lib.hs_kan_refit_ws_bytes(B, in_f, out_f, grid_size, order, 1 if y is not None else 0)
    if nbytes < 0:
        raise L.HamspineError(f"kan refit: unsupported shape B={B} in={in_f} out={out_f} grid_size={grid_size} order={order}")
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=x.device)
    L.check(lib.hs_kan_refit(rt.p(x), rt.p(grid_new), rt.p(grid_old), rt.p(y), rt.p(spline_weight), rt.p(spline_scaler), rt.p(out),
                             B, in_f, out_f, grid_size, order, rt.p(ws), nbytes, rt.stream()), "hs_kan_refit")


def _param_f32(t, what):
    """a parameter or buffer the kernels write in place: it has to be the f32 contiguous storage itself, never a copy"""
    rt.need_gpu(t)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise L.HamspineError(f"{what}: expected a contiguous f32 tensor, got {t.dtype}, strides {t.stride()}")
    return t


@torch.no_grad()
def kan_update_grid(x, grid, spline_weight, spline_scaler, grid_size, spline_order, grid_eps=0.02, margin=0.01):
    """KANLinear.update_grid (reference kan1.py:167-214) on the device: `grid` (in, knots) moves to the per-feature quantiles of
    x (B, in) blended with a uniform grid, and `spline_weight` (out, in, coeffs) is re-fitted so that the spline part keeps its
    outputs on x.  Both are written in place on the current stream; nothing comes back to the host.  spline_scaler (out, in) or
    None.  A rank-deficient feature gets the least-norm least-squares solution (see hs_kan_refit)."""
    x = _f32c(x.detach())
    grid, spline_weight = _param_f32(grid, "grid"), _param_f32(spline_weight, "spline_weight")
    spline_scaler = _f32c(spline_scaler.detach()) if spline_scaler is not None else None
    grid_size, order = int(grid_size), int(spline_order)
    B, in_f = x.shape
    if B < 1:
        raise L.HamspineError("kan_update_grid: an empty batch has no quantiles")
    lib = L.lib()
    ranks = torch.linspace(0, B - 1, grid_size + 1, dtype=torch.int64)       # host: the reference's own index arithmetic
    new_grid = torch.empty_like(grid)
    L.check(lib.hs_kan_grid_knots(rt.p(x), ranks.data_ptr(), rt.p(new_grid), B, in_f, grid_size, order, grid_eps, 1 - grid_eps,
                                  margin, None, 0, rt.stream()), "hs_kan_grid_knots")
    _refit(x, new_grid, grid, None, spline_weight, spline_scaler, spline_weight, grid_size, order)
    grid.copy_(new_grid)


@torch.no_grad()
def kan_curve2coeff(x, y, grid, grid_size, spline_order):
    """KANLinear.curve2coeff (reference kan1.py:112-142) on the device: the coefficients (out, in, coeffs) whose splines on the
    knots `grid` (in, knots) fit y (B, in, out) at x (B, in) in the least-squares sense, per input feature."""
    x, y, grid = _f32c(x.detach()), _f32c(y.detach()), _f32c(grid.detach())
    grid_size, order = int(grid_size), int(spline_order)
    B, in_f = x.shape
    if y.dim() != 3 or y.shape[0] != B or y.shape[1] != in_f:
        raise L.HamspineError(f"kan_curve2coeff: y {tuple(y.shape)} is not (batch, in, out) = ({B}, {in_f}, out)")
    out = torch.empty((y.shape[2], in_f, grid_size + order), dtype=torch.float32, device=x.device)
    _refit(x, grid, None, y, None, None, out, grid_size, order)
    return out


class MoEGateFn(Function):
    """x -> (gates (B,E), aux loss) with w_gate / w_noise; noisy top-k in training, plain top-k in eval.  `noise`: optional
    (B,E) standard-normal draw (the reference's torch.randn_like(clean_logits), moe.py:247); None draws from the counter RNG."""

    @staticmethod
    def forward(ctx, x, w_gate, w_noise, k, noisy, coef, noise=None):
        x, w_gate, w_noise = _f32c(x), _f32c(w_gate), _f32c(w_noise)
        if noise is not None:
            noise = _f32c(noise)
            if tuple(noise.shape) != (x.shape[0], w_gate.shape[1]):
                raise ValueError(f"MoE gating noise must be (batch, experts) = {(x.shape[0], w_gate.shape[1])}, got {tuple(noise.shape)}")
        B, in_f = x.shape
        E = w_gate.shape[1]
        dev = x.device
        lib = L.lib()
        clean = torch.empty((B, E), dtype=torch.float32, device=dev)
        raw.gemm(x, w_gate, clean, B, E, in_f, a_kind=L.A_KC, b_kind=L.B_RC, lda=in_f, ldb=E)
        rawn = None
        if noisy:
            rawn = torch.empty((B, E), dtype=torch.float32, device=dev)
            raw.gemm(x, w_noise, rawn, B, E, in_f, a_kind=L.A_KC, b_kind=L.B_RC, lda=in_f, ldb=E)
        gates = torch.empty((B, E), dtype=torch.float32, device=dev)
        p = torch.empty_like(gates)
        z = torch.empty_like(gates)
        sigma = torch.empty_like(gates)
        loadrow = torch.empty_like(gates)
        top = torch.empty((B, 17), dtype=torch.int32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        d_imp = torch.empty(E, dtype=torch.float32, device=dev)
        d_load = torch.empty(E, dtype=torch.float32, device=dev)
        seed = rt.next_seed() if noisy else 0
        L.check(lib.hs_moe_gate_fwd(rt.p(clean), rt.p(rawn), rt.p(noise) if noisy else None, B, E, k, 1 if noisy else 0, 1e-2, seed, coef, rt.p(gates), rt.p(p),
                                    rt.p(top), rt.p(z), rt.p(sigma), rt.p(loadrow), rt.p(loss), rt.p(d_imp), rt.p(d_load),
                                    rt.stream()), "hs_moe_gate_fwd")
        ctx.save_for_backward(x, w_gate, w_noise, clean, rawn, p, top, z, sigma, d_imp, d_load)
        ctx.meta = (k, noisy)
        return gates, loss

    @staticmethod
    def backward(ctx, dgates, dloss):
        x, w_gate, w_noise, clean, rawn, p, top, z, sigma, d_imp, d_load = ctx.saved_tensors
        k, noisy = ctx.meta
        B, in_f = x.shape
        E = w_gate.shape[1]
        dev = x.device
        lib = L.lib()
        dgates = _f32c(dgates) if dgates is not None else torch.zeros((B, E), dtype=torch.float32, device=dev)
        gl = dloss.contiguous().float() if dloss is not None else None
        d_clean = torch.empty((B, E), dtype=torch.float32, device=dev)
        d_raw = torch.empty((B, E), dtype=torch.float32, device=dev) if noisy else None
        L.check(lib.hs_moe_gate_bwd(rt.p(clean), rt.p(rawn), rt.p(p), rt.p(top), rt.p(z), rt.p(sigma), rt.p(dgates), rt.p(gl),
                                    rt.p(d_imp), rt.p(d_load), B, E, k, 1 if noisy else 0, rt.p(d_clean), rt.p(d_raw),
                                    rt.stream()), "hs_moe_gate_bwd")
        # w_gate (in,E): d = x^T d_clean ; dx = d_clean w_gate^T (+ d_raw w_noise^T)
        d_wg = torch.empty_like(w_gate)
        raw.gemm(x, d_clean, d_wg, in_f, E, B, a_kind=L.A_RC, b_kind=L.B_RC, lda=in_f, ldb=E)
        d_wn = None
        if noisy:
            d_wn = torch.empty_like(w_noise)
            raw.gemm(x, d_raw, d_wn, in_f, E, B, a_kind=L.A_RC, b_kind=L.B_RC, lda=in_f, ldb=E)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            raw.gemm(d_clean, w_gate, dx, B, in_f, E, a_kind=L.A_KC, b_kind=L.B_KC, lda=E, ldb=E)
            if noisy:
                raw.gemm(d_raw, w_noise, dx, B, in_f, E, a_kind=L.A_KC, b_kind=L.B_KC, lda=E, ldb=E, accumulate=True)
        return dx, d_wg, d_wn, None, None, None, None


def moe_dispatch_index(gates):
    """-> (idx (E,B) int32: idx[e, :count[e]] = rows with gates[:, e] > 0 ascending, counts as a Python list).  The counts
    come back to the host -- the reference's SparseDispatcher does the same (`.tolist()`, moe.py:60): the experts' batch
    sizes are data-dependent launch shapes."""
    gates = _f32c(gates.detach())
    B, E = gates.shape
    idx = torch.empty((E, B), dtype=torch.int32, device=gates.device)
    cnt = torch.empty(E, dtype=torch.int32, device=gates.device)
    L.check(L.lib().hs_moe_dispatch_index(rt.p(gates), B, E, rt.p(idx), rt.p(cnt), rt.stream()), "hs_moe_dispatch_index")
    return idx, cnt.tolist()


class RowsGatherFn(Function):
    """x (B,D), idx (n,) int32 unique -> x[idx] (n,D); backward adds the rows' gradients back into a (B,D) zero tensor."""

    @staticmethod
    def forward(ctx, x, idx, n):
        x = _f32c(x)
        out = torch.empty((n, x.shape[1]), dtype=torch.float32, device=x.device)
        L.check(L.lib().hs_rows_gather(rt.p(x), rt.p(idx), rt.p(out), n, x.shape[1], rt.stream()), "hs_rows_gather")
        ctx.save_for_backward(idx)
        ctx.meta = (x.shape[0], n)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        B, n = ctx.meta
        dout = _f32c(dout)
        dx = torch.zeros((B, dout.shape[1]), dtype=torch.float32, device=dout.device)
        L.check(L.lib().hs_rows_scatter_add(rt.p(dx), rt.p(idx), None, 0, 0, rt.p(dout), n, dout.shape[1], rt.stream()),
                "hs_rows_scatter_add")
        return dx, None, None


class MoESparseCombineFn(Function):
    """y[b] = sum over the experts e that row b was dispatched to of gates[b, e] * out_e[position of b in e's batch]
    (SparseDispatcher.combine, moe.py:86-103: stitched * nonzero gates, index_add).  Experts are added in index order and a
    row occurs once per expert, so the sum is deterministic."""

    @staticmethod
    def forward(ctx, gates, idx, counts, B, *outs):
        gates = _f32c(gates)
        outs = [_f32c(o) for o in outs]
        O = outs[0].shape[1] if outs else 0
        for o in outs:
            if o.shape[0]:
                O = o.shape[1]
        y = torch.zeros((B, O), dtype=torch.float32, device=gates.device)
        E = gates.shape[1]
        lib = L.lib()
        for e, (o, n) in enumerate(zip(outs, counts)):
            if n:
                L.check(lib.hs_rows_scatter_add(rt.p(y), rt.p(idx[e]), rt.p(gates), E, e, rt.p(o), n, O, rt.stream()),
                        "hs_rows_scatter_add")
        ctx.save_for_backward(gates, idx, *outs)
        ctx.counts = counts
        return y

    @staticmethod
    def backward(ctx, dy):
        gates, idx, *outs = ctx.saved_tensors
        counts = ctx.counts
        dy = _f32c(dy)
        E = gates.shape[1]
        dgates = torch.zeros_like(gates)
        douts = []
        lib = L.lib()
        for e, (o, n) in enumerate(zip(outs, counts)):
            d = torch.empty_like(o)
            if n:
                L.check(lib.hs_rows_scatter_add_bwd(rt.p(dy), rt.p(idx[e]), rt.p(gates), E, e, rt.p(o), rt.p(d), rt.p(dgates), n,
                                                    o.shape[1], rt.stream()), "hs_rows_scatter_add_bwd")
            douts.append(d)
        return (dgates, None, None, None, *douts)


class MoECombineFn(Function):
    """y = sum_e gates[:, e, None] * out_e  (dense SparseDispatcher.combine)."""

    @staticmethod
    def forward(ctx, gates, *outs):
        gates = _f32c(gates)
        outs = [_f32c(o) for o in outs]
        B, E = gates.shape
        O = outs[0].shape[1]
        y = torch.empty((B, O), dtype=torch.float32, device=gates.device)
        ptrs = (C.c_void_p * E)(*[o.data_ptr() for o in outs])
        L.check(L.lib().hs_moe_combine_fwd(rt.p(gates), ptrs, rt.p(y), B, E, O, rt.stream()), "hs_moe_combine_fwd")
        ctx.save_for_backward(gates, *outs)
        return y

    @staticmethod
    def backward(ctx, dy):
        gates, *outs = ctx.saved_tensors
        dy = _f32c(dy)
        B, E = gates.shape
        O = outs[0].shape[1]
        douts = [torch.empty_like(o) for o in outs]
        dgates = torch.empty_like(gates)
        ptrs = (C.c_void_p * E)(*[o.data_ptr() for o in outs])
        dptrs = (C.c_void_p * E)(*[o.data_ptr() for o in douts])
        L.check(L.lib().hs_moe_combine_bwd(rt.p(gates), ptrs, rt.p(dy), dptrs, rt.p(dgates), B, E, O, rt.stream()),
                "hs_moe_combine_bwd")
        return (dgates, *douts)


class SupConFn(Function):
    @staticmethod
    def forward(ctx, feat, labels, temperature):
        feat = _f32c(feat)
        labels = labels.contiguous().long()
        B, D = feat.shape
        lib = L.lib()
        ws = torch.empty(lib.hs_supcon_ws_bytes(B, D) // 4, dtype=torch.float32, device=feat.device)
        loss = torch.empty((), dtype=torch.float32, device=feat.device)
        df = torch.empty_like(feat)
        L.check(lib.hs_supcon_loss(rt.p(feat), rt.p(labels), B, D, temperature, rt.p(loss), rt.p(df), rt.p(ws), rt.stream()),
                "hs_supcon_loss")
        ctx.save_for_backward(df)
        return loss

    @staticmethod
    def backward(ctx, g):
        (df,) = ctx.saved_tensors
        g = g.contiguous().float()
        out = torch.empty_like(df)
        L.check(L.lib().hs_mul_dev_scalar(rt.p(df), rt.p(g), rt.p(out), df.numel(), rt.stream()), "hs_mul_dev_scalar")
        return out, None, None


def _resolve_group(group):
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise L.HamspineError("supcon_loss(group=...): torch.distributed is not initialised")
    return dist.group.WORLD if isinstance(group, str) and group == "world" else group


def _gather_rows(t, pg, world):
    """rows of every rank, in rank order, without an autograd graph: on the device for nccl, through host memory otherwise"""
    import torch.distributed as dist
    shape = (world * t.shape[0],) + tuple(t.shape[1:])
    if dist.get_backend(pg) == "nccl":
        out = torch.empty(shape, dtype=t.dtype, device=t.device)
        dist.all_gather_into_tensor(out, t, group=pg)
        return out
    out = torch.empty(shape, dtype=t.dtype)
    dist.all_gather(list(out.chunk(world)), t.cpu(), group=pg)
    return out.to(t.device)


def _require_equal_batches(B, D, pg, world):
    """ValueError on EVERY rank when the local (B, D) differ, before any rank enters the gather (so none is left waiting).
    Host-route backends only: with nccl the check would need a read-back, i.e. a host synchronisation per step, and equal
    sizes are the caller's contract there, as they are for all_gather_into_tensor itself."""
    import torch.distributed as dist
    if dist.get_backend(pg) == "nccl":
        return
    sizes = [torch.zeros(2, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(sizes, torch.tensor([B, D], dtype=torch.int64), group=pg)
    sizes = [tuple(s.tolist()) for s in sizes]
    if any(s != sizes[0] for s in sizes):
        raise ValueError(f"supcon_loss(group=...): every rank must hold the same (batch, dim), got {sizes}")


class SupConTiledFn(Function):
    """hs_supcon_tiled: the loss over all rows (of all ranks of `pg`, if given) and the gradient of this rank's rows, computed
    together in the forward.  grad_scale multiplies the saved gradient (the world size when the trainer averages)."""

    @staticmethod
    def forward(ctx, feat, labels, temperature, pg, average_across_ranks):
        feat = _f32c(feat)
        labels = labels.contiguous().long()
        rt.need_gpu(labels)
        B, D = feat.shape
        if labels.shape != (B,):
            raise L.HamspineError(f"supcon_loss: labels {tuple(labels.shape)} for features {tuple(feat.shape)}")
        row0, scale, allf, alll = 0, 1.0, feat, labels
        if pg is not None:
            import torch.distributed as dist
            world, rank = dist.get_world_size(pg), dist.get_rank(pg)
            _require_equal_batches(B, D, pg, world)
            allf, alll = _gather_rows(feat.detach(), pg, world), _gather_rows(labels, pg, world)
            row0, scale = rank * B, float(world) if average_across_ranks else 1.0
        N = allf.shape[0]
        lib = L.lib()
        nbytes = lib.hs_supcon_tiled_ws_bytes(N, D)
        if nbytes < 0:
            raise L.HamspineError(f"supcon_loss: {N} rows of {D} features are outside the tiled kernel's range "
                                  f"(N <= {L._header.constants['HS_SUPCON_TILED_MAX_N']}, "
                                  f"D <= {L._header.constants['HS_SUPCON_TILED_MAX_D']})")
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=feat.device)
        loss = torch.empty((), dtype=torch.float32, device=feat.device)
        df = torch.empty_like(feat)
        L.check(lib.hs_supcon_tiled(rt.p(allf), rt.p(alll), N, D, row0, B, temperature, scale, rt.p(loss), rt.p(df), rt.p(ws),
                                    rt.stream()), "hs_supcon_tiled")
        ctx.save_for_backward(df)
        return loss

    @staticmethod
    def backward(ctx, g):
        (df,) = ctx.saved_tensors
        g = g.contiguous().float()
        out = torch.empty_like(df)
        L.check(L.lib().hs_mul_dev_scalar(rt.p(df), rt.p(g), rt.p(out), df.numel(), rt.stream()), "hs_mul_dev_scalar")
        return out, None, None, None, None


def supcon_loss(features, labels, temperature=0.07, *, group=None, tiled=None, average_across_ranks=True):
    """SupConLoss(temperature) of the reference (scripts/train.py:23-44) with its gradient.

    group=None: the loss of these rows.  Up to 256 rows take the single-workgroup kernel (hs_supcon_loss) unless tiled=True;
    more rows, or tiled=True, take the tiled MFMA kernels (hs_supcon_tiled).
    group=<process group> or "world": the loss of the step's GLOBAL batch -- features and labels of all ranks are gathered
    (equal local batch sizes are required: ValueError), every rank returns the same loss, and each rank's backward yields the
    gradient of that global loss with respect to its own rows, terms of the other ranks' anchors included.  A contrastive loss
    is not a sum over ranks: the mean of per-rank losses has other negatives, other positives and another gradient.
    average_across_ranks=True (default) multiplies that gradient by the world size, for trainers that AVERAGE parameter
    gradients (hamspine.ddp.DataParallel, torch DDP): after the average every parameter holds exactly the gradient of the
    global loss.  False leaves the factor 1 (trainers that sum)."""
    T = float(temperature)
    if group is not None:
        return SupConTiledFn.apply(features, labels, T, _resolve_group(group), bool(average_across_ranks))
    if tiled is True or (tiled is None and features.shape[0] > 256):
        return SupConTiledFn.apply(features, labels, T, None, False)
    return SupConFn.apply(features, labels, T)


class SupConLoss(torch.nn.Module):
    """The reference's SupConLoss(temperature=0.07) (scripts/train.py:23-44); group: see supcon_loss."""

    def __init__(self, temperature=0.07, group=None):
        super().__init__()
        self.temperature = temperature
        self.group = group

    def forward(self, features, labels):
        return supcon_loss(features, labels, self.temperature, group=self.group)


class KANRegularizationFn(Function):
    """KANLinear.regularization_loss on spline_weight (out, in, coeffs): scalar loss with its gradient (one kernel each)"""

    @staticmethod
    def forward(ctx, w, ra, re):
        rt.need_gpu(w)
        w = w.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=w.device)
        L.check(L.lib().hs_kan_regularization(rt.p(w), w.numel() // w.shape[-1], w.shape[-1], ra, re, rt.p(loss), None, rt.stream()),
                "hs_kan_regularization")
        ctx.save_for_backward(w)
        ctx.meta = (ra, re)
        return loss

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        ra, re = ctx.meta
        dw = torch.empty_like(w)
        L.check(L.lib().hs_kan_regularization(rt.p(w), w.numel() // w.shape[-1], w.shape[-1], ra, re, None, rt.p(dw), rt.stream()),
                "hs_kan_regularization")
        g = g.contiguous().float()
        out = torch.empty_like(dw)
        L.check(L.lib().hs_mul_dev_scalar(rt.p(dw), rt.p(g), rt.p(out), dw.numel(), rt.stream()), "hs_mul_dev_scalar")
        return out, None, None


def kan_regularization(spline_weight, regularize_activation=1.0, regularize_entropy=1.0):
    return KANRegularizationFn.apply(spline_weight, float(regularize_activation), float(regularize_entropy))
