"""Autograd integration of the HIP biGRU recurrence.

Composition (MI355X-first): the time-batched input projections
gi = x @ W_ih^T + b_ih for both directions run as ONE rocBLAS MFMA GEMM in
torch (plain library GEMM); the sequential recurrence runs in the
hand-written persistent HIP kernel (`csrc/gru_kernels.hip`); dW_hh/db_hh are
reduced from the kernel's dGh output by one more plain GEMM. Everything
stays inside torch autograd, so dropout, pooling, head, loss and DDP
compose naturally.

Replaces the reference's `self.gru(input_seq)` cuDNN RNN call site
(biGRU_model.py:102).
"""
import os
from typing import List, Optional, Tuple

import torch

from . import load_extension
from .blas import (chunked_colsum, chunked_outer, chunked_outer_parts,
                   enable_tunableop, split_chunks)

# Minimum padded hidden is 32: the bf16 recurrence tiles MFMA K=32, so
# Hp=16 would give a ZERO-trip GEMM loop (caught by the randomized shape
# sweep; bf16 Hp=16 is also rejected at the binding).
_ALLOWED_HP = [32, 64, 128, 256, 512]


def _pad_h(H: int) -> int:
    for hp in _ALLOWED_HP:
        if H <= hp:
            return hp
    raise ValueError(f"hidden size {H} > {_ALLOWED_HP[-1]} not supported")


def _glue_mode() -> int:
    """FMDA_NATIVE_GLUE, read per call:
    1 (default): weight packing, the head's read of the fp32 masters, the
       pooling casts and the pooled-head feature path (pooled_features) run
       as single HIP kernels; so do the split-K chunk sums of the GRU and
       head weight grads where the kernels can follow the order of torch's
       own sum (_eager_sum_known), and metrics.subset_accuracy. Every one
       of these steps is exact, so a training step computes what the eager
       formulation computes, bit for bit.
    2: also the weight-gradient reductions (finalize_gru_wgrads,
       head_wgrads). They sum in fp32 in their own fixed order, and the
       head's dW / db skip the round trip through bf16, so gradients differ
       from the eager ones in the last bits (fewer launches, not the same
       numbers).
    0: the eager torch formulation of all of it (A/B runs on one build)."""
    return {"0": 0, "2": 2}.get(os.environ.get("FMDA_NATIVE_GLUE", "1"), 1)


def _native_glue() -> bool:
    return _glue_mode() >= 1


def _native_reductions() -> bool:
    return _glue_mode() == 2


def _eager_sum_known(M: int, outputs: int) -> bool:
    """Whether the native kernels can sum the split-K partials of an
    (M, N)^T @ (M, K) chunked_outer with N*K = `outputs` exactly as
    `parts.float().sum(dim=0)` does. That order is derived (and tested) for
    ATen's 64 x 2 reduce block only: 64 chunks, at least 512 outputs, a
    multiple of 4 (the extension's eager_sum_applies checks the same on
    the partials). Everything else, ragged M included, stays eager."""
    return split_chunks(M) == 64 and outputs >= 512 and outputs % 4 == 0


def _fp32_cuda(*tensors) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _pad_gate_rows(w: torch.Tensor, H: int, Hp: int) -> torch.Tensor:
    """(3H, ...) -> (3Hp, ...): zero-pad each of the r/z/n row blocks."""
    if H == Hp:
        return w
    shape = list(w.shape)
    shape[0] = 3 * Hp
    out = w.new_zeros(shape)
    for g in range(3):
        out[g * Hp:g * Hp + H] = w[g * H:(g + 1) * H]
    return out


def _pad_cols(w: torch.Tensor, H: int, Hp: int) -> torch.Tensor:
    """(..., H) -> (..., Hp) zero-pad."""
    if H == Hp:
        return w
    shape = list(w.shape)
    shape[-1] = Hp
    out = w.new_zeros(shape)
    out[..., :H] = w
    return out


def _pack_layer_eager(params, H: int, Hp: int, dtype):
    """Eager pack of one layer. params: per direction (w_ih, w_hh, b_ih,
    b_hh). Returns w_ih_cat (D*3Hp, F), b_ih_cat (D*3Hp), w_hh_cat
    (D, 3Hp, Hp) in `dtype` and b_hh_cat (D, 3Hp) in fp32."""
    w_ihs, w_hhs, b_ihs, b_hhs = [], [], [], []
    for (w_ih, w_hh, b_ih, b_hh) in params:
        w_ihs.append(_pad_gate_rows(w_ih, H, Hp))
        w_hhs.append(_pad_cols(_pad_gate_rows(w_hh, H, Hp), H, Hp))
        b_ihs.append(_pad_gate_rows(b_ih, H, Hp))
        b_hhs.append(_pad_gate_rows(b_hh, H, Hp))
    return (torch.cat(w_ihs, dim=0).to(dtype),
            torch.cat(b_ihs, dim=0).to(dtype),
            torch.stack(w_hhs, dim=0).to(dtype).contiguous(),
            torch.stack(b_hhs, dim=0).float().contiguous())


def _pack_layer(params, H: int, Hp: int, dtype):
    """(w_ih_cat, b_ih_cat, w_hh_cat, b_hh_cat, wt) for one layer: one HIP
    kernel from the fp32 masters, which also emits wt = W_hh^T (D, Hp, 3Hp)
    for the BPTT kernel; the eager pack (wt None: gru_bwd transposes
    itself) for other master dtypes or FMDA_NATIVE_GLUE=0."""
    flat = [t for four in params for t in four]
    if (_native_glue() and _fp32_cuda(*flat)
            and dtype in (torch.bfloat16, torch.float32)):
        return tuple(load_extension().pack_gru_layer(
            [t.detach().contiguous() for t in flat], Hp, dtype))
    return _pack_layer_eager(params, H, Hp, dtype) + (None,)


class _GRURecurrence(torch.autograd.Function):
    """Custom op: (gi, w_hh, b_hh) -> (out, h_last) for 1 or 2 directions.

    gi:  (B, T, n_dir*3Hp) input projections incl. b_ih
    w:   (n_dir, 3Hp, Hp) recurrent weights
    bhh: (n_dir, 3Hp) fp32
    out: (B, T, n_dir*Hp) hidden states (direction-concat layout)
    h_last: (n_dir, B, Hp) fp32
    """

    @staticmethod
    def forward(ctx, gi, w, bhh, h0=None):
        ext = load_extension()
        gi = gi.contiguous()
        w = w.contiguous()
        bhh32 = bhh.to(torch.float32).contiguous()
        h0c = (h0.detach().to(torch.float32).contiguous()
               if h0 is not None else None)
        out, h_last = ext.gru_fwd(gi, w, bhh32, h0c)
        ctx.save_for_backward(gi, w, bhh32, out)
        ctx.h0 = h0c
        return out, h_last

    @staticmethod
    def backward(ctx, d_out, d_hlast):
        ext = load_extension()
        gi, w, bhh32, out = ctx.saved_tensors
        h0c = ctx.h0
        B, T, _ = gi.shape
        n_dir, threeHp, Hp = w.shape
        d_out = d_out.contiguous().to(gi.dtype)
        d_hlast = d_hlast.contiguous().to(torch.float32)
        res = ext.gru_bwd(gi, w, bhh32, out, d_out, d_hlast, 0.0, 0, h0c)
        dgi, dgh, dh0_out, dbhh, _dbih = res[:5]
        dgh0 = res[5] if len(res) > 5 else None

        # dW_hh[n, k] = sum_{b,t} dGh_shifted[b,t,n] * out[b,t,k]: the
        # kernel stores dGh time-shifted so slot t pairs with out[t] — one
        # contiguous MFMA reduction (zero copies); chunked_outer hand-splits
        # the fat K = B*T dimension (the library's unsplit algo is ~5x
        # slower on MI355X). Off-diagonal direction blocks are discarded.
        cross = chunked_outer(dgh.reshape(-1, n_dir * threeHp),
                              out.reshape(-1, n_dir * Hp))
        dw = torch.empty_like(w)
        for d in range(n_dir):
            dw[d] = cross[d * threeHp:(d + 1) * threeHp,
                          d * Hp:(d + 1) * Hp]
            if dgh0 is not None:  # t=0 term pairs with h0, not out
                dw[d] += (dgh0[d].float().t() @ h0c[d]).to(dw.dtype)
        dh0_grad = dh0_out if h0c is not None else None
        return dgi, dw, dbhh, dh0_grad


def gru_directions(gi: torch.Tensor, w: torch.Tensor, bhh: torch.Tensor,
                   h0: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    return _GRURecurrence.apply(gi, w, bhh, h0)


class _IHProjection(torch.autograd.Function):
    """gi = x @ w^T + b with MI355X-tuned backward: dW/db reduce over the
    fat K = B*T axis via chunked_outer instead of the library's unsplit
    fat-K GEMM; dx is skipped entirely when x doesn't require grad (layer-1
    input data)."""

    @staticmethod
    def forward(ctx, x2d, w, b):
        ctx.save_for_backward(x2d, w)
        return torch.addmm(b, x2d, w.t())

    @staticmethod
    def backward(ctx, dgi):
        x2d, w = ctx.saved_tensors
        dgi = dgi.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.matmul(dgi, w)
        if ctx.needs_input_grad[1]:
            dw = chunked_outer(dgi, x2d)
        if ctx.needs_input_grad[2]:
            db = chunked_colsum(dgi).to(dgi.dtype)
        return dx, dw, db


class _FusedDropout(torch.autograd.Function):
    """Counter-based dropout: the mask is a pure function of (seed, index),
    so backward recomputes it instead of materializing a mask tensor
    (reference nn.Dropout call sites, biGRU_model.py:50-52,87-94)."""

    @staticmethod
    def forward(ctx, x, p, seed):
        ext = load_extension()
        ctx.p = p
        ctx.seed = seed
        return ext.dropout_fused(x.contiguous(), p, seed)

    @staticmethod
    def backward(ctx, dy):
        ext = load_extension()
        return ext.dropout_fused(dy.contiguous(), ctx.p, ctx.seed), None, None


def fused_dropout(x: torch.Tensor, p: float) -> torch.Tensor:
    """Training-mode dropout on the HIP engine (bf16 CUDA tensors);
    falls back to torch for other dtypes/devices."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and 0.0 < p < 1.0):
        return torch.nn.functional.dropout(x, p=p, training=True)
    seed = int(torch.empty((), dtype=torch.int64).random_())
    return _FusedDropout.apply(x, p, seed)


class _FusedSpatialDropout(torch.autograd.Function):
    """Channel (Dropout2d) dropout on (B, T, F): the mask is per (b, f) and
    shared across timesteps (reference biGRU_model.py:50-52,87-94 semantics
    without the permute(0,2,1) round trips). Counter-based: backward
    recomputes the identical mask instead of saving it."""

    @staticmethod
    def forward(ctx, x, p, seed):
        ext = load_extension()
        ctx.p = p
        ctx.seed = seed
        return ext.spatial_dropout_fused(x.contiguous(), p, seed)

    @staticmethod
    def backward(ctx, dy):
        ext = load_extension()
        return (ext.spatial_dropout_fused(dy.contiguous(), ctx.p, ctx.seed),
                None, None)


def fused_spatial_dropout(x: torch.Tensor, p: float) -> torch.Tensor:
    """Training-mode spatial dropout on the HIP engine; torch Dropout2d
    fallback for other dtypes/devices."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and 0.0 < p < 1.0):
        y = torch.nn.functional.dropout2d(
            x.permute(0, 2, 1).unsqueeze(-1), p=p, training=True)
        return y.squeeze(-1).permute(0, 2, 1)
    seed = int(torch.empty((), dtype=torch.int64).random_())
    return _FusedSpatialDropout.apply(x, p, seed)


def window_batch(table: torch.Tensor, starts: torch.Tensor, window: int,
                 p: float = 0.0, spatial: bool = False,
                 seed: Optional[int] = None) -> torch.Tensor:
    """(B, window, F) training batch of the windows
    table[starts[b] : starts[b] + window] of a normalised (N, F) table,
    with training-mode input dropout (`spatial`: whole (b, f) channels)
    applied on the way. The table is data: there is no backward.

    bf16 on the GPU: one HIP kernel writes the dropped batch straight from
    the table; the result is bit for bit fused_dropout /
    fused_spatial_dropout of the materialised gather under the same seed.
    fp32 on the GPU gathers with the kernel and takes torch's dropout
    afterwards, CPU tables are indexed: the fallbacks of those two
    functions. seed=None draws one seed from the CPU generator exactly as
    they do (only when a bf16 kernel mask is needed).

    `starts` on the CPU is validated here (0 <= starts <= N - window,
    ValueError before any launch) and uploaded; a `starts` that already
    lives on the table's device is used as is: the caller has validated it,
    checking it here would cost a device sync per batch.
    FMDA_NATIVE_GLUE=0 runs an eager gather followed by the existing
    dropout call (A/B runs on one build)."""
    assert not table.requires_grad, "window_batch: the table is data"
    assert table.dim() == 2 and starts.dim() == 1
    N = table.size(0)
    if window < 1 or window > N:
        raise ValueError(f"window {window} outside [1, {N}]")
    if starts.dtype != torch.int64:
        raise TypeError("window_batch: starts must be int64")
    if starts.numel() < 1:
        raise ValueError("window_batch: no windows")
    if not starts.is_cuda:
        lo, hi = int(starts.min()), int(starts.max())
        if lo < 0 or hi > N - window:
            raise ValueError(
                f"window starts [{lo}, {hi}] outside [0, {N - window}]")
        starts = starts.to(table.device)
    kernel_drop = (table.is_cuda and table.dtype == torch.bfloat16
                   and 0.0 < p < 1.0)
    if (table.is_cuda and _native_glue()
            and table.dtype in (torch.bfloat16, torch.float32)):
        if kernel_drop:
            if seed is None:
                seed = int(torch.empty((), dtype=torch.int64).random_())
            return load_extension().window_batch(table, starts, window, p,
                                                 seed, spatial)
        x = load_extension().window_batch(table, starts, window, 0.0, 0,
                                          False)
    else:
        idx = starts[:, None] + torch.arange(window, device=starts.device)
        x = table[idx]
        if kernel_drop and seed is not None:
            ext = load_extension()
            return (ext.spatial_dropout_fused(x, p, seed) if spatial
                    else ext.dropout_fused(x, p, seed))
    if not p > 0.0:
        return x
    return fused_spatial_dropout(x, p) if spatial else fused_dropout(x, p)


class _DirSumPool(torch.autograd.Function):
    """Fused direction-sum + max/avg temporal pooling on the HIP engine
    (biGRU_model.py:108-133 semantics). Returns (max (B,H), avg (B,H)) in
    the activation dtype; backward assembles the full d_out tensor in one
    kernel instead of an eager add/scatter chain."""

    @staticmethod
    def forward(ctx, out, n_dir):
        ext = load_extension()
        out = out.contiguous()
        # native: the kernels emit max / avg and take their grads in the
        # activation dtype (same rounding points, four cast kernels fewer)
        native = _native_glue()
        maxv, avgv, amax = ext.pool_fwd(out, n_dir, native)
        ctx.save_for_backward(amax)
        ctx.meta = (out.shape[1], n_dir, out.dtype, native)
        return maxv.to(out.dtype), avgv.to(out.dtype)

    @staticmethod
    def backward(ctx, dmax, davg):
        ext = load_extension()
        (amax,) = ctx.saved_tensors
        T, n_dir, dtype, native = ctx.meta
        if native and dmax.dtype == dtype and davg.dtype == dtype:
            # column slices of the (B, 3H) feature gradient are read in
            # place through their row pitch
            if any(g.stride(1) != 1 or g.stride(0) < g.shape[1]
                   for g in (dmax, davg)):
                dmax, davg = dmax.contiguous(), davg.contiguous()
        else:
            dmax, davg = dmax.float().contiguous(), davg.float().contiguous()
        dout = ext.pool_bwd(dmax, davg, amax, T, n_dir, dtype)
        return dout, None


def dirsum_pool(out: torch.Tensor, n_dir: int):
    return _DirSumPool.apply(out, n_dir)


class _PooledFeatures(torch.autograd.Function):
    """(out (B, T, D*H) bf16, raw h_last (D, B, H) fp32) -> feat (B, 3H)
    bf16 = [dirsum(h_last) | max_T | avg_T], one kernel each way. Forward
    and backward give the bits of the chain they replace: the h_n cast,
    hidden_v[-1].sum(0), dirsum_pool, torch.cat and their autograd
    (d_hlast = float(dfeat[:, :H]) for every direction).

    Second form, apply(None, None, *layer) with `layer` the inputs of the
    top _BiGRULayer (x, Hp, the eight masters, h0): that layer and the
    pooling as one node. The forward runs the same kernels; in the backward
    gru_bwd builds d_out and d_hlast from (dfeat, amax) in its own prologue
    instead of reading the (B, T, D*H) tensor pool_features_bwd would have
    written (fused_pool_bwd_native). Every bit stays what the two nodes
    compute."""

    @staticmethod
    def forward(ctx, out, h_last, *layer):
        ext = load_extension()
        saved = ()
        ctx.fused = bool(layer)
        if layer:
            (out, h_last), saved = _BiGRULayer.run_forward(
                ctx, *layer[:10], 0.0, 0, layer[10])
        feat, amax = ext.pool_features_fwd(out.contiguous(),
                                           h_last.contiguous())
        ctx.save_for_backward(*saved, amax)
        ctx.pool_meta = (out.shape[1], h_last.shape[0])
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        ext = load_extension()
        *saved, amax = ctx.saved_tensors
        T, n_dir = ctx.pool_meta
        # the fused kernel loads dfeat rows in 16-byte pieces
        if (dfeat.dtype != torch.bfloat16 or dfeat.stride(1) != 1
                or dfeat.stride(0) < dfeat.shape[1]
                or (ctx.fused and dfeat.stride(0) % 8 != 0)):
            dfeat = dfeat.to(torch.bfloat16).contiguous()
        if not ctx.fused:
            d_out, d_hlast = ext.pool_features_bwd(dfeat, amax, T, n_dir)
            return d_out, d_hlast
        if dfeat.data_ptr() % 16 != 0:
            dfeat = dfeat.clone(memory_format=torch.contiguous_format)
        g = _BiGRULayer.run_backward(ctx, tuple(saved), None, None,
                                     dfeat=dfeat, amax=amax, x_index=2)
        return (None, None) + g[:10] + (g[12],)


# fmda_pool_fwd_launch gives grids below this many column pairs to the
# wave-per-pair kernel, which sums T in a lane-butterfly order
_POOL_SMALL_GRID = 4096


def pooled_features_native(x: torch.Tensor, H: int) -> bool:
    """Whether the model input x (B, T, F) gets its pooled features from
    pooled_features(out, raw h_last): bf16 on the GPU, whole 8-column
    groups, unpadded H, native glue on, and a grid that dirsum_pool gives
    to its thread-per-column kernel. Below that grid size (the batch-1
    predict path) dirsum_pool sums T in another order, so the eager chain
    stays and results stay what they were."""
    return (_native_glue() and x.is_cuda and x.dtype == torch.bfloat16
            and H % 8 == 0 and H <= _ALLOWED_HP[-1] and _pad_h(H) == H
            and x.shape[0] * (H // 2) >= _POOL_SMALL_GRID)


def pooled_features(out: torch.Tensor, h_last: torch.Tensor) -> torch.Tensor:
    return _PooledFeatures.apply(out, h_last)


class _HeadLoss(torch.autograd.Function):
    """Fused classifier head + BCEWithLogitsLoss(weight, pos_weight):
    one kernel computes logits, sigmoid and the mean loss; backward is one
    kernel (dlogits + dx) plus split-K dW/db reductions. Returns
    (loss, logits); logits are non-differentiable (metrics only)."""

    @staticmethod
    def forward(ctx, x2d, W, b, y, wgt, pw):
        ext = load_extension()
        x2d = x2d.contiguous()
        logits, sig, loss_sum = ext.head_loss_fwd(
            x2d, W.contiguous(), b.contiguous(), y.contiguous(),
            wgt.contiguous(), pw.contiguous())
        B, C = logits.shape
        loss = (loss_sum / float(B * C)).reshape(())
        ctx.save_for_backward(x2d, W, y, wgt, pw, sig)
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        ext = load_extension()
        x2d, W, y, wgt, pw, sig = ctx.saved_tensors
        dlogits, dx = ext.head_loss_bwd(sig, y, wgt, pw,
                                        dloss.reshape(1).float().contiguous(),
                                        W, x2d.dtype)
        dl = dlogits.to(x2d.dtype)
        dW = chunked_outer(dl, x2d)
        db = dlogits.sum(dim=0).to(W.dtype)
        return dx, dW, db, None, None, None


class _HeadLossMaster(torch.autograd.Function):
    """_HeadLoss with the fp32 master W / b as the differentiable inputs:
    the kernels round them to x's dtype in registers (loss, logits and dx
    are bit-identical to _HeadLoss on the cast copies), so the two cast
    kernels of the forward go. dW / db are, by default, computed and
    rounded exactly as _HeadLoss plus autograd's cast-back would; with
    FMDA_NATIVE_GLUE=2 they come in fp32 from one two-stage reduction over
    the batch (no bf16 rounding: close to, not equal to, the default)."""

    @staticmethod
    def forward(ctx, x2d, W, b, y, wgt, pw):
        ext = load_extension()
        ctx.native_reductions = _native_reductions()
        x2d = x2d.contiguous()
        W = W.contiguous()
        y, wgt, pw = y.contiguous(), wgt.contiguous(), pw.contiguous()
        logits, sig, loss_sum, _ = ext.head_loss_fwd_master(
            x2d, W, b.contiguous(), y, wgt, pw)
        B, C = logits.shape
        loss = (loss_sum / float(B * C)).reshape(())
        ctx.save_for_backward(x2d, W, y, wgt, pw, sig)
        ctx.mark_non_differentiable(logits)
        return loss, logits

    @staticmethod
    def backward(ctx, dloss, _dlogits):
        ext = load_extension()
        x2d, W, y, wgt, pw, sig = ctx.saved_tensors
        gscale = dloss.reshape(1).float().contiguous()
        if ctx.native_reductions:
            dlogits, dx = ext.head_loss_bwd_master(sig, y, wgt, pw, gscale,
                                                   W, x2d.dtype)
            dW, db = ext.head_wgrads(dlogits, x2d)
        elif _eager_sum_known(x2d.shape[0], W.numel()):
            # the chain of the branch below in 4 launches: the kernel also
            # emits dlogits.to(dtype), the split-K bmm stays the library's,
            # and one kernel sums its partials in the eager sum's order and
            # applies the two casts to dW and db. Same bits.
            dlogits, dx, dl = ext.head_loss_bwd_master(
                sig, y, wgt, pw, gscale, W, x2d.dtype, True)
            dW, db = ext.head_wgrads_eager(chunked_outer_parts(dl, x2d),
                                           dlogits.sum(dim=0))
        else:
            dlogits, dx = ext.head_loss_bwd_master(sig, y, wgt, pw, gscale,
                                                   W, x2d.dtype)
            # _HeadLoss.backward on the cast copies, then the cast-back of
            # W.to(dtype) / b.to(dtype): the same values, rounding included
            dW = chunked_outer(dlogits.to(x2d.dtype), x2d).to(W.dtype)
            db = dlogits.sum(dim=0).to(x2d.dtype).to(W.dtype)
        return dx, dW, db, None, None, None


def fused_head_loss(x2d, weight, bias, y, wgt, pw):
    """(loss, logits) for the reference head + class-weighted BCE
    (biGRU_model.py:137 + notebook cell 29 loss)."""
    if (_native_glue() and x2d.is_cuda and _fp32_cuda(weight, bias)
            and x2d.dtype in (torch.bfloat16, torch.float32)):
        return _HeadLossMaster.apply(x2d, weight, bias, y.float(),
                                     wgt.float(), pw.float())
    Wc = weight.to(x2d.dtype)
    bc = bias.to(x2d.dtype)
    return _HeadLoss.apply(x2d, Wc, bc, y.float(), wgt.float(), pw.float())


def _unpad_gate_rows(w, H, Hp):
    """(3Hp, ...) -> (3H, ...): inverse of _pad_gate_rows."""
    if H == Hp:
        return w
    return torch.cat([w[g * Hp:g * Hp + H] for g in range(3)], dim=0)


class _BiGRULayer(torch.autograd.Function):
    """One (bi)directional GRU layer as a single autograd node: weight
    pack/cast, the input-projection MFMA GEMM, and the persistent
    recurrence kernels. Collapsing the eager pack/cast/cat graph removed
    ~80 four-microsecond kernels per training step; both bias gradients
    come straight from the BPTT kernel's register accumulators.
    Parameter tensors are the raw fp32 nn.GRU masters."""

    @staticmethod
    def forward(ctx, x, Hp, w_ih0, w_hh0, b_ih0, b_hh0,
                w_ih1, w_hh1, b_ih1, b_hh1, out_drop_p=0.0,
                out_drop_seed=0, h0=None):
        res, saved = _BiGRULayer.run_forward(
            ctx, x, Hp, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1,
            b_hh1, out_drop_p, out_drop_seed, h0)
        ctx.save_for_backward(*saved)
        return res

    @staticmethod
    def run_forward(ctx, x, Hp, w_ih0, w_hh0, b_ih0, b_hh0,
                    w_ih1, w_hh1, b_ih1, b_hh1, out_drop_p, out_drop_seed,
                    h0):
        """The layer's forward for this node and _PooledFeatures: returns
        (outputs, tensors to save); the caller saves them."""
        ext = load_extension()
        D = 2 if w_ih1 is not None else 1
        H = w_hh0.shape[1]
        dtype = x.dtype
        B, T, F = x.shape
        params = [(w_ih0, w_hh0, b_ih0, b_hh0)]
        if D == 2:
            params.append((w_ih1, w_hh1, b_ih1, b_hh1))
        with torch.no_grad():
            # w_ih_cat (D*3Hp, F), b_ih_cat (D*3Hp), w_hh_cat (D, 3Hp, Hp),
            # b_hh_cat (D, 3Hp) fp32, wt (D, Hp, 3Hp) or None
            w_ih_cat, b_ih_cat, w_hh_cat, b_hh_cat, wt = _pack_layer(
                params, H, Hp, dtype)
        x2d = x.reshape(B * T, F)
        gi = torch.addmm(b_ih_cat, x2d, w_ih_cat.t()).view(B, T, -1)
        h0c = h0.detach().contiguous() if h0 is not None else None
        # out_drop_p > 0: the fwd kernel emits out AND the dropped copy
        # (the next layer's input) from its store epilogue — no separate
        # dropout pass; the mask is recomputed in the BPTT kernel's d_out
        # read (backward half of the fusion).
        res = ext.gru_fwd(gi, w_hh_cat, b_hh_cat, h0c, out_drop_p,
                          out_drop_seed)
        out, h_last = res[0], res[1]
        saved = (x2d, w_ih_cat, w_hh_cat, b_hh_cat, gi, out, wt)
        ctx.h0 = h0c
        ctx.meta = (D, H, Hp, out_drop_p, out_drop_seed)
        ctx.native_reductions = _native_reductions()
        ctx.native_glue = _native_glue()
        ctx.set_materialize_grads(False)
        if len(res) > 2:
            return (out, h_last, res[2]), saved
        return (out, h_last), saved

    @staticmethod
    def backward(ctx, d_out, d_hlast, d_outdrop=None):
        return _BiGRULayer.run_backward(ctx, ctx.saved_tensors, d_out,
                                        d_hlast, d_outdrop)

    @staticmethod
    def run_backward(ctx, saved, d_out, d_hlast, d_outdrop=None,
                     dfeat=None, amax=None, x_index=0):
        """The layer's backward from (d_out, d_hlast), or from the pooled
        head's (dfeat, amax), which gru_bwd turns into both itself (the
        second form of _PooledFeatures, where x is input `x_index`)."""
        ext = load_extension()
        x2d, w_ih_cat, w_hh_cat, b_hh_cat, gi, out, wt = saved
        D, H, Hp, drop_p, drop_seed = ctx.meta
        need_dx = ctx.needs_input_grad[x_index]
        if dfeat is not None:
            res = ext.gru_bwd(gi, w_hh_cat, b_hh_cat, out, None, None,
                              0.0, 0, ctx.h0, wt, dfeat, amax)
            return _BiGRULayer.finish_backward(ctx, saved, res, need_dx)
        if drop_p > 0:
            # the raw `out` output feeds nothing downstream when the fused
            # dropout path is active (h_n comes from h_last; the layer
            # above consumes the DROPPED output) — its grad must be empty
            assert d_out is None, "unexpected grad on raw out with fused dropout"
            d_out = d_outdrop
        if d_out is None:
            d_out = torch.zeros_like(out)
        if d_hlast is None:
            d_hlast = out.new_zeros(
                (w_hh_cat.shape[0], out.shape[0], Hp), dtype=torch.float32)
        d_out = d_out.contiguous().to(gi.dtype)
        d_hlast = d_hlast.contiguous().float()
        h0c = ctx.h0
        # wt (from the native pack) spares gru_bwd its own transpose
        res = ext.gru_bwd(gi, w_hh_cat, b_hh_cat, out, d_out, d_hlast,
                          drop_p, drop_seed, h0c, wt)
        return _BiGRULayer.finish_backward(ctx, saved, res, need_dx)

    @staticmethod
    def finish_backward(ctx, saved, res, need_dx):
        """dx and the weight / bias gradients from gru_bwd's outputs."""
        ext = load_extension()
        x2d, w_ih_cat, w_hh_cat, b_hh_cat, gi, out, wt = saved
        D, H, Hp, _, _ = ctx.meta
        h0c = ctx.h0
        dgi, dgh, dh0_out, dbhh, dbih = res[:5]
        dgh0 = res[5] if len(res) > 5 else None
        M = dgi.shape[0] * dgi.shape[1]
        dx = None
        if need_dx:
            dx = torch.matmul(dgi.reshape(M, -1), w_ih_cat)
            dx = dx.view(dgi.shape[0], dgi.shape[1], -1)
        dh0_grad = dh0_out if h0c is not None else None

        if wt is not None and ctx.native_reductions and dgh0 is None:
            # FMDA_NATIVE_GLUE=2: the split-K partials of dGi^T x and
            # dGh^T out go straight to one kernel that sums the chunks in
            # fp32 (ascending, not torch's order) and writes the four
            # contiguous master-shaped grads; it reads only the diagonal
            # direction blocks of the dW_hh partials
            wg = ext.finalize_gru_wgrads(
                chunked_outer_parts(dgi.reshape(M, -1), x2d),
                chunked_outer_parts(dgh.reshape(M, -1), out.reshape(M, -1)),
                D, H, Hp)
            wgrads = [(wg[2 * d], wg[2 * d + 1]) for d in range(D)]
        elif (ctx.native_glue and dgh0 is None
              and dgi.dtype in (torch.bfloat16, torch.float32)
              and _eager_sum_known(M, D * 3 * Hp * x2d.shape[1])
              and _eager_sum_known(M, D * 3 * Hp * D * Hp)):
            # default mode: the same kernel shape, but the 64 chunks are
            # summed in the order of the eager `parts.float().sum(dim=0)`
            # below, so the four grads are the eager chain's bits: per
            # layer 2 casts, 2 sums, D strided copies (and the unpadding
            # copies) become one launch
            wg = ext.finalize_gru_wgrads(
                chunked_outer_parts(dgi.reshape(M, -1), x2d),
                chunked_outer_parts(dgh.reshape(M, -1), out.reshape(M, -1)),
                D, H, Hp, True)
            wgrads = [(wg[2 * d], wg[2 * d + 1]) for d in range(D)]
        else:
            # dW_hh via the time-shifted dGh and one split-K reduction (fp32
            # out: the grads feed fp32 masters, skip the bf16 round trip)
            cross = chunked_outer(dgh.reshape(M, -1), out.reshape(M, -1),
                                  out_fp32=True)
            if dgh0 is not None:
                # t=0 term of dW_hh: dGh_0 (x) h0 (boundary slot holds zeros)
                for d in range(D):
                    cross[d * 3 * Hp:(d + 1) * 3 * Hp,
                          d * Hp:(d + 1) * Hp] += dgh0[d].float().t() @ h0c[d]
            # dW_ih for both directions in one split-K reduction
            dwih_cat = chunked_outer(dgi.reshape(M, -1), x2d, out_fp32=True)
            wgrads = []
            for d in range(D):
                dwih = dwih_cat[d * 3 * Hp:(d + 1) * 3 * Hp]
                # the column-block slice is non-contiguous; the fused
                # optimizer (and DDP flattening) need contiguous grads
                dwhh = cross[d * 3 * Hp:(d + 1) * 3 * Hp,
                             d * Hp:(d + 1) * Hp].contiguous()
                wgrads.append((_unpad_gate_rows(dwih, H, Hp),
                               _unpad_gate_rows(dwhh, H, Hp)[:, :H]))

        grads = [wgrads[d] + (_unpad_gate_rows(dbih[d], H, Hp),
                              _unpad_gate_rows(dbhh[d], H, Hp))
                 for d in range(D)]
        if D == 1:
            grads.append((None, None, None, None))
        (a0, b0, c0, e0), (a1, b1, c1, e1) = grads
        return (dx, None, a0, b0, c0, e0, a1, b1, c1, e1, None, None,
                dh0_grad)


def _fused_pool_bwd() -> bool:
    """FMDA_FUSED_POOL_BWD, read per call like FMDA_NATIVE_GLUE: 0 keeps the
    top layer and the pooled features two autograd nodes, with d_out
    written by pool_features_bwd and read back by gru_bwd (A/B runs)."""
    return os.environ.get("FMDA_FUSED_POOL_BWD", "1") != "0"


def fused_pool_bwd_native(x: torch.Tensor, H: int) -> bool:
    """Whether the top layer of a stack fed x (B, T, F) and its pooled
    features run as one node (_PooledFeatures' second form): the
    pooled_features_native
    conditions, H == Hp == 128, T <= 256 (amax travels as one byte),
    training with grad enabled, and the switch on."""
    return (_fused_pool_bwd() and pooled_features_native(x, H)
            and H == 128 and x.shape[1] <= 256 and torch.is_grad_enabled())



# Bumped by FusedClipAdam.step(): its HIP kernel mutates the masters via
# raw pointers, which does NOT advance torch's per-tensor _version counter,
# so the packed-weight cache must also key on this epoch.
_PACK_EPOCH = 0


def _packed_inference_weights(gru_module, layer, params, Hp, H, dtype):
    """Inference-path cache of the per-layer packed/cast weights.

    Training re-packs every step (Adam mutates the masters), but in
    eval/no-grad the ~8 cat/cast kernels per layer are pure overhead —
    at batch=1 streaming they were ~40% of the captured predict graph.
    Keyed by the params' in-place version counters, so an optimizer step
    (in-place update) invalidates the cache automatically."""
    key = f"_fmda_pack_l{layer}_{dtype}_{params[0][0].device}"
    flat = [t for four in params for t in four]
    versions = (_PACK_EPOCH,) + tuple(t._version for t in flat)
    ent = getattr(gru_module, key, None)
    if ent is not None and ent[0] == versions:
        return ent[1]
    packed = _pack_layer(params, H, Hp, dtype)[:4]
    setattr(gru_module, key, (versions, packed))
    return packed


def _layer_params(gru_module, layer: int, D: int):
    """Per direction (w_ih, w_hh, b_ih, b_hh) masters of one nn.GRU layer."""
    params = []
    for sfx_d in ["", "_reverse"][:D]:
        sfx = f"l{layer}{sfx_d}"
        params.append((getattr(gru_module, f"weight_ih_{sfx}"),
                       getattr(gru_module, f"weight_hh_{sfx}"),
                       getattr(gru_module, f"bias_ih_{sfx}"),
                       getattr(gru_module, f"bias_hh_{sfx}")))
    return params


def _unpad_out(out_pad: torch.Tensor, H: int, Hp: int, D: int):
    """(B, T, D*Hp) kernel output -> (B, T, D*H)."""
    if Hp == H:
        return out_pad
    if D == 2:
        return torch.cat([out_pad[..., :H], out_pad[..., Hp:Hp + H]], dim=-1)
    return out_pad[..., :H]


def _infer_layer(gru_module, layer, params, Hp, H, inp, h0=None):
    """Inference fast path of one layer: cached packed weights, one
    projection GEMM, direct kernel call. Returns (out_pad, h_last)."""
    w_ih_cat, b_ih_cat, w_hh_cat, b_hh_cat = _packed_inference_weights(
        gru_module, layer, params, Hp, H, inp.dtype)
    B, T, F = inp.shape
    gi = torch.addmm(b_ih_cat, inp.reshape(B * T, F),
                     w_ih_cat.t()).view(B, T, -1)
    return load_extension().gru_fwd(gi, w_hh_cat, b_hh_cat, h0)


def bigru_stack(x: torch.Tensor, gru_module: torch.nn.GRU, n_layers: int,
                bidirectional: bool, dropout_p: float, training: bool,
                hidden: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """nn.GRU(batch_first=True)-equivalent stacked biGRU on the HIP engine.

    Weights come from the nn.GRU parameter container (reference state_dict
    layout); masters stay fp32 and are packed/cast to the compute dtype
    inside the single-layer autograd node. Replaces the reference's
    `self.gru(input_seq)` call (biGRU_model.py:102); `hidden` is the
    optional (L*D, B, H) initial state of the nn.GRU signature."""
    out, h_n, _ = _bigru_stack(x, gru_module, n_layers, bidirectional,
                               dropout_p, training, hidden)
    return out, h_n


def bigru_stack_raw(x: torch.Tensor, gru_module: torch.nn.GRU, n_layers: int,
                    bidirectional: bool, dropout_p: float, training: bool,
                    hidden: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """bigru_stack for a caller that wants only the top layer's state:
    returns (out, h_last) with h_last the top layer's raw fp32 (D, B, Hp)
    final state as the recurrence kernel left it. h_n is not assembled, so
    the lower layers' final states cost no cast and no cat."""
    out, _, h_last = _bigru_stack(x, gru_module, n_layers, bidirectional,
                                  dropout_p, training, hidden, need_h_n=False)
    return out, h_last


def bigru_stack_features(x: torch.Tensor, gru_module: torch.nn.GRU,
                         n_layers: int, bidirectional: bool,
                         dropout_p: float, training: bool,
                         hidden: Optional[torch.Tensor] = None
                         ) -> torch.Tensor:
    """pooled_features(*bigru_stack_raw(...)) for a caller that holds
    pooled_features_native(x, H): the (B, 3H) features alone. Where
    fused_pool_bwd_native holds too, the top layer and the pooling are one
    autograd node and d_out is never materialised."""
    feat, _, _ = _bigru_stack(x, gru_module, n_layers, bidirectional,
                              dropout_p, training, hidden, need_h_n=False,
                              pooled=True)
    return feat


def _bigru_stack(x, gru_module, n_layers, bidirectional, dropout_p, training,
                 hidden=None, need_h_n=True, pooled=False):
    """(out, h_n or None, raw fp32 h_last of the top layer); with `pooled`
    (pooled features, None, None)."""
    enable_tunableop()
    D = 2 if bidirectional else 1
    H = gru_module.hidden_size
    Hp = _pad_h(H)
    assert not (pooled and need_h_n)
    fuse_top = pooled and fused_pool_bwd_native(x, H)

    h0_layers = [None] * n_layers
    if hidden is not None:
        B = x.shape[0]
        assert hidden.shape == (n_layers * D, B, H), \
            f"hidden must be ({n_layers * D}, {B}, {H})"
        hid32 = hidden.float()
        for layer in range(n_layers):
            h0_layers[layer] = _pad_cols(
                hid32[layer * D:(layer + 1) * D], H, Hp).contiguous()

    h_n_parts: List[torch.Tensor] = []
    inp = x
    for layer in range(n_layers):
        p = _layer_params(gru_module, layer, D)
        # inter-layer dropout planned for this layer's output? choose the
        # seed NOW so the producing layer's BPTT kernel can apply the same
        # counter-based mask at its d_out read (backward pass fused away)
        drop_here = (training and dropout_p > 0 and layer < n_layers - 1)
        # fully fused inter-layer dropout: v3 (Hp=128) and column-split
        # (Hp=512, zero-h0) kernels emit the dropped copy in forward and
        # recompute the mask at the backward d_out read
        defer = (drop_here and Hp == H and Hp in (128, 512)
                 and x.dtype == torch.bfloat16 and x.is_cuda
                 and (Hp == 128 or (h0_layers[layer] is None
                      and os.environ.get("FMDA_CS_DROP", "1") != "0")))
        seed = (int(torch.empty((), dtype=torch.int64).random_())
                if defer else 0)
        dp = (dropout_p, seed) if defer else (0.0, 0)

        h0_l = h0_layers[layer]
        dropped_pad = None
        if not training and not torch.is_grad_enabled():
            out_pad, h_last = _infer_layer(gru_module, layer, p, Hp, H, inp,
                                           h0_l)
        elif fuse_top and training and layer == n_layers - 1:
            p1 = p[1] if D == 2 else (None, None, None, None)
            return (_PooledFeatures.apply(None, None, inp, Hp, *p[0], *p1,
                                          h0_l), None, None)
        elif D == 2:
            res = _BiGRULayer.apply(inp, Hp, *p[0], *p[1], *dp, h0_l)
            out_pad, h_last = res[0], res[1]
            dropped_pad = res[2] if len(res) > 2 else None
        else:
            res = _BiGRULayer.apply(inp, Hp, *p[0],
                                    None, None, None, None, *dp, h0_l)
            out_pad, h_last = res[0], res[1]
            dropped_pad = res[2] if len(res) > 2 else None

        out = _unpad_out(out_pad, H, Hp, D)
        if need_h_n:
            h_n_parts.append(h_last[:, :, :H].to(x.dtype))

        inp = out
        if drop_here:
            if defer:
                # fused: the fwd kernel already emitted the dropped copy
                inp = dropped_pad
            else:
                inp = fused_dropout(inp, dropout_p)

    if pooled:
        return pooled_features(inp, h_last), None, None
    h_n = torch.cat(h_n_parts, dim=0) if need_h_n else None  # (L*D, B, H)
    return inp, h_n, h_last


def table_projections(table: torch.Tensor, gru_module: torch.nn.GRU,
                      bidirectional: bool) -> torch.Tensor:
    """Layer-0 input projections of every table row, once: gi_rows
    (N, D*3Hp) = table @ W_ih^T + b_ih. A row's projection does not depend
    on the window it sits in (eval mode: no input dropout), so every
    sliding window over the table reads these rows in place."""
    assert not torch.is_grad_enabled(), "windowed inference runs under no_grad"
    enable_tunableop()
    D = 2 if bidirectional else 1
    H = gru_module.hidden_size
    Hp = _pad_h(H)
    w_ih_cat, b_ih_cat, _, _ = _packed_inference_weights(
        gru_module, 0, _layer_params(gru_module, 0, D), Hp, H, table.dtype)
    return torch.addmm(b_ih_cat, table, w_ih_cat.t())


def bigru_stack_windows(table: torch.Tensor, gru_module: torch.nn.GRU,
                        n_layers: int, bidirectional: bool, window: int,
                        stride: int = 1,
                        gi_rows: Optional[torch.Tensor] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """bigru_stack (inference, zero h0) over every sliding window of a
    normalised (N, F) table, without materialising the windows: window b is
    table[b*stride : b*stride + window]. Layer 0 runs the recurrence
    straight on the shared table of projections (gru_fwd_windows); layers
    above take the ordinary inference path, their inputs differ per window.
    gi_rows: table_projections of these table rows if the caller already
    has them (a chunked caller computes them once for the whole table and
    passes matching row-slices). Returns (out (B, window, D*H),
    h_n (L*D, B, H)) like bigru_stack."""
    assert not torch.is_grad_enabled(), "windowed inference runs under no_grad"
    enable_tunableop()
    D = 2 if bidirectional else 1
    H = gru_module.hidden_size
    Hp = _pad_h(H)
    if gi_rows is None:
        gi_rows = table_projections(table, gru_module, bidirectional)
    assert gi_rows.shape[0] == table.shape[0], "gi_rows / table rows differ"
    h_n_parts: List[torch.Tensor] = []
    inp = None
    for layer in range(n_layers):
        p = _layer_params(gru_module, layer, D)
        if layer == 0:
            _, _, w_hh_cat, b_hh_cat = _packed_inference_weights(
                gru_module, 0, p, Hp, H, gi_rows.dtype)
            out_pad, h_last = load_extension().gru_fwd_windows(
                gi_rows, w_hh_cat, b_hh_cat, window, stride)
        else:
            out_pad, h_last = _infer_layer(gru_module, layer, p, Hp, H, inp)
        inp = _unpad_out(out_pad, H, Hp, D)
        h_n_parts.append(h_last[:, :, :H].to(gi_rows.dtype))
    return inp, torch.cat(h_n_parts, dim=0)
