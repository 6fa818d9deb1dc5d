"""The glue kernels (csrc/glue_kernels.hip and the activation-dtype pooling
variants) against the eager formulation they replace, which stays reachable
with FMDA_NATIVE_GLUE=0.

The default mode (1) uses only the exact kernels (casts, padding, the
forward of the head, pooling): everything it computes, gradients included,
must equal the eager path bit for bit. Mode 2 adds the kernels that sum in
their own order; those are held to the a-priori fp32 reordering bound
against an fp64 sum of the very partials the kernel read.
"""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, FP32], ids=["bf16", "fp32"])


def _ext():
    from fmda_amd.ops import load_extension
    return load_extension()


@contextlib.contextmanager
def glue(mode: int):
    """Run a block with FMDA_NATIVE_GLUE=mode: 0 eager, 1 the exact native
    kernels (default), 2 also the native weight-gradient reductions."""
    old = os.environ.get("FMDA_NATIVE_GLUE")
    os.environ["FMDA_NATIVE_GLUE"] = str(int(mode))
    try:
        yield
    finally:
        if old is None:
            del os.environ["FMDA_NATIVE_GLUE"]
        else:
            os.environ["FMDA_NATIVE_GLUE"] = old


def _gru_masters(H, F, D, seed, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    return [tuple((torch.randn(*shape, generator=g) * 0.3).to(device)
                  for shape in [(3 * H, F), (3 * H, H), (3 * H,), (3 * H,)])
            for _ in range(D)]


# ---------------------------------------------------------------------------
# pack_gru_layer
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("H,F,D,dtype", [
    (128, 96, 2, BF16),    # the flagship layer 0: no padding
    (100, 7, 2, BF16),     # padded rows and columns, odd F
    (8, 5, 1, BF16),       # one direction, Hp = 32 = 4 H
    (16, 12, 2, FP32),
])
def test_pack_gru_layer_equals_eager_pack(H, F, D, dtype):
    from fmda_amd.ops import interface as itf
    Hp = itf._pad_h(H)
    params = _gru_masters(H, F, D, seed=3)
    with glue(0):
        ref = itf._pack_layer(params, H, Hp, dtype)
    assert ref[4] is None
    # what gru_bwd derives itself when no wt is passed
    ref = ref[:4] + (ref[2].transpose(1, 2).contiguous(),)
    with glue(1):
        got = itf._pack_layer(params, H, Hp, dtype)
    names = ["w_ih_cat", "b_ih_cat", "w_hh_cat", "b_hh_cat", "wt"]
    for name, a, r in zip(names, got, ref):
        assert a.dtype == r.dtype and a.shape == r.shape, name
        assert a.is_contiguous(), name
        assert torch.equal(a, r), name
    w_ih_cat, b_ih_cat, w_hh_cat, b_hh_cat, wt = got
    assert b_hh_cat.dtype == FP32
    # pad rows / columns are exactly zero
    rows = w_ih_cat.view(D, 3, Hp, F)
    assert not rows[:, :, H:].any()
    assert not b_ih_cat.view(D, 3, Hp)[:, :, H:].any()
    assert not b_hh_cat.view(D, 3, Hp)[:, :, H:].any()
    hh = w_hh_cat.view(D, 3, Hp, Hp)
    assert not hh[:, :, H:].any() and not hh[..., H:].any()
    t = wt.view(D, Hp, 3, Hp)
    assert not t[:, H:].any() and not t[..., H:].any()


# ---------------------------------------------------------------------------
# finalize_gru_wgrads
# ---------------------------------------------------------------------------

def _unpad_rows(w, H, Hp):
    return torch.cat([w[g * Hp:g * Hp + H] for g in range(3)], dim=0)


@DTYPES
@pytest.mark.parametrize("F", [5, 96])
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("Hp,H", [(32, 8), (128, 100), (128, 128)])
@pytest.mark.parametrize("c", [1, 4])
def test_finalize_gru_wgrads_fp32_reordering_bound(c, Hp, H, D, F, dtype):
    g = torch.Generator().manual_seed(100 * c + Hp + H + 10 * D + F)
    part_ih = torch.randn(c, D * 3 * Hp, F, generator=g).to(dtype).cuda()
    part_hh = torch.randn(c, D * 3 * Hp, D * Hp, generator=g).to(dtype).cuda()
    if D == 2:
        # the off-diagonal direction blocks must never be read
        for d in range(2):
            part_hh[:, d * 3 * Hp:(d + 1) * 3 * Hp,
                    (1 - d) * Hp:(2 - d) * Hp] = float("nan")
    got = _ext().finalize_gru_wgrads(part_ih, part_hh, D, H, Hp)
    again = _ext().finalize_gru_wgrads(part_ih, part_hh, D, H, Hp)
    assert len(got) == 2 * D
    for d in range(D):
        rows = slice(d * 3 * Hp, (d + 1) * 3 * Hp)
        p_ih = part_ih[:, rows].double()
        p_hh = part_hh[:, rows, d * Hp:(d + 1) * Hp].double()
        for name, a, b, p in [("dw_ih", got[2 * d], again[2 * d], p_ih),
                              ("dw_hh", got[2 * d + 1], again[2 * d + 1],
                               p_hh)]:
            ref = _unpad_rows(p.sum(dim=0), H, Hp)
            mag = _unpad_rows(p.abs().sum(dim=0), H, Hp)
            if name == "dw_hh":
                ref, mag = ref[:, :H], mag[:, :H]
            assert a.dtype == FP32 and a.is_contiguous(), name
            assert a.shape == ref.shape, (name, a.shape, ref.shape)
            assert torch.isfinite(a).all(), name
            err = (a.double() - ref).abs()
            bound = c * 2.0 ** -23 * mag
            assert (err <= bound).all(), (name, d, float(err.max()))
            assert torch.equal(a, b), name      # fixed summation order


# ---------------------------------------------------------------------------
# head: forward on the fp32 masters, fp32 two-stage dW / db
# ---------------------------------------------------------------------------

def _head_inputs(B, K, dtype):
    C = 4
    g = torch.Generator().manual_seed(1000 + B + K)
    x = (torch.randn(B, K, generator=g) * 0.5).to(dtype).cuda()
    W = (torch.randn(C, K, generator=g) * 0.2).cuda()
    b = (torch.randn(C, generator=g) * 0.1).cuda()
    y = (torch.rand(B, C, generator=g) < 0.3).float().cuda()
    wgt = (torch.rand(C, generator=g) * 3 + 0.5).cuda()
    pw = (torch.rand(C, generator=g) * 4 + 0.5).cuda()
    return x, W, b, y, wgt, pw


def _head_run(mode, x, W, b, y, wgt, pw):
    from fmda_amd.ops.interface import fused_head_loss
    x = x.clone().requires_grad_(True)
    W = W.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    with glue(mode):
        loss, logits = fused_head_loss(x, W, b, y, wgt, pw)
        loss.backward()
    return loss.detach(), logits.detach(), x.grad, W.grad, b.grad


@DTYPES
@pytest.mark.parametrize("K", [24, 384])
@pytest.mark.parametrize("B", [1, 37, 300])
def test_head_master_path(B, K, dtype):
    """B = 1 / 37 / 300 is 1, 1 and 5 slabs of the dW reduction and 1, 1 and
    5 blocks of loss partials."""
    x, W, b, y, wgt, pw = _head_inputs(B, K, dtype)
    loss0, logits0, dx0, dW0, db0 = _head_run(0, x, W, b, y, wgt, pw)
    # default mode: the whole step equals the eager one
    for a, r in zip(_head_run(1, x, W, b, y, wgt, pw),
                    (loss0, logits0, dx0, dW0, db0)):
        assert a.dtype == r.dtype and torch.equal(a, r)
    # mode 2: same forward and dx, fp32 dW / db from head_wgrads
    loss1, logits1, dx1, dW1, db1 = _head_run(2, x, W, b, y, wgt, pw)
    assert torch.equal(loss1, loss0)
    assert torch.equal(logits1, logits0)
    assert torch.equal(dx1, dx0)
    assert dW1.dtype == FP32 and db1.dtype == FP32
    assert dW1.shape == W.shape and db1.shape == b.shape

    # fp64 truth from the values both paths read: the fp32 dlogits of the
    # backward kernel, rounded to the compute dtype for dW only
    sig = _ext().head_loss_fwd(x, W.to(dtype), b.to(dtype), y, wgt, pw)[1]
    dlogits = _ext().head_loss_bwd(sig, y, wgt, pw,
                                   torch.ones(1, device="cuda"),
                                   W.to(dtype), dtype)[0]
    dW_ref = dlogits.to(dtype).double().t() @ x.double()
    db_ref = dlogits.double().sum(dim=0)
    for name, new, old, ref in [("dW", dW1, dW0, dW_ref),
                                ("db", db1, db0, db_ref)]:
        e_new = float((new.double() - ref).abs().max())
        e_old = float((old.double() - ref).abs().max())
        print(f"head {name} B={B} K={K} {dtype}: max err native {e_new:.3e} "
              f"eager {e_old:.3e}")
        assert e_new <= e_old, (name, e_new, e_old)


# ---------------------------------------------------------------------------
# pooling in the activation dtype
# ---------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("pitched", [False, True], ids=["dense", "pitched"])
@pytest.mark.parametrize("H", [8, 128])
@pytest.mark.parametrize("B", [1, 37])
def test_dirsum_pool_activation_dtype_equals_eager_casts(B, H, pitched,
                                                         dtype):
    """pitched: the grads arrive as column slices of a (B, 3H) feature
    gradient, as in the model, and the native path reads them in place."""
    from fmda_amd.ops.interface import dirsum_pool
    T = 5
    g = torch.Generator().manual_seed(B + H)
    out = (torch.randn(B, T, 2 * H, generator=g) * 2).to(dtype).cuda()
    gfeat = torch.randn(B, 3 * H, generator=g).to(dtype).cuda()
    res = []
    for mode in (0, 1):
        o = out.clone().requires_grad_(True)
        with glue(mode):
            mx, av = dirsum_pool(o, 2)
            if pitched:
                feat = torch.cat([mx.new_zeros(B, H), mx, av], dim=1)
                feat.backward(gfeat)
            else:
                torch.autograd.backward(
                    [mx, av], [gfeat[:, H:2 * H].contiguous(),
                               gfeat[:, 2 * H:].contiguous()])
        assert mx.dtype == dtype and av.dtype == dtype
        res.append((mx.detach(), av.detach(), o.grad))
    for a, r in zip(res[1], res[0]):
        assert torch.equal(a, r)


# ---------------------------------------------------------------------------
# one biGRU layer node, native against eager glue
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("drop_p", [0.0, 0.5], ids=["nodrop", "drop"])
def test_bigru_layer_native_glue_against_eager(drop_p, monkeypatch):
    from fmda_amd.ops import interface as itf
    B, T, H, F, D = 37, 5, 128, 96, 2
    Hp = itf._pad_h(H)
    seed = 20240607
    masters = _gru_masters(H, F, D, seed=9)
    g = torch.Generator().manual_seed(17)
    x0 = (torch.randn(B, T, F, generator=g) * 0.5).bfloat16().cuda()
    d_seq = torch.randn(B, T, D * H, generator=g).bfloat16().cuda()
    d_hl = torch.randn(D, B, Hp, generator=g).cuda()

    # record the split-K partials the native path hands to the kernel
    seen = []
    real_parts = itf.chunked_outer_parts

    def recording_parts(dg, xx, chunks=64):
        p = real_parts(dg, xx, chunks)
        seen.append(p)
        return p
    monkeypatch.setattr(itf, "chunked_outer_parts", recording_parts)

    def run(mode):
        x = x0.clone().requires_grad_(True)
        ps = [t.clone().requires_grad_(True) for four in masters
              for t in four]
        with glue(mode):
            res = itf._BiGRULayer.apply(x, Hp, *ps, drop_p, seed, None)
            # with fused dropout the sequence output that feeds the next
            # layer is the dropped copy; the raw one gets no gradient
            seq = res[2] if drop_p > 0 else res[0]
            torch.autograd.backward([seq, res[1]], [d_seq, d_hl])
        return [r.detach() for r in res], x.grad, [p.grad for p in ps]

    res0, dx0, g0 = run(0)
    # default mode: native pack (and wt), eager reductions: all equal
    res_d, dx_d, g_d = run(1)
    assert not seen
    for a, r in zip(res_d + [dx_d] + g_d, res0 + [dx0] + g0):
        assert a.dtype == r.dtype and torch.equal(a, r)
    # mode 2: finalize_gru_wgrads sums the partials in its own order
    res1, dx1, g1 = run(2)
    part_ih, part_hh = seen
    c = part_ih.shape[0]
    assert len(res1) == len(res0) == (3 if drop_p > 0 else 2)
    for a, r in zip(res1, res0):
        assert torch.equal(a, r)
    # dx and the bias grads run the same kernels on the same inputs
    assert torch.equal(dx1, dx0)
    for d in range(D):
        rows = slice(d * 3 * Hp, (d + 1) * 3 * Hp)
        w_ih1, w_hh1, b_ih1, b_hh1 = g1[4 * d:4 * d + 4]
        w_ih0, w_hh0, b_ih0, b_hh0 = g0[4 * d:4 * d + 4]
        assert torch.equal(b_ih1, b_ih0) and torch.equal(b_hh1, b_hh0)
        mag_ih = part_ih[:, rows].double().abs().sum(dim=0)
        mag_hh = part_hh[:, rows, d * Hp:(d + 1) * Hp].double().abs().sum(0)
        for name, a, r, mag in [("w_ih", w_ih1, w_ih0, mag_ih),
                                ("w_hh", w_hh1, w_hh0, mag_hh)]:
            assert a.dtype == FP32 and a.is_contiguous() and a.shape == r.shape
            err = (a.double() - r.double()).abs()
            assert (err <= c * 2.0 ** -23 * mag).all(), (
                name, d, float(err.max()))
