"""pool_features_fwd / pool_features_bwd (the pooled-head feature path in one
HIP kernel each way) against the path they replace: the h_n cast, the
direction sum of the last hidden state, dirsum_pool, torch.cat, and the
autograd of that chain. Every comparison is torch.equal.

Two references are used. `_existing_path` is the literal chain with
dirsum_pool. For grids below 4096 column pairs dirsum_pool's launcher picks
its wave-per-pair kernel, which adds the T values in a lane-butterfly order;
that is the thread-per-column order (ascending t) only up to T = 3. The new
kernel is specified against the thread-per-column kernel, so the avg columns
of a small grid with T > 3 are compared with `_octet_path` instead: the
same chain with pool_fwd(serial=True), which runs that kernel at any grid
size. Everything else (last hidden, max, amax, d_out, d_hlast) does not
depend on the summation order and is compared with both. B = 1024 gives
grids of at least 4096 pairs, where the literal chain itself runs the
thread-per-column kernel. The model uses the new path only from that grid
size on, so a training step computes what it computed before at every
batch size.
"""
import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
SMALL_GRID = 4096   # fmda_pool_fwd_launch: pairs below this -> wave kernel


def _ext():
    from fmda_amd.ops import load_extension
    return load_extension()


@contextlib.contextmanager
def glue(mode: int):
    old = os.environ.get("FMDA_NATIVE_GLUE")
    os.environ["FMDA_NATIVE_GLUE"] = str(int(mode))
    try:
        yield
    finally:
        if old is None:
            del os.environ["FMDA_NATIVE_GLUE"]
        else:
            os.environ["FMDA_NATIVE_GLUE"] = old


def _inputs(B, T, H, D, case, seed):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(B, T, D * H, generator=g)
    if case == "const":
        # every comparison over t ties: the first t must win
        out = out[:, :1].expand(B, T, D * H).contiguous()
    elif case == "max_first":
        out[:, 0] = 16.0
    elif case == "max_last":
        out[:, T - 1] = 16.0
    h_last = torch.randn(D, B, H, generator=g) * 3
    big = torch.randn(B, 3 * H + 5, generator=g)
    return (out.to(BF16).cuda(), h_last.cuda(), big.to(BF16).cuda())


def _last_hidden_chain(h_last, D, B, H):
    """bigru_stack's h_n (with a lower layer in front of the top one) and
    _pool_concat's direction sum of its last layer."""
    hl = h_last.clone().requires_grad_(True)
    lower = torch.zeros(D, B, H, dtype=BF16, device=hl.device)
    h_n = torch.cat([lower, hl[:, :, :H].to(BF16)], dim=0)
    last = h_n.view(2, D, B, H)[-1].sum(dim=0)
    return hl, last


def _existing_path(out, h_last, dfeat, D):
    from fmda_amd.ops.interface import dirsum_pool
    B, T, DH = out.shape
    H = DH // D
    o = out.clone().requires_grad_(True)
    hl, last = _last_hidden_chain(h_last, D, B, H)
    mx, av = dirsum_pool(o, D)
    feat = torch.cat([last, mx, av], dim=1)
    feat.backward(dfeat)
    return feat.detach(), o.grad, hl.grad


def _octet_path(out, h_last, dfeat, D):
    B, T, DH = out.shape
    H = DH // D
    hl, last = _last_hidden_chain(h_last, D, B, H)
    mx, av, amax = _ext().pool_fwd(out, D, True, serial=True)
    feat = torch.cat([last, mx, av], dim=1)
    last.backward(dfeat[:, :H])
    d_out = _ext().pool_bwd(dfeat[:, H:2 * H], dfeat[:, 2 * H:], amax, T, D,
                            BF16)
    return feat.detach(), amax, d_out, hl.grad


@pytest.mark.parametrize("case", ["random", "const", "max_first", "max_last"])
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("H", [8, 128])
# the load loop takes 8 timesteps at a time: below, equal, not a multiple
@pytest.mark.parametrize("T", [1, 2, 3, 7, 8, 19])
@pytest.mark.parametrize("B", [2, 37, 1024])
def test_pool_features_kernels_equal_existing_path(B, T, H, D, case):
    ext = _ext()
    with glue(1):
        out, h_last, big = _inputs(B, T, H, D, case,
                                   seed=B + 10 * T + H + 1000 * D)
        feat, amax = ext.pool_features_fwd(out, h_last)
        assert feat.dtype == BF16 and feat.shape == (B, 3 * H)
        assert amax.dtype == torch.int32 and amax.shape == (B, H)
        if case in ("const", "max_first"):
            assert not amax.any()
        elif case == "max_last":
            assert (amax == T - 1).all()
        same_order = T <= 3 or B * (H // 2) >= SMALL_GRID
        for name, dfeat in [("dense", big[:, 3:3 + 3 * H].contiguous()),
                            ("pitched", big[:, 3:3 + 3 * H])]:
            d_out, d_hlast = ext.pool_features_bwd(dfeat, amax, T, D)
            assert d_out.dtype == BF16 and d_out.shape == out.shape, name
            assert d_hlast.dtype == FP32 and d_hlast.shape == (D, B, H), name
            assert torch.equal(d_hlast, dfeat[:, :H].float().expand(D, B, H))

            r_feat, r_amax, r_dout, r_dhl = _octet_path(out, h_last, dfeat, D)
            assert torch.equal(amax, r_amax), name
            assert torch.equal(feat, r_feat), name
            assert torch.equal(d_out, r_dout), name
            assert torch.equal(d_hlast, r_dhl), name

            e_feat, e_dout, e_dhl = _existing_path(out, h_last, dfeat, D)
            cols = 3 * H if same_order else 2 * H
            assert torch.equal(feat[:, :cols], e_feat[:, :cols]), name
            assert torch.equal(d_out, e_dout), name
            assert torch.equal(d_hlast, e_dhl), name


def test_pooled_features_autograd_function():
    """_PooledFeatures end to end on a grid the model gives it, dense and
    pitched incoming gradient, against the literal chain."""
    from fmda_amd.ops.interface import pooled_features
    B, T, H, D = 64, 7, 128, 2
    out, h_last, big = _inputs(B, T, H, D, "random", seed=5)
    for dfeat in (big[:, 3:3 + 3 * H].contiguous(), big[:, 3:3 + 3 * H]):
        o = out.clone().requires_grad_(True)
        hl = h_last.clone().requires_grad_(True)
        with glue(1):
            feat = pooled_features(o, hl)
            feat.backward(dfeat)
            e_feat, e_dout, e_dhl = _existing_path(out, h_last, dfeat, D)
        assert torch.equal(feat.detach(), e_feat)
        assert torch.equal(o.grad, e_dout)
        assert hl.grad.dtype == FP32 and torch.equal(hl.grad, e_dhl)


def _train_step(mode, B, H=128, dtype=BF16, T=5, F=96):
    from fmda_amd.models import BiGRU
    from fmda_amd.ops.interface import fused_head_loss
    torch.manual_seed(11)
    model = BiGRU(H, F, 4, n_layers=2, dropout=0.5,
                  spatial_dropout=False).cuda()
    model.train()
    g = torch.Generator().manual_seed(B + H)
    x = (torch.randn(B, T, F, generator=g) * 0.5).to(dtype).cuda()
    y = (torch.rand(B, 4, generator=g) < 0.3).float().cuda()
    wgt = torch.tensor([4.0, 6.0, 4.0, 6.0]).cuda()
    pw = torch.tensor([3.0, 5.0, 3.0, 5.0]).cuda()
    torch.manual_seed(77)   # the dropout seeds come from the global RNG
    with glue(mode):
        feats = model.forward_features(x)
        loss, logits = fused_head_loss(feats, model.linear.weight,
                                       model.linear.bias, y, wgt, pw)
        loss.backward()
    grads = {n: p.grad for n, p in model.named_parameters()}
    return feats, loss.detach(), logits.detach(), grads


# B = 37: below the grid size from which the model uses the new path (the
# eager chain stays, with its summation order); B = 64: the new path
@pytest.mark.parametrize("B,native", [(37, False), (64, True)])
def test_forward_features_step_equals_eager_glue(B, native):
    f1, loss1, logits1, g1 = _train_step(1, B)
    f0, loss0, logits0, g0 = _train_step(0, B)
    assert (type(f1.grad_fn).__name__ == "_PooledFeaturesBackward") == native
    assert type(f0.grad_fn).__name__ != "_PooledFeaturesBackward"
    assert torch.equal(f1, f0)
    assert torch.equal(loss1, loss0) and torch.equal(logits1, logits0)
    assert g1.keys() == g0.keys() and len(g1) == 18
    for name in g0:
        assert g1[name] is not None, name
        assert g1[name].dtype == g0[name].dtype, name
        assert torch.equal(g1[name], g0[name]), name


@pytest.mark.parametrize("H,dtype", [(7, BF16), (104, BF16), (128, FP32)],
                         ids=["oddH", "paddedH", "fp32"])
def test_fallback_cases_still_run(H, dtype):
    """Odd H, H below its padded size and fp32 activations keep the eager
    feature path."""
    feats, loss, logits, grads = _train_step(1, 64, H=H, dtype=dtype, T=3,
                                             F=12)
    assert type(feats.grad_fn).__name__ != "_PooledFeaturesBackward"
    assert feats.shape == (64, 3 * H) and feats.dtype == dtype
    assert torch.isfinite(loss) and torch.isfinite(logits).all()
    for name, gr in grads.items():
        assert gr is not None and torch.isfinite(gr).all(), name
