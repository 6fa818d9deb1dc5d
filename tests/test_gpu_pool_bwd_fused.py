"""The top layer's BPTT kernel building d_out / d_hlast from the pooled
head's (dfeat, amax) itself (gru_bwd(dfeat=, amax=), the fused _PooledFeatures)
against the two-kernel path it replaces: pool_features_bwd writes the dense
(B, T, D*H) d_out and gru_bwd reads it back. FMDA_FUSED_POOL_BWD=0 keeps
that path reachable at model level.

Every comparison is bitwise. The kernel changes no arithmetic, it only picks
one of two precomputed bf16 values per (row, column, step), so anything but
equal bits is a wrong table entry, a wrong owner slot or a wrong step.
"""
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
H = 128


def _ext():
    from fmda_amd.ops import load_extension
    return load_extension()


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal as bit patterns (-0.0 != 0.0, NaN == the same NaN)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = {FP32: torch.int32, BF16: torch.int16}[a.dtype]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


# ---------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------

BMAX = 70     # 1: lone tail block, 31: tail, 32: full, 33: full + tail, 70: 3
BATCHES = [1, 31, 32, 33, 70]


@functools.lru_cache(maxsize=None)
def _weights(D):
    g = torch.Generator().manual_seed(100 + D)
    w = (torch.randn(D, 3 * H, H, generator=g) * 0.1).to(BF16).cuda()
    bhh = (torch.randn(D, 3 * H, generator=g) * 0.1).cuda()
    return w, bhh


@functools.lru_cache(maxsize=None)
def _case(D, T, B=BMAX):
    """Inputs of one (D, T): the first rows of it serve every batch size."""
    g = torch.Generator().manual_seed(1000 * D + T)
    gi = (torch.randn(B, T, D * 3 * H, generator=g) * 0.5).to(BF16).cuda()
    out = torch.tanh(torch.randn(B, T, D * H, generator=g)).to(BF16).cuda()
    h0 = (torch.randn(D, B, H, generator=g) * 0.5).cuda()
    # randn * 2^U{-12..12}: v0 and v1 round differently all over the range
    e = torch.randint(-12, 13, (B, 3 * H), generator=g)
    dfeat = (torch.randn(B, 3 * H, generator=g) * torch.exp2(e.float()))
    # average-pool gradients of -0.0 and +0.0: d_out is +0.0 off the argmax
    # either way, and -0.0 at the argmax only where the max gradient is -0.0
    dfeat[:, 2 * H + 3] = -0.0
    dfeat[:, 2 * H + 4] = 0.0
    dfeat[:, 2 * H + 5] = -0.0
    dfeat[:, H + 5] = -0.0
    dfeat[:, 2 * H + 6] = 0.0
    dfeat[:, H + 6] = -0.0
    dfeat = dfeat.to(BF16).cuda()
    # argmax: varies per row and column, hits t = 0 and t = T - 1
    b = torch.arange(B)[:, None]
    j = torch.arange(H)[None, :]
    amax = ((3 * b + 5 * j + (b * j) // 7) % T).int()
    amax[:, 0] = 0
    amax[:, 1] = T - 1
    amax[:, 5] = T - 1
    amax[:, 127] = (b[:, 0] % 2) * (T - 1)
    return gi, out, h0, dfeat, amax.cuda()


def _both_ways(D, T, B, use_h0, dfeat=None):
    """(dense results, pooled results) of gru_bwd on the first B rows."""
    ext = _ext()
    w, bhh = _weights(D)
    gi, out, h0, df, amax = _case(D, T, max(B, BMAX) if T != 256 else B)
    gi, out, amax = gi[:B].contiguous(), out[:B].contiguous(), amax[:B].contiguous()
    h0 = h0[:, :B].contiguous() if use_h0 else None
    dfeat = df[:B].contiguous() if dfeat is None else dfeat
    d_out, d_hlast = ext.pool_features_bwd(dfeat, amax, T, D)
    dense = ext.gru_bwd(gi, w, bhh, out, d_out, d_hlast, 0.0, 0, h0, None)
    pooled = ext.gru_bwd(gi, w, bhh, out, None, None, 0.0, 0, h0, None,
                         dfeat, amax)
    return dense, pooled


NAMES = ["dgi", "dgh", "dh0", "dbhh", "dbih", "dgh0"]


def _assert_same(dense, pooled, use_h0, tag):
    assert len(dense) == len(pooled) == (6 if use_h0 else 5), tag
    for name, a, r in zip(NAMES, pooled, dense):
        assert _bits_equal(a, r), (tag, name)


@pytest.mark.parametrize("use_h0", [False, True], ids=["zero_h0", "h0"])
@pytest.mark.parametrize("T", [1, 2, 3, 7])
@pytest.mark.parametrize("D", [1, 2])
def test_pooled_gru_bwd_equals_dense(D, T, use_h0):
    for B in BATCHES:
        dense, pooled = _both_ways(D, T, B, use_h0)
        assert torch.isfinite(dense[0].float()).all()
        _assert_same(dense, pooled, use_h0, f"B={B}")


def test_pooled_gru_bwd_equals_dense_T256():
    """The longest sequence one amax byte holds: argmax values up to 255."""
    dense, pooled = _both_ways(2, 256, 33, False)
    assert int(_case(2, 256, 33)[4].max()) == 255
    _assert_same(dense, pooled, False, "T=256")


def test_pooled_gru_bwd_row_pitched_dfeat():
    """dfeat as a column slice of a wider buffer (ld = 3H + 16 > 3H)."""
    B, T, D = 33, 3, 2
    df = _case(D, T)[3][:B]
    wide = torch.full((B, 3 * H + 16), float("nan"), dtype=BF16,
                      device="cuda")
    wide[:, 8:8 + 3 * H] = df
    view = wide[:, 8:8 + 3 * H]
    assert view.stride() == (3 * H + 16, 1)
    dense, pooled = _both_ways(D, T, B, False, dfeat=view)
    _assert_same(dense, pooled, False, "pitched")
    ref, _ = _both_ways(D, T, B, False)
    _assert_same(ref, pooled, False, "pitched vs contiguous")


def test_pooled_gru_bwd_refusals():
    ext = _ext()

    def call(Hh, T, drop_p, B=4, D=2):
        g = torch.Generator().manual_seed(5)
        w = (torch.randn(D, 3 * Hh, Hh, generator=g) * 0.1).to(BF16).cuda()
        bhh = torch.zeros(D, 3 * Hh, device="cuda")
        gi = torch.zeros(B, T, D * 3 * Hh, dtype=BF16, device="cuda")
        out = torch.zeros(B, T, D * Hh, dtype=BF16, device="cuda")
        dfeat = torch.zeros(B, 3 * Hh, dtype=BF16, device="cuda")
        amax = torch.zeros(B, Hh, dtype=torch.int32, device="cuda")
        return ext.gru_bwd(gi, w, bhh, out, None, None, drop_p, 7, None,
                           None, dfeat, amax)

    assert len(call(128, 256, 0.0)) == 5          # the accepted neighbour
    with pytest.raises(RuntimeError, match="256"):
        call(128, 257, 0.0)
    with pytest.raises(RuntimeError, match="dropout"):
        call(128, 4, 0.25)
    with pytest.raises(RuntimeError, match="128"):
        call(64, 4, 0.0)
    with pytest.raises(RuntimeError, match="128"):
        call(256, 4, 0.0)
    # one gradient source: not half of one
    w, bhh = _weights(2)
    with pytest.raises(RuntimeError, match="either"):
        ext.gru_bwd(torch.zeros(4, 2, 768, dtype=BF16, device="cuda"),
                    w, bhh, torch.zeros(4, 2, 256, dtype=BF16, device="cuda"),
                    None, None, 0.0, 0, None, None,
                    torch.zeros(4, 384, dtype=BF16, device="cuda"), None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------

def _spy_bwd(monkeypatch):
    """Counts of gru_bwd calls by gradient source, and of pool_features_bwd."""
    ext = _ext()
    counts = {"pooled": 0, "dense": 0, "pool_bwd": 0}
    real_bwd, real_pool = ext.gru_bwd, ext.pool_features_bwd

    def gru_bwd(*args, **kwargs):
        fused = kwargs.get("dfeat") is not None or (
            len(args) > 10 and args[10] is not None)
        counts["pooled" if fused else "dense"] += 1
        return real_bwd(*args, **kwargs)

    def pool_bwd(*args, **kwargs):
        counts["pool_bwd"] += 1
        return real_pool(*args, **kwargs)
    monkeypatch.setattr(ext, "gru_bwd", gru_bwd)
    monkeypatch.setattr(ext, "pool_features_bwd", pool_bwd)
    return counts


def _model_step(B, T=5, hidden=128, layers=2, grad_view=False):
    from fmda_amd.models import BiGRU
    from fmda_amd.ops.interface import fused_head_loss
    torch.manual_seed(11)
    model = BiGRU(hidden, 96, 4, n_layers=layers, dropout=0.1).cuda().train()
    g = torch.Generator().manual_seed(B)
    x = (torch.randn(B, T, 96, generator=g) * 0.5).bfloat16().cuda()
    y = (torch.rand(B, 4, generator=g) < 0.3).float().cuda()
    wgt = (torch.rand(4, generator=g) * 3 + 0.5).cuda()
    pw = (torch.rand(4, generator=g) * 4 + 0.5).cuda()
    torch.manual_seed(12)            # the dropout seeds come from here
    feats = model.forward_features(x)
    if grad_view:
        # a feature gradient the kernel cannot load in 16-byte pieces
        # (row pitch 3H + 3): the node's fix-up copies it
        wide = (torch.randn(B, 3 * hidden + 3, generator=g)).bfloat16().cuda()
        feats.backward(wide[:, :3 * hidden])
        head = [feats.detach(), feats.detach()]
    else:
        loss, logits = fused_head_loss(feats, model.linear.weight,
                                       model.linear.bias, y, wgt, pw)
        loss.backward()
        head = [loss.detach(), logits.detach()]
    grads = [p.grad for _, p in sorted(model.named_parameters())]
    return head + grads


def _step_both(monkeypatch, counts, **kw):
    monkeypatch.setenv("FMDA_FUSED_POOL_BWD", "0")
    ref = _model_step(**kw)
    assert counts["pooled"] == 0
    for k in counts:
        counts[k] = 0
    monkeypatch.delenv("FMDA_FUSED_POOL_BWD")
    got = _model_step(**kw)
    assert len(got) == len(ref)
    for i, (a, r) in enumerate(zip(got, ref)):
        if a is None and r is None:      # the head's grads under grad_view
            continue
        assert a is not None and r is not None and _bits_equal(a, r), i
    return got


@pytest.mark.parametrize("B", [64, 70, 37])
def test_model_step_default_equals_two_nodes(B, monkeypatch):
    """L2 / H128 / T5: loss, logits and all 18 gradients. B = 64 and B = 70
    (two full 32-row blocks + a tail) take the fused node. B = 37 does not
    meet pooled_features_native (its grid goes to dirsum_pool's other
    summation order, so the eager pooling chain stays and so do its
    results): there the top layer's gru_bwd must stay dense."""
    from fmda_amd.ops.interface import pooled_features_native
    x = torch.empty(B, 5, 96, dtype=BF16, device="cuda")
    native = pooled_features_native(x, 128)
    assert native == (B >= 64)
    counts = _spy_bwd(monkeypatch)
    got = _step_both(monkeypatch, counts, B=B)
    assert len(got) == 2 + 18 and all(t is not None for t in got)
    if native:
        assert counts == {"pooled": 1, "dense": 1, "pool_bwd": 0}
    else:
        assert counts == {"pooled": 0, "dense": 2, "pool_bwd": 0}


def test_model_step_unusable_grad_pitch(monkeypatch):
    counts = _spy_bwd(monkeypatch)
    _step_both(monkeypatch, counts, B=64, grad_view=True)
    assert counts == {"pooled": 1, "dense": 1, "pool_bwd": 0}


@pytest.mark.parametrize("kw", [dict(B=64, T=257, layers=1),
                                dict(B=128, T=3, hidden=64, layers=1)],
                         ids=["T257", "H64"])
def test_model_step_outside_the_variant_runs_dense(kw, monkeypatch):
    """What the binding refuses never reaches it: the two nodes run."""
    counts = _spy_bwd(monkeypatch)
    _step_both(monkeypatch, counts, **kw)
    assert counts == {"pooled": 0, "dense": 1, "pool_bwd": 1}


def _window_model():
    from fmda_amd.models import BiGRU
    from fmda_amd.optim import FusedClipAdam
    torch.manual_seed(3)
    dev = torch.device("cuda")
    model = BiGRU(128, 12, 4, n_layers=2, dropout=0.5, clip=0.25).to(dev)
    model.add_loss_fn(nn.BCEWithLogitsLoss(
        weight=torch.tensor([1.0, 2.0, 0.5, 1.5], device=dev),
        pos_weight=torch.tensor([3.0, 1.0, 2.0, 0.75], device=dev)))
    model.add_optimizer(FusedClipAdam(model.parameters(), lr=1e-3,
                                      clip=model.clip))
    model.add_device(dev)
    return model


def test_train_windows_step_equals_two_nodes(monkeypatch):
    """One train_windows step: 70 windows of 8 rows in one batch."""
    g = torch.Generator().manual_seed(21)
    table = torch.rand(77, 12, generator=g).to(BF16).cuda()
    targets = (torch.rand(77, 4, generator=g) < 0.4).float().cuda()
    counts = _spy_bwd(monkeypatch)

    def run():
        model = _window_model()
        torch.manual_seed(17)
        _, _, losses, _ = model.train_windows(table, targets, 8, 70)
        assert len(losses) == 1
        return float(losses[0]), model.state_dict()

    monkeypatch.setenv("FMDA_FUSED_POOL_BWD", "0")
    loss_r, sd_r = run()
    assert counts == {"pooled": 0, "dense": 2, "pool_bwd": 1}
    monkeypatch.delenv("FMDA_FUSED_POOL_BWD")
    loss_g, sd_g = run()
    assert counts == {"pooled": 1, "dense": 3, "pool_bwd": 1}
    assert loss_g == loss_r
    fresh = _window_model().state_dict()
    for k in sd_r:
        assert torch.equal(sd_g[k], sd_r[k]), k
        if not k.startswith("loss_fn."):
            assert not torch.equal(sd_g[k], fresh[k]), k     # it did train
