"""The exact step-glue kernels of the default mode (FMDA_NATIVE_GLUE=1)
against the eager chains they replace, which stay reachable with
FMDA_NATIVE_GLUE=0 or a binding flag:

  finalize_gru_wgrads(eager_order=True)  split-K partials -> the four
      master-shaped grads, summed in the order of parts.float().sum(dim=0)
  head_wgrads_eager + the cast emitted by head_loss_bwd_master
  head_loss_fwd_master(staged=True)      operands read through LDS
  subset_accuracy                        one kernel for the metric

Every comparison is bitwise. Sums of same-magnitude values almost never
show the order they were made in, so the reduction inputs are scaled by
2^U{-12..12} element by element: on such data the ascending order and
torch's order differ in most outputs.
"""
import contextlib
import os

import numpy as np
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
    old = os.environ.get("FMDA_NATIVE_GLUE")
    os.environ["FMDA_NATIVE_GLUE"] = str(int(mode))
    try:
        yield
    finally:
        if old is None:
            del os.environ["FMDA_NATIVE_GLUE"]
        else:
            os.environ["FMDA_NATIVE_GLUE"] = old


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal as bit patterns (-0.0 != 0.0, NaN == the same NaN)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = {FP32: torch.int32, BF16: torch.int16}[a.dtype]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _scaled_randn(shape, gen, dtype):
    """randn * 2^U{-12..12}, rounded to dtype: order-sensitive sums."""
    e = torch.randint(-12, 13, shape, generator=gen, device=gen.device)
    v = torch.randn(shape, generator=gen, device=gen.device)
    return (v * torch.exp2(e.float())).to(dtype)


def _spy(monkeypatch, name):
    """Count the calls of one extension function (and keep its kwargs)."""
    ext = _ext()
    real = getattr(ext, name)
    calls = []

    def wrapper(*args, **kwargs):
        calls.append(args)
        return real(*args, **kwargs)
    monkeypatch.setattr(ext, name, wrapper)
    return calls


# ---------------------------------------------------------------------------
# 1. GRU weight-grad finalisation in the eager sum's order
# ---------------------------------------------------------------------------

def _eager_gru_wgrads(part_ih, part_hh, D, H, Hp):
    """The eager lines of _BiGRULayer.backward on given partials."""
    from fmda_amd.ops.interface import _unpad_gate_rows
    cross = part_hh.float().sum(dim=0)
    dwih_cat = part_ih.float().sum(dim=0)
    out = []
    for d in range(D):
        dwih = dwih_cat[d * 3 * Hp:(d + 1) * 3 * Hp]
        dwhh = cross[d * 3 * Hp:(d + 1) * 3 * Hp,
                     d * Hp:(d + 1) * Hp].contiguous()
        out += [_unpad_gate_rows(dwih, H, Hp),
                _unpad_gate_rows(dwhh, H, Hp)[:, :H]]
    return out


def _gru_partials(c, D, Hp, F, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    part_ih = _scaled_randn((c, D * 3 * Hp, F), g, dtype)
    part_hh = _scaled_randn((c, D * 3 * Hp, D * Hp), g, dtype)
    if D == 2:
        # the off-diagonal direction blocks must never be read
        for d in range(2):
            part_hh[:, d * 3 * Hp:(d + 1) * 3 * Hp,
                    (1 - d) * Hp:(2 - d) * Hp] = float("nan")
    return part_ih, part_hh


@DTYPES
@pytest.mark.parametrize("F", [8, 96])
@pytest.mark.parametrize("H,Hp", [(32, 32), (24, 32), (128, 128), (25, 32)])
@pytest.mark.parametrize("D", [1, 2])
def test_finalize_gru_wgrads_eager_order(D, H, Hp, F, dtype):
    """(25, 32) has rows that are no whole 4-vectors: the scalar kernel."""
    ext = _ext()
    part_ih, part_hh = _gru_partials(64, D, Hp, F, dtype,
                                     seed=1000 * D + 10 * H + F)
    assert ext.eager_sum_applies(part_ih) and ext.eager_sum_applies(part_hh)
    ref = _eager_gru_wgrads(part_ih, part_hh, D, H, Hp)
    got = ext.finalize_gru_wgrads(part_ih, part_hh, D, H, Hp, True)
    again = ext.finalize_gru_wgrads(part_ih, part_hh, D, H, Hp, True)
    assert len(got) == 2 * D
    n_diff_ascending = 0
    asc = ext.finalize_gru_wgrads(part_ih, part_hh, D, H, Hp)
    for a, b, r, s in zip(got, again, ref, asc):
        assert a.dtype == FP32 and a.is_contiguous()
        assert _bits_equal(a, r), float((a - r).abs().max())
        assert _bits_equal(a, b)
        n_diff_ascending += int((s != r).sum())
    # the data tells the orders apart: the ascending sum of mode 2 differs
    assert n_diff_ascending > 0


def test_finalize_gru_wgrads_eager_order_v1_odd_f():
    """F = 5: odd rows, scalar kernel; D = 2 keeps >= 512 outputs."""
    ext = _ext()
    D, H, Hp, F = 2, 25, 32, 5
    part_ih, part_hh = _gru_partials(64, D, Hp, F, BF16, seed=77)
    ref = _eager_gru_wgrads(part_ih, part_hh, D, H, Hp)
    got = ext.finalize_gru_wgrads(part_ih, part_hh, D, H, Hp, True)
    for a, r in zip(got, ref):
        assert _bits_equal(a, r)


def test_eager_order_is_refused_where_it_is_not_derived():
    """32 chunks, or fewer than 512 outputs, are not the 64 x 2 block."""
    from fmda_amd.ops.interface import _eager_sum_known
    ext = _ext()
    p32 = torch.zeros(32, 96, 8, device="cuda", dtype=BF16)
    small = torch.zeros(64, 96, 4, device="cuda", dtype=BF16)     # 384
    odd = torch.zeros(64, 171, 3, device="cuda", dtype=BF16)      # 513
    ok = torch.zeros(64, 96, 8, device="cuda", dtype=BF16)
    assert ext.eager_sum_applies(ok)
    for p in (p32, small, odd):
        assert not ext.eager_sum_applies(p)
    hh = torch.zeros(64, 96, 32, device="cuda", dtype=BF16)
    with pytest.raises(RuntimeError):
        ext.finalize_gru_wgrads(small, hh, 1, 32, 32, True)
    assert _eager_sum_known(320, 768) and _eager_sum_known(64, 512)
    assert not _eager_sum_known(96, 768)      # c = 32
    assert not _eager_sum_known(185, 768)     # c = 1
    assert not _eager_sum_known(320, 384)
    assert not _eager_sum_known(320, 514)


def _layer_run(mode, B, T, H, F, D, seed):
    from fmda_amd.ops import interface as itf
    Hp = itf._pad_h(H)
    g = torch.Generator().manual_seed(seed)
    masters = [(torch.randn(*shape, generator=g) * 0.3).cuda()
               .requires_grad_(True)
               for _ in range(D)
               for shape in [(3 * H, F), (3 * H, H), (3 * H,), (3 * H,)]]
    x = (torch.randn(B, T, F, generator=g) * 0.5).bfloat16().cuda()
    d_seq = _scaled_randn((B, T, D * Hp), g, BF16).cuda()
    d_hl = torch.randn(D, B, Hp, generator=g).cuda()
    x.requires_grad_(True)
    pad = masters + [None] * (8 - len(masters))
    with glue(mode):
        res = itf._BiGRULayer.apply(x, Hp, *pad, 0.0, 0, None)
        torch.autograd.backward([res[0], res[1]], [d_seq, d_hl])
    return [x.grad] + [p.grad for p in masters]


@pytest.mark.parametrize("B,T,H,F,D,native", [
    (64, 5, 32, 8, 2, True),      # M = 320: c = 64
    (32, 3, 32, 8, 1, False),     # M = 96: c = 32, eager
    (64, 2, 8, 4, 1, False),      # 384 dW_ih outputs, eager
    (37, 5, 32, 8, 2, False),     # ragged M: c = 1, eager
])
def test_bigru_layer_default_mode_equals_eager(B, T, H, F, D, native,
                                               monkeypatch):
    calls = _spy(monkeypatch, "finalize_gru_wgrads")
    ref = _layer_run(0, B, T, H, F, D, seed=5)
    assert not calls
    got = _layer_run(1, B, T, H, F, D, seed=5)
    assert len(calls) == (1 if native else 0)
    for a, r in zip(got, ref):
        assert a.is_contiguous() or not native
        assert _bits_equal(a, r)


# ---------------------------------------------------------------------------
# 2. head weight grads
# ---------------------------------------------------------------------------

def _head_inputs(B, K, C, dtype, scaled):
    g = torch.Generator().manual_seed(1000 + B + K + C)
    if scaled:
        x = _scaled_randn((B, K), g, dtype).cuda()
    else:
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
@pytest.mark.parametrize("B", [64, 320, 2048])
def test_head_wgrads_equal_eager(B, K, dtype, monkeypatch):
    """All three B split into 64 chunks; C*K = 96 (K = 24) is below the 512
    outputs the order is derived for and stays eager. x is scaled, so the
    64 partials of an output span 24 binades; three B x 1536 outputs per
    dtype are compared, and fp32 has no final rounding to hide behind."""
    C = 4
    calls = _spy(monkeypatch, "head_wgrads_eager")
    x, W, b, y, wgt, pw = _head_inputs(B, K, C, dtype, scaled=True)
    ref = _head_run(0, x, W, b, y, wgt, pw)
    assert not calls
    got = _head_run(1, x, W, b, y, wgt, pw)
    assert len(calls) == (1 if K == 384 else 0)
    for name, a, r in zip(["loss", "logits", "dx", "dW", "db"], got, ref):
        assert _bits_equal(a, r), name
    assert got[3].dtype == FP32 and got[4].dtype == FP32


@DTYPES
def test_head_bwd_emits_the_cast_of_dlogits(dtype):
    B, K, C = 300, 24, 4
    ext = _ext()
    x, W, b, y, wgt, pw = _head_inputs(B, K, C, dtype, scaled=False)
    sig = ext.head_loss_fwd_master(x, W, b, y, wgt, pw)[1]
    one = torch.ones(1, device="cuda")
    dlogits, dx = ext.head_loss_bwd_master(sig, y, wgt, pw, one, W, dtype)
    dlogits2, dx2, dl = ext.head_loss_bwd_master(sig, y, wgt, pw, one, W,
                                                 dtype, True)
    assert _bits_equal(dlogits2, dlogits) and _bits_equal(dx2, dx)
    assert dl.dtype == dtype and _bits_equal(dl, dlogits.to(dtype))


# ---------------------------------------------------------------------------
# 3. head forward through LDS
# ---------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("K", [24, 384, 1536])
@pytest.mark.parametrize("B", [1, 37, 300])
def test_head_fwd_staged_equals_direct(B, K, C, dtype):
    """B = 300, C = 4 is 5 blocks, the last one partly filled; C = 1 puts
    256 rows into a block, K = 1536 needs several column tiles."""
    ext = _ext()
    x, W, b, y, wgt, pw = _head_inputs(B, K, C, dtype, scaled=False)
    ref = ext.head_loss_fwd_master(x, W, b, y, wgt, pw, staged=False)
    got = ext.head_loss_fwd_master(x, W, b, y, wgt, pw, staged=True)
    assert len(got) == len(ref) == 4
    for name, a, r in zip(["logits", "sig", "loss_sum", "partials"], got,
                          ref):
        assert _bits_equal(a, r), name
    assert got[3].numel() == (B * C + 255) // 256


# ---------------------------------------------------------------------------
# 4. subset_accuracy
# ---------------------------------------------------------------------------

def _differing_counts(n):
    """Counts k <= n where k * fp32(1/n) != fp32(k / n) in fp32."""
    k = np.arange(n + 1, dtype=np.float32)
    inv = np.float32(1.0) / np.float32(n)
    return np.nonzero(k * inv != k / np.float32(n))[0].tolist()


def test_differing_counts_table():
    assert _differing_counts(7) == [3, 6]
    assert len(_differing_counts(37)) == 12
    assert len(_differing_counts(1000)) == 584
    d = _differing_counts(8191)
    assert len(d) == 1024 and d[0] == 2049
    assert _differing_counts(8192) == []


def _accuracy_cases():
    cases = []
    for B in (1, 7, 37, 1000, 8191):
        counts = {0, B}
        diff = _differing_counts(B)
        counts.update(diff[:2] + diff[-1:])
        for C in (1, 4):
            for k in sorted(counts):
                cases.append((B, C, k))
    return cases


@pytest.mark.parametrize("target_dtype", [FP32, torch.bool],
                         ids=["float", "bool"])
@pytest.mark.parametrize("B,C,right", _accuracy_cases())
def test_subset_accuracy_equals_eager(B, C, right, target_dtype):
    """`right` rows match in every label, the others differ in one."""
    from fmda_amd.metrics import subset_accuracy
    g = torch.Generator().manual_seed(B * 10 + C)
    pred = torch.rand(B, C, generator=g) < 0.5
    target = pred.clone()
    wrong = torch.randperm(B, generator=g)[:B - right]
    col = torch.randint(0, C, (B - right,), generator=g)
    target[wrong, col] = ~target[wrong, col]
    if target_dtype == FP32:
        # any non-zero value is a set label
        target = target.float() * (torch.rand(B, C, generator=g) * 4 - 2.5)
    target, pred = target.cuda(), pred.cuda()
    with glue(0):
        ref = subset_accuracy(target, pred)
    got = subset_accuracy(target, pred)
    assert got.dim() == 0 and got.dtype == FP32
    assert _bits_equal(got, ref), (float(got), float(ref))
    assert abs(float(got) - right / B) < 1e-6


def test_subset_accuracy_kernel_is_used_and_other_layouts_are_eager(
        monkeypatch):
    from fmda_amd.metrics import subset_accuracy
    calls = _spy(monkeypatch, "subset_accuracy")
    g = torch.Generator().manual_seed(3)
    pred = (torch.rand(37, 4, generator=g) < 0.5).cuda()
    target = (torch.rand(37, 4, generator=g) < 0.5).float().cuda()
    ref = (target.bool() == pred).all(dim=1).float().mean()
    assert _bits_equal(subset_accuracy(target, pred), ref)
    assert len(calls) == 1
    # transposed storage, a float pred, CPU tensors: the expression itself
    tt, pt = target.t().contiguous().t(), pred.t().contiguous().t()
    assert _bits_equal(subset_accuracy(tt, pt), ref)
    assert _bits_equal(subset_accuracy(target, pred.float()), ref)
    tc, pc = target.cpu(), pred.cpu()
    assert torch.equal(subset_accuracy(tc, pc),
                       (tc.bool() == pc).all(dim=1).float().mean())
    with glue(0):
        assert _bits_equal(subset_accuracy(target, pred), ref)
    assert len(calls) == 1


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------

def _model_step(mode, B):
    from fmda_amd.models import BiGRU
    from fmda_amd.ops.interface import fused_head_loss
    torch.manual_seed(11)
    model = BiGRU(128, 96, 4, n_layers=2, dropout=0.1).cuda().train()
    g = torch.Generator().manual_seed(B)
    x = (torch.randn(B, 5, 96, generator=g) * 0.5).bfloat16().cuda()
    y = (torch.rand(B, 4, generator=g) < 0.3).float().cuda()
    wgt = (torch.rand(4, generator=g) * 3 + 0.5).cuda()
    pw = (torch.rand(4, generator=g) * 4 + 0.5).cuda()
    torch.manual_seed(12)            # the dropout seeds come from here
    with glue(mode):
        feats = model.forward_features(x)
        loss, logits = fused_head_loss(feats, model.linear.weight,
                                       model.linear.bias, y, wgt, pw)
        loss.backward()
    grads = [p.grad for _, p in sorted(model.named_parameters())]
    return [loss.detach(), logits.detach()] + grads


@pytest.mark.parametrize("B,native", [(64, True), (37, False)])
def test_model_step_default_mode_equals_eager(B, native, monkeypatch):
    """L2/H128/T5. B = 64: M = 320 rows split into 64 chunks, both layers'
    grads and the head's come from the new kernels. B = 37: one chunk,
    everything eager."""
    gru = _spy(monkeypatch, "finalize_gru_wgrads")
    head = _spy(monkeypatch, "head_wgrads_eager")
    ref = _model_step(0, B)
    assert not gru and not head
    got = _model_step(1, B)
    assert len(gru) == (2 if native else 0)
    assert len(head) == (1 if native else 0)
    assert len(got) == len(ref) == 2 + 18
    for i, (a, r) in enumerate(zip(got, ref)):
        assert a is not None and _bits_equal(a, r), i
