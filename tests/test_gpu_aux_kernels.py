"""Oracle tests for the kernels around the recurrence: dropout, pooling, the
streaming-inference trio, head + loss, and the bias-gradient reduction.

Each HIP kernel is compared with a host oracle (tests/oracles.py) computed in
exact integer or fp64 arithmetic from the very values the kernel read, at
the shapes where its launcher switches kernels or a loop takes another trip.
Bounds are a-priori (number-format precision, summation length), never taken
from the kernel's own output.
"""
import pytest
import torch
import torch.nn as nn

import oracles as orc

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24       # fp32 unit roundoff
BF16_ULP_REL = 2.0 ** -7   # one bf16 ulp, relative to |ref| (upper bound)


def _ext():
    from fmda_amd.ops import load_extension
    return load_extension()


# ---------------------------------------------------------------------------
# 1. dropout: bit-exact against the host counter hash
# ---------------------------------------------------------------------------

DROP_PS = [0.3, 0.6, 0.8]
# the second seed has the top bit set once reinterpreted as uint64
DROP_SEEDS = [987654321, -(1 << 62) - 0x1234567]


def _rand_bf16(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 1.5).bfloat16()


@pytest.mark.parametrize("seed", DROP_SEEDS)
@pytest.mark.parametrize("p", DROP_PS)
@pytest.mark.parametrize("shape", [(3, 1371), (4113,), (4111,), (512, 8),
                                   (1,)])
def test_dropout_fused_matches_host_oracle(shape, p, seed):
    """numel % 8 in {1, 1, 7, 0, 1}: (3,1371)=4113 and 4111 run the tail
    branch after full octets, (1,) is a tail-only launch."""
    x = _rand_bf16(shape, 5)
    y = _ext().dropout_fused(x.cuda(), p, seed).cpu()
    assert torch.equal(y, orc.dropout_ref(x, p, seed))


@pytest.mark.parametrize("p", DROP_PS)
def test_dropout_fused_every_bf16_pattern(p):
    """All 2560 positive bf16 patterns in [2^-10, 2^10), repeated 4x so
    nearly every pattern is kept at least once: hits every rounding tie of
    x*scale, which is where a one-ulp-off scale shows."""
    x = orc.all_positive_normal_bf16().repeat(4)
    x = torch.cat([x, -x[:3]])          # 10243 elements: tail of 3
    seed = DROP_SEEDS[0]
    y = _ext().dropout_fused(x.cuda(), p, seed).cpu()
    ref = orc.dropout_ref(x, p, seed)
    assert torch.equal(y, ref), int((y != ref).sum())


@pytest.mark.parametrize("seed", DROP_SEEDS)
@pytest.mark.parametrize("p", DROP_PS)
def test_fused_dropout_backward_same_mask(p, seed):
    from fmda_amd.ops.interface import _FusedDropout
    x = _rand_bf16((3, 1371), 6).cuda().requires_grad_(True)
    dy = _rand_bf16((3, 1371), 7)
    y = _FusedDropout.apply(x, p, seed)
    y.backward(dy.cuda())
    assert torch.equal(y.detach().cpu(), orc.dropout_ref(x, p, seed))
    assert torch.equal(x.grad.cpu(), orc.dropout_ref(dy, p, seed))


@pytest.mark.parametrize("seed", DROP_SEEDS)
@pytest.mark.parametrize("p", DROP_PS)
@pytest.mark.parametrize("B,T,F", [(2, 5, 108), (3, 7, 5), (1, 1, 13)])
def test_spatial_dropout_fused_matches_host_oracle(B, T, F, p, seed):
    """F is no multiple of 8, so channel octets straddle batch rows; the
    105- and 13-element shapes also run the tail branch."""
    assert F % 8
    x = _rand_bf16((B, T, F), 8)
    y = _ext().spatial_dropout_fused(x.cuda(), p, seed).cpu()
    assert torch.equal(y, orc.spatial_dropout_ref(x, p, seed))


@pytest.mark.parametrize("p", DROP_PS)
def test_spatial_dropout_backward_same_mask(p):
    from fmda_amd.ops.interface import _FusedSpatialDropout
    seed = DROP_SEEDS[1]
    x = _rand_bf16((2, 5, 108), 9).cuda().requires_grad_(True)
    dy = _rand_bf16((2, 5, 108), 10)
    y = _FusedSpatialDropout.apply(x, p, seed)
    y.backward(dy.cuda())
    assert torch.equal(y.detach().cpu(), orc.spatial_dropout_ref(x, p, seed))
    assert torch.equal(x.grad.cpu(), orc.spatial_dropout_ref(dy, p, seed))


@pytest.mark.parametrize("p", DROP_PS)
@pytest.mark.parametrize("H,B,T", [(128, 37, 5), (512, 37, 3)])
def test_gru_fwd_fused_dropout_matches_host_oracle(H, B, T, p):
    """The `dropped` output of gru_fwd's store epilogue (v3 H=128 and
    column-split H=512, partial batch tile) is the host oracle applied to
    its own `out`, bit for bit."""
    ext = _ext()
    torch.manual_seed(4)
    gi = (torch.randn(B, T, 2 * 3 * H) * 0.5).bfloat16().cuda()
    w = (torch.randn(2, 3 * H, H) * 0.1).bfloat16().cuda()
    bhh = (torch.randn(2, 3 * H) * 0.1).cuda()
    seed = DROP_SEEDS[1]
    out, _, dropped = ext.gru_fwd(gi, w, bhh, None, p, seed)
    assert torch.equal(dropped.cpu(), orc.dropout_ref(out, p, seed))
    assert torch.equal(ext.dropout_fused(out, p, seed), dropped)


# ---------------------------------------------------------------------------
# 2. direction-sum + max/avg pooling
# ---------------------------------------------------------------------------

# (B, H, T): one shape on each side of every dispatch threshold of
# fmda_pool_fwd_launch (n = B*H/2 vs 4096; bf16 H%8) and
# fmda_pool_bwd_launch (bf16, H%8 == 0, B*H/8 vs 4096)
POOL_SMALL_OCT = [
    (3, 24, 130),     # small fwd, 3 lane-stride trips over T
    (63, 130, 9),     # small fwd, n = 4095
    (64, 128, 9),     # n = 4096: oct fwd (bf16), pair bwd (B*H/8 = 1024)
    (256, 128, 9),    # oct fwd and oct bwd (B*H/8 = 4096)
]
POOL_CASES = ([(s, nd) for s in POOL_SMALL_OCT for nd in (1, 2)]
              + [((320, 26, 9), 2)])   # large pair kernels, H % 8 != 0


def _pool_input(B, T, HD, dtype, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "ties":
        vals = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0])
        x = vals[torch.randint(0, 5, (B, T, HD), generator=g)]
    else:
        x = torch.randn(B, T, HD, generator=g) * 2
    return x.to(dtype)


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape,n_dir", POOL_CASES)
def test_pool_fwd_matches_oracle(shape, n_dir, dtype, kind):
    B, H, T = shape
    x = _pool_input(B, T, n_dir * H, dtype, kind, 11)
    ref = orc.pool_ref(x, n_dir)
    maxv, avgv, amax = [t.cpu() for t in _ext().pool_fwd(x.cuda(), n_dir)]
    # the fp32 direction sum is formed once, so max and argmax are exact;
    # ties resolve to the smallest t
    assert torch.equal(amax, ref["amax"]), \
        int((amax != ref["amax"]).sum())
    assert torch.equal(maxv, ref["maxv"])
    # fp32 summation of T terms + the division: T * 2^-24 * sum|x_t| / T
    bound = T * U32 * ref["abssum"] / T
    err = (avgv.double() - ref["avg"]).abs()
    assert (err <= bound).all(), float((err - bound).max())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape,n_dir", POOL_CASES)
def test_pool_bwd_matches_oracle(shape, n_dir, dtype):
    B, H, T = shape
    g = torch.Generator().manual_seed(12)
    # dmax in [1, 2): a max-gradient landing on the wrong t is an O(1) error
    dmax = 1.0 + torch.rand(B, H, generator=g)
    davg = torch.randn(B, H, generator=g)
    # argmax with many ties, from the oracle (not from the GPU forward)
    amax = orc.pool_ref(
        _pool_input(B, T, n_dir * H, torch.bfloat16, "ties", 13),
        n_dir)["amax"]
    dout = _ext().pool_bwd(dmax.cuda(), davg.cuda(), amax.cuda(), T, n_dir,
                           dtype).cpu()
    ref = orc.pool_bwd_ref(dmax, davg, amax, T, n_dir)
    assert dout.shape == ref.shape and dout.dtype == dtype
    if dtype == torch.float32:
        err = (dout.double() - ref).abs()
        tol = 4 * orc.fp32_ulp(ref)
    else:
        refb = ref.to(torch.float32).bfloat16().double()
        err = (dout.double() - refb).abs()
        tol = BF16_ULP_REL * ref.abs()
    assert (err <= tol).all(), float((err - tol).max())


# ---------------------------------------------------------------------------
# 3. streaming-inference kernels
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,Hp", [(128, 128), (24, 32)])
@pytest.mark.parametrize("n_dir", [1, 2])
@pytest.mark.parametrize("T", [32, 130])
@pytest.mark.parametrize("B", [1, 3])
def test_pool_concat_infer_matches_oracle(B, T, n_dir, H, Hp, dtype):
    g = torch.Generator().manual_seed(21)
    out = (torch.randn(B, T, n_dir * H, generator=g) * 2).to(dtype)
    hlast = torch.randn(n_dir, B, Hp, generator=g)
    feat = _ext().pool_concat_infer(out.cuda(), hlast.cuda(), H).cpu()
    assert feat.shape == (B, 3 * H) and feat.dtype == dtype

    pr = orc.pool_ref(out, n_dir)
    hl64 = hlast[:, :, :H].double()
    ref = torch.cat([hl64.sum(0), pr["max64"], pr["avg"]], dim=1)
    if dtype == torch.float32:
        # fp32 sums of n terms: n * 2^-24 * sum|terms| / n. The h_last and
        # max columns are direction sums (n = n_dir), the average has n = T
        bound = torch.cat([U32 * hl64.abs().sum(0),
                           U32 * pr["absdir"].max(dim=1).values,
                           T * U32 * pr["abssum"] / T], dim=1)
    else:
        bound = BF16_ULP_REL * ref.abs()
    err = (feat.double() - ref).abs()
    assert (err <= bound).all(), float((err - bound).max())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("K", [50, 72, 384])
@pytest.mark.parametrize("B", [1, 5])
def test_head_sigmoid_matches_oracle(B, K, dtype):
    """B=5 appends rows steered to logits of about +-40 and +-100 on class
    0: exp2 over/underflows there and the probabilities must saturate
    cleanly."""
    C = 4
    g = torch.Generator().manual_seed(31)
    W = (torch.randn(C, K, generator=g) * 0.2).to(dtype)
    b = (torch.randn(C, generator=g) * 0.1).to(dtype)
    x = (torch.randn(B, K, generator=g) * 0.5)
    if B == 5:
        w0 = W[0].float()
        for r, target in zip(range(1, 5), (40.0, -40.0, 100.0, -100.0)):
            x[r] = w0 * (target / float(w0 @ w0))
    x = x.to(dtype)
    probs = _ext().head_sigmoid(x.cuda(), W.cuda(), b.cuda()).cpu()

    prod = x.double()[:, None, :] * W.double()[None, :, :]     # (B, C, K)
    logits = prod.sum(-1) + b.double()
    ref = torch.sigmoid(logits)
    if B == 5:
        got = logits[1:, 0].abs()
        assert (got[:2] > 35).all() and (got[2:] > 90).all(), got
    # |sigmoid'| <= 1/4 times the K-term fp32 dot bound, + 1e-6 for the
    # fast exp2/rcp (about 1e-7 relative per the kernel's own comment)
    bound = 0.25 * K * U32 * prod.abs().sum(-1) + 1e-6
    assert torch.isfinite(probs).all()
    assert (probs >= 0).all() and (probs <= 1).all()
    err = (probs.double() - ref).abs()
    assert (err <= bound).all(), float((err - bound).max())


@pytest.mark.parametrize("T,F", [(1, 96), (2, 5), (32, 96), (120, 108),
                                 (513, 96)])
def test_ingest_row_shift_and_normalize(T, F):
    """(513, 96) is exactly the single-workgroup capacity (T-1)*F = 48*1024."""
    ext = _ext()
    g = torch.Generator().manual_seed(41)
    ring = torch.randn(T, F, generator=g).bfloat16().cuda()
    xmin = torch.randn(F, generator=g)
    xrng = torch.rand(F, generator=g) * 3 + 0.5
    xmin_d, xrng_d = xmin.cuda(), xrng.cuda()
    prev = ring.cpu().clone()
    for push in range(T + 3):
        row = torch.randn(F, generator=g) * 2
        ext.ingest_row(ring, row.cuda(), xmin_d, xrng_d)
        cur = ring.cpu().clone()
        assert torch.equal(cur[:T - 1], prev[1:]), push
        want = ((row - xmin) / xrng).bfloat16().double()   # fp32 math, RNE
        err = (cur[T - 1].double() - want).abs()
        assert (err <= BF16_ULP_REL * want.abs()).all(), (push, float(err.max()))
        prev = cur


def test_ingest_row_rejects_window_over_capacity():
    ext = _ext()
    T, F = 514, 96
    ring = torch.zeros(T, F, dtype=torch.bfloat16, device="cuda")
    z = torch.zeros(F, device="cuda")
    with pytest.raises(RuntimeError, match="ingest_row launch failed"):
        ext.ingest_row(ring, z, z, torch.ones(F, device="cuda"))
    torch.cuda.synchronize()
    assert not ring.any()


# ---------------------------------------------------------------------------
# 4. head + loss with more than one block of per-block partials
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,xscale", [(64, 0.5), (65, 0.5), (700, 0.5),
                                      (65, 8.0)])
def test_fused_head_loss_multi_block_matches_fp64(B, xscale, dtype):
    """B*C/256 = 1, 2 and 11 blocks; xscale=8 drives logits past |60|,
    where log(sigmoid(x)) evaluated naively is -inf."""
    from fmda_amd.ops.interface import fused_head_loss
    K, C = 384, 4
    g = torch.Generator().manual_seed(51)
    x = (torch.randn(B, K, generator=g) * xscale).to(dtype)
    W = torch.randn(C, K, generator=g) * 0.2
    bias = torch.randn(C, generator=g) * 0.1
    y = (torch.rand(B, C, generator=g) < 0.3).float()
    wgt = torch.rand(C, generator=g) * 3 + 0.5
    pw = torch.rand(C, generator=g) * 4 + 0.5

    xg = x.cuda().requires_grad_(True)
    Wg = W.cuda().requires_grad_(True)
    bg = bias.cuda().requires_grad_(True)
    loss1, logits1 = fused_head_loss(xg, Wg, bg, y.cuda(), wgt.cuda(),
                                     pw.cuda())
    loss1.backward()

    # fp64 oracle on the values the kernel read (params cast to dtype)
    x64 = x.double().requires_grad_(True)
    W64 = W.to(dtype).double().requires_grad_(True)
    b64 = bias.to(dtype).double().requires_grad_(True)
    logits2 = torch.nn.functional.linear(x64, W64, b64)
    loss2 = nn.functional.binary_cross_entropy_with_logits(
        logits2, y.double(), weight=wgt.double(), pos_weight=pw.double())
    loss2.backward()
    if xscale > 1:
        assert logits2.abs().max() > 60, float(logits2.abs().max())

    assert torch.isfinite(loss1).item()
    for t in (xg.grad, Wg.grad, bg.grad):
        assert torch.isfinite(t).all()
    tol = 1e-5 if dtype == torch.float32 else 3e-2
    assert torch.allclose(loss1.double().cpu(), loss2.detach(), atol=tol,
                          rtol=tol), (float(loss1), float(loss2))
    gtol = 1e-4 if dtype == torch.float32 else 5e-2

    def rel(a, b):
        return float((a.double().cpu() - b).abs().max() /
                     b.abs().max().clamp(min=1e-3))
    assert rel(xg.grad, x64.grad) < gtol, rel(xg.grad, x64.grad)
    assert rel(Wg.grad, W64.grad) < gtol, rel(Wg.grad, W64.grad)
    assert rel(bg.grad, b64.grad) < gtol, rel(bg.grad, b64.grad)


# ---------------------------------------------------------------------------
# 5. bias-gradient reduction over more than 16 partial rows
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,H,B,rows", [
    ("fp32", 32, 545, 18),     # 32-row batch tiles
    ("bf16", 128, 545, 18),    # v3, 32-row tiles
    ("bf16", 512, 520, 24),    # column-split: 8 waves x 3 batch groups
])
def test_db_reduce_more_than_16_partial_rows(dtype, H, B, rows):
    """db_reduce_kernel strides the partial rows by 16 per wave: with more
    than 16 rows its row loop takes a second trip."""
    from fmda_amd.ops.interface import _BiGRULayer, gru_directions
    # rows of the partials table: one per 32-row batch tile, or one per
    # (256-row batch group, wave of 8) on the column-split kernel
    assert rows == (8 * -(-B // 256) if H == 512 else -(-B // 32)) > 16
    T, n_dir, F = 3, 2, 24
    torch.manual_seed(61)
    bf16 = dtype == "bf16"

    def check(nm, a, ref):
        a, ref = a.float(), ref.float()
        if not bf16:
            scale = ref.abs().max().clamp(min=1.0)
            v = float((a - ref).abs().max() / scale)
            assert v < 1e-4, (nm, v)
        elif H <= 128:
            v = float((a - ref).abs().max() / ref.abs().max().clamp(min=1e-2))
            assert v < 6e-2, (nm, v)
        else:
            v = float((a - ref).norm() / ref.norm().clamp(min=1e-2))
            assert v < 8e-2, (nm, v)

    # recurrence alone: db_hh against autograd on the golden recurrence
    gi = (torch.randn(B, T, n_dir * 3 * H) * 0.5).cuda()
    w = (torch.randn(n_dir, 3 * H, H) * 0.2).cuda()
    bhh = (torch.randn(n_dir, 3 * H) * 0.1).cuda()
    dO = torch.randn(B, T, n_dir * H).cuda()
    dH = torch.randn(n_dir, B, H).cuda()
    cast = (lambda t: t.bfloat16()) if bf16 else (lambda t: t.clone())
    gi1 = cast(gi).requires_grad_(True)
    w1 = cast(w).requires_grad_(True)
    b1 = bhh.clone().requires_grad_(True)
    out1, hl1 = gru_directions(gi1, w1, b1)
    ((out1.float() * dO).sum() + (hl1 * dH).sum()).backward()
    gi2 = gi.clone().requires_grad_(True)
    w2 = w.clone().requires_grad_(True)
    b2 = bhh.clone().requires_grad_(True)
    out2, hl2 = orc.gru_ref_from_gi(gi2, w2, b2)
    ((out2 * dO).sum() + (hl2 * dH).sum()).backward()
    check("db_hh", b1.grad, b2.grad)
    if not bf16:
        return

    # whole layer node: db_ih (slots 0, 1, 3 of the same partial rows)
    params = []
    for d in range(2):
        params += [
            (torch.randn(3 * H, F, device="cuda") * 0.2).requires_grad_(True),
            (torch.randn(3 * H, H, device="cuda") * 0.2).requires_grad_(True),
            (torch.randn(3 * H, device="cuda") * 0.1).requires_grad_(True),
            (torch.randn(3 * H, device="cuda") * 0.1).requires_grad_(True),
        ]
    x = (torch.randn(B, T, F, device="cuda") * 0.5).bfloat16()
    out, hl = _BiGRULayer.apply(x, H, *params)
    ((out.float() * dO).sum() + (hl * dH).sum()).backward()
    got = {"b_ih0": params[2].grad.clone(), "b_hh0": params[3].grad.clone(),
           "b_ih1": params[6].grad.clone(), "b_hh1": params[7].grad.clone()}
    for p in params:
        p.grad = None
    x32 = x.float().reshape(-1, F)
    gi3 = torch.cat([x32 @ params[0].t() + params[2],
                     x32 @ params[4].t() + params[6]], dim=-1).view(B, T, -1)
    out3, hl3 = orc.gru_ref_from_gi(
        gi3, torch.stack([params[1], params[5]], 0),
        torch.stack([params[3], params[7]], 0))
    ((out3 * dO).sum() + (hl3 * dH).sum()).backward()
    for nm, i in (("b_ih0", 2), ("b_hh0", 3), ("b_ih1", 6), ("b_hh1", 7)):
        check(nm, got[nm], params[i].grad)
