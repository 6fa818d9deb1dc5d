"""gru_bwd_v3's per-step integer work: the fused inter-layer dropout mask
drawn once per octet and shared by 8 lanes, and the one-step-late dGi / dGh
tile stores addressed from offsets formed once per launch.

Neither changes a value, so every comparison is on bit patterns: a wrong
byte of a draw, a wrong lane of the exchange, a wrong counter (batch offset
b0 > 0, dir = 1) or a chunk stored to the wrong row, column or time step
shows as unequal bits. Shapes: Hp = H = 128, D in {1, 2}, T in {1, 2, 3, 7},
B in {1, 31, 32, 33, 70} (one row, a tail of a 32-row block, exactly full,
one row over, a third block with b0 = 64), with and without h0, wt passed.
tests/test_bwd_step_int_cases.py checks on the CPU that both mask values
occur in every (shape, p, seed) used here.
"""
import functools

import numpy as np
import pytest
import torch

import oracles as orc

pytestmark = pytest.mark.gpu

BF16, FP32 = torch.bfloat16, torch.float32
H = 128
BMAX = 70
BATCHES = [1, 31, 32, 33, 70]
DIRS = [1, 2]
STEPS = [1, 2, 3, 7]
# scale 2, 4, 8: the fp32 product is exact, so pre-dropping d_out in bf16
# and dropping inside the kernel in fp32 give the same bits
P_POW2 = [0.5, 0.75, 0.875]
P_ANY = [0.3, 0.6]
# int64 as the binding receives it; two with the top bit set
SEEDS = [1234, -1, -(2 ** 63) + 12345, 0x5DEECE66D]
NAMES = ["dgi", "dgh", "dh0", "dbhh", "dbih", "dgh0"]


def seed_for(D, T, B, p):
    """The seed of one case: every seed is used, spread over the cases."""
    return SEEDS[(D + T + B + int(p * 1000)) % len(SEEDS)]


def _ext():
    from fmda_amd.ops import load_extension
    return load_extension()


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal as bit patterns (-0.0 != 0.0, NaN == the same NaN)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = {FP32: torch.int32, BF16: torch.int16}[a.dtype]
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _assert_same(got, ref, use_h0, tag, names=NAMES):
    assert len(got) == len(ref) == (6 if use_h0 else 5), tag
    for name, a, r in zip(NAMES, got, ref):
        if name in names:
            assert _bits_equal(a, r), (tag, name)


@functools.lru_cache(maxsize=None)
def _weights(D):
    g = torch.Generator().manual_seed(200 + D)
    w = (torch.randn(D, 3 * H, H, generator=g) * 0.1).to(BF16).cuda()
    bhh = (torch.randn(D, 3 * H, generator=g) * 0.1).cuda()
    wt = w.transpose(1, 2).contiguous()
    return w, bhh, wt


@functools.lru_cache(maxsize=None)
def _case(D, T):
    """CPU inputs of one (D, T) at BMAX rows; the first B rows serve every
    batch size. |d_out| stays far below bf16's range / 8."""
    g = torch.Generator().manual_seed(2000 * D + T)
    gi = (torch.randn(BMAX, T, D * 3 * H, generator=g) * 0.5).to(BF16)
    out = torch.tanh(torch.randn(BMAX, T, D * H, generator=g)).to(BF16)
    dout = (torch.randn(BMAX, T, D * H, generator=g) * 0.5).to(BF16)
    dout[dout == 0] = 0.25                      # nonzero everywhere
    dhT = torch.randn(D, BMAX, H, generator=g) * 0.5
    h0 = torch.randn(D, BMAX, H, generator=g) * 0.5
    return gi, out, dout, dhT, h0


def _rows(D, T, lo, hi, use_h0):
    """Rows [lo, hi) of the case, on the device."""
    gi, out, dout, dhT, h0 = _case(D, T)
    return (gi[lo:hi].contiguous().cuda(), out[lo:hi].contiguous().cuda(),
            dout[lo:hi].contiguous(), dhT[:, lo:hi].contiguous().cuda(),
            h0[:, lo:hi].contiguous().cuda() if use_h0 else None)


def _bwd(D, gi, out, dout, dhT, h0, p, seed):
    w, bhh, wt = _weights(D)
    return _ext().gru_bwd(gi, w, bhh, out, dout.cuda(), dhT, p, seed, h0, wt)


# ---------------------------------------------------------------------------
# 1. mask and scale exact where the scale is a power of two
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("use_h0", [False, True], ids=["zero_h0", "h0"])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("D", DIRS)
def test_fused_dropout_equals_predropped(D, T, use_h0):
    for B in BATCHES:
        gi, out, dout, dhT, h0 = _rows(D, T, 0, B, use_h0)
        for p in P_POW2:
            seed = seed_for(D, T, B, p)
            fused = _bwd(D, gi, out, dout, dhT, h0, p, seed)
            ref = _bwd(D, gi, out, orc.dropout_ref(dout, p, seed), dhT, h0,
                       0.0, 0)
            assert torch.isfinite(ref[0].float()).all()
            _assert_same(fused, ref, use_h0, f"B={B} p={p} seed={seed}")


def test_wt_argument_changes_nothing():
    """wt passed (every other case here) against wt built by the binding."""
    D, T, B, p = 2, 3, 33, 0.5
    gi, out, dout, dhT, h0 = _rows(D, T, 0, B, True)
    w, bhh, _ = _weights(D)
    a = _bwd(D, gi, out, dout, dhT, h0, p, SEEDS[1])
    b = _ext().gru_bwd(gi, w, bhh, out, dout.cuda(), dhT, p, SEEDS[1], h0,
                       None)
    _assert_same(a, b, True, "wt")


# ---------------------------------------------------------------------------
# 2. mask exact at any p
# ---------------------------------------------------------------------------

def _mask_probe(D, T, B, use_h0, p, seed):
    """dgi's n columns (B, T, D, H) of a launch built so that they carry
    bf16(doval) and nothing else: W = 0 and b_hh = 0 give hn = 0, gi_r =
    gi_n = 0 give r = 1/2 and n = tanh(0), gi_z = -30000 saturates the
    sigmoid to z = 0 exactly, so dn_pre = dht * (1 - n * n), the carry
    dht * z + dGh W is 0 and dht = doval at every step."""
    _, _, dout, _, h0 = _case(D, T)
    dout = dout[:B].contiguous()
    gi = torch.zeros(B, T, D, 3, H, dtype=BF16)
    gi[:, :, :, 1, :] = -30000.0
    gi = gi.reshape(B, T, D * 3 * H).cuda()
    w = torch.zeros(D, 3 * H, H, dtype=BF16, device="cuda")
    res = _ext().gru_bwd(
        gi, w, torch.zeros(D, 3 * H, device="cuda"),
        torch.zeros(B, T, D * H, dtype=BF16, device="cuda"), dout.cuda(),
        torch.zeros(D, B, H, device="cuda"), p, seed,
        h0[:, :B].contiguous().cuda() if use_h0 else None,
        w.transpose(1, 2).contiguous())
    dgi_n = res[0].reshape(B, T, D, 3, H)[:, :, :, 2, :].cpu()
    return dgi_n, dout.reshape(B, T, D, H)


@pytest.mark.parametrize("use_h0", [False, True], ids=["zero_h0", "h0"])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("D", DIRS)
def test_mask_pattern_any_p(D, T, use_h0):
    for B in BATCHES:
        # n is exactly 0 on the device iff the launch without dropout hands
        # d_out through unchanged; only then are the kept values comparable
        plain, dout = _mask_probe(D, T, B, use_h0, 0.0, 0)
        n_is_zero = _bits_equal(plain.contiguous(), dout.contiguous())
        for p in P_ANY:
            seed = seed_for(D, T, B, p)
            got, _ = _mask_probe(D, T, B, use_h0, p, seed)
            idx = np.arange(B * T * D * H, dtype=np.uint64)
            dropped = torch.from_numpy(
                orc.drop_mask(idx, p, seed)).reshape(B, T, D, H)
            tag = f"B={B} p={p} seed={seed}"
            assert torch.equal(got.view(torch.int16) == 0, dropped), tag
            if n_is_zero:
                ref = orc.dropout_ref(dout.contiguous(), p, seed)
                assert _bits_equal(got.contiguous(), ref), tag
    # tanh(0) = 1 - 2 * rcp(1 + exp2(0)) is exactly 0 on gfx950 (rcp(2) is
    # exact), so the value comparison above is expected to run; the probe
    # without dropout decides it, not this comment.


# ---------------------------------------------------------------------------
# 3. store placement
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.0, 0.5], ids=["nodrop", "drop"])
@pytest.mark.parametrize("use_h0", [False, True], ids=["zero_h0", "h0"])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("D", DIRS)
def test_dgh_is_dgi_shifted_one_step(D, T, use_h0, p):
    for B in BATCHES:
        gi, out, dout, dhT, h0 = _rows(D, T, 0, B, use_h0)
        res = _bwd(D, gi, out, dout, dhT, h0, p, seed_for(D, T, B, p))
        dgi = res[0].reshape(B, T, D, 3 * H)
        dgh = res[1].reshape(B, T, D, 3 * H)
        assert torch.isfinite(dgi.float()).all()
        assert (dgi.view(torch.int16) != 0).any()
        for d in range(D):
            if d == 0:      # forward direction: dGh of step t sits at t - 1
                a, b, edge = dgh[:, :T - 1, d, :2 * H], dgi[:, 1:, d, :2 * H], T - 1
            else:           # reverse direction: at t + 1
                a, b, edge = dgh[:, 1:, d, :2 * H], dgi[:, :T - 1, d, :2 * H], 0
            assert _bits_equal(a, b), (B, d)
            assert not dgh[:, edge, d, :].view(torch.int16).any(), (B, d)


@pytest.mark.parametrize("p", [0.0, 0.5], ids=["nodrop", "drop"])
@pytest.mark.parametrize("use_h0", [False, True], ids=["zero_h0", "h0"])
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("D", DIRS)
def test_rows_independent_of_their_block(D, T, use_h0, p):
    """Rows of the B = 70 launch against the same rows launched as 32, 32
    and 6. The dropout counter follows the row's place in the whole batch,
    so the pieces get the whole batch's d_out dropped beforehand (exact at
    p = 0.5) and no dropout of their own."""
    seed = seed_for(D, T, BMAX, p)
    gi, out, dout, dhT, h0 = _rows(D, T, 0, BMAX, use_h0)
    whole = _bwd(D, gi, out, dout, dhT, h0, p, seed)
    dropped = orc.dropout_ref(dout, p, seed) if p else dout
    for lo, hi in [(0, 32), (32, 64), (64, 70)]:
        gi, out, _, dhT, h0 = _rows(D, T, lo, hi, use_h0)
        part = _bwd(D, gi, out, dropped[lo:hi].contiguous(), dhT, h0, 0.0, 0)
        assert _bits_equal(part[0], whole[0][lo:hi]), ("dgi", lo)
        assert _bits_equal(part[1], whole[1][lo:hi]), ("dgh", lo)
        assert _bits_equal(part[2], whole[2][:, lo:hi]), ("dh0", lo)
        if use_h0:
            assert _bits_equal(part[5], whole[5][:, lo:hi]), ("dgh0", lo)


# ---------------------------------------------------------------------------
# 4. the pooled entry point
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("use_h0", [False, True], ids=["zero_h0", "h0"])
def test_pooled_entry_point_equals_dense(use_h0):
    ext = _ext()
    D, T, B = 2, 7, 70
    w, bhh, wt = _weights(D)
    gi, out, _, _, h0 = _rows(D, T, 0, B, use_h0)
    g = torch.Generator().manual_seed(77)
    dfeat = torch.randn(B, 3 * H, generator=g).to(BF16).cuda()
    b = torch.arange(B)[:, None]
    j = torch.arange(H)[None, :]
    amax = ((3 * b + 5 * j + (b * j) // 7) % T).int().cuda()
    d_out, d_hlast = ext.pool_features_bwd(dfeat, amax, T, D)
    dense = ext.gru_bwd(gi, w, bhh, out, d_out, d_hlast, 0.0, 0, h0, wt)
    pooled = ext.gru_bwd(gi, w, bhh, out, None, None, 0.0, 0, h0, wt,
                         dfeat, amax)
    _assert_same(pooled, dense, use_h0, "pooled")
    dgi = pooled[0].reshape(B, T, D, 3 * H)
    dgh = pooled[1].reshape(B, T, D, 3 * H)
    assert _bits_equal(dgh[:, :T - 1, 0, :2 * H], dgi[:, 1:, 0, :2 * H])
    assert _bits_equal(dgh[:, 1:, 1, :2 * H], dgi[:, :T - 1, 1, :2 * H])
