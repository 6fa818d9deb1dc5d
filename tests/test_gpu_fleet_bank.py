"""GPU tests of the banked fleet predictor: the three kernels that read a
per-stream slot into a bank of models, and BankedFleetPredictor's captured
tick with `assign` / `swap_model` between replays."""
import functools
import itertools
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HP = 128
S_MAX = 17
M_MAX = 3


def _ext():
    from fmda_amd.ops import load_extension
    return load_extension()


def _slots(S, M, pattern):
    """"rot" is a permutation of the slots at S == M (not the identity),
    "pairs" repeats every slot; both use every slot once S allows it."""
    if pattern == "rot":
        return [(s + 2) % M for s in range(S)]
    return [(s // 2) % M for s in range(S)]


def _slot_t(slots):
    return torch.tensor(slots, dtype=torch.int32, device="cuda")


def _poison(*shapes_dtypes):
    """The bindings allocate their outputs; fill the blocks the caching
    allocator will hand them with NaN, so an unwritten row or a stream
    writing into a neighbour's slab shows as NaN / a mismatch."""
    junk = [torch.full(shape, float("nan"), device="cuda", dtype=dt)
            for shape, dt in shapes_dtypes]
    torch.cuda.synchronize()
    del junk


# ---------------- gru_fwd_streams_bank ----------------

@functools.lru_cache(maxsize=None)
def _streams_case(T, n_dir):
    """Inputs for S_MAX streams and M_MAX models, seeded as the
    gru_fwd_streams tests seed theirs, and what gru_fwd_streams gives for
    every (stream, model) pair on that stream alone. Computed once per
    (T, n_dir) and shared by the whole sweep."""
    ext = _ext()
    g = torch.Generator().manual_seed(1000 * T + n_dir)
    gi = (torch.randn(S_MAX, T, n_dir * 3 * HP, generator=g) * 0.5
          ).to("cuda", torch.bfloat16)
    w = (torch.randn(M_MAX, n_dir, 3 * HP, HP, generator=g) * 0.08
         ).to("cuda", torch.bfloat16)
    bhh = (torch.randn(M_MAX, n_dir, 3 * HP, generator=g) * 0.1).cuda()
    ref = [[ext.gru_fwd_streams(gi[s:s + 1].contiguous(), w[m], bhh[m])
            for m in range(M_MAX)] for s in range(S_MAX)]
    assert not torch.isnan(ref[0][0][0].float()).any()
    assert not torch.equal(ref[0][0][0], ref[0][1][0])   # the models differ
    return gi, w, bhh, ref


@pytest.mark.parametrize("pattern", ["rot", "pairs"])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("n_dir", [1, 2])
@pytest.mark.parametrize("T", [1, 2, 32])
@pytest.mark.parametrize("S", [1, 3, 17])
def test_gru_fwd_streams_bank_is_bitwise_gru_fwd_streams(S, T, n_dir, M,
                                                         pattern):
    ext = _ext()
    gi, w, bhh, ref = _streams_case(T, n_dir)
    slots = _slots(S, M, pattern)
    gi_s = gi[:S].contiguous()
    wb, bb = w[:M].contiguous(), bhh[:M].contiguous()
    _poison(((S, T, n_dir * HP), torch.bfloat16),
            ((n_dir, S, HP), torch.float32))
    out, hl = ext.gru_fwd_streams_bank(gi_s, _slot_t(slots), wb, bb)
    assert out.shape == (S, T, n_dir * HP) and out.dtype == torch.bfloat16
    assert hl.shape == (n_dir, S, HP) and hl.dtype == torch.float32
    for s, m in enumerate(slots):
        r_out, r_hl = ref[s][m]
        assert torch.equal(out[s], r_out[0]), (s, m)
        assert torch.equal(hl[:, s], r_hl[:, 0]), (s, m)


def test_gru_fwd_streams_bank_binding_checks():
    ext = _ext()
    gi, w, bhh, _ = _streams_case(2, 2)
    slot = _slot_t([0] * S_MAX)
    ext.gru_fwd_streams_bank(gi, slot, w, bhh)                  # well-formed
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams_bank(gi.float(), slot, w, bhh)      # dtype
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams_bank(gi[:, :, :-8], slot, w, bhh)   # contiguity
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams_bank(gi[:, :, :3 * HP].contiguous(), slot, w,
                                 bhh)                           # shape
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams_bank(gi, slot, w[0], bhh[0])        # no bank dim
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams_bank(gi, slot, w, bhh[:2].contiguous())  # M
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams_bank(gi, slot, w, bhh.to(torch.bfloat16))
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams_bank(gi, slot.long(), w, bhh)       # slot dtype
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams_bank(gi, slot[:-1].contiguous(), w, bhh)
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams_bank(gi, slot.cpu(), w, bhh)        # device
    t_over = (150 * 1024 - 2080) // (2 * 392) + 1
    big = torch.zeros(1, t_over, 2 * 3 * HP, device="cuda",
                      dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="LDS"):
        ext.gru_fwd_streams_bank(big, _slot_t([0]), w, bhh)


# ---------------- head_sigmoid_bank ----------------

@pytest.mark.parametrize("pattern", ["rot", "pairs"])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("S", [1, 3, 17])
def test_head_sigmoid_bank_is_bitwise_head_sigmoid(S, M, pattern):
    ext = _ext()
    K, C = 3 * HP, 4
    g = torch.Generator().manual_seed(77)
    feat = torch.randn(S_MAX, K, generator=g).to("cuda", torch.bfloat16)
    W = (torch.randn(M_MAX, C, K, generator=g) * 0.05
         ).to("cuda", torch.bfloat16)
    b = (torch.randn(M_MAX, C, generator=g) * 0.1).to("cuda", torch.bfloat16)
    slots = _slots(S, M, pattern)
    f = feat[:S].contiguous()
    _poison(((S, C), torch.float32))
    got = ext.head_sigmoid_bank(f, _slot_t(slots), W[:M].contiguous(),
                                b[:M].contiguous())
    assert got.shape == (S, C) and got.dtype == torch.float32
    for s, m in enumerate(slots):
        want = ext.head_sigmoid(f[s:s + 1].contiguous(), W[m], b[m])
        assert torch.equal(got[s:s + 1], want), (s, m)
    if M == 3 and S >= 3:
        assert not torch.equal(
            got[0:1], ext.head_sigmoid(f[0:1].contiguous(), W[1], b[1]))


def test_head_sigmoid_bank_binding_checks():
    ext = _ext()
    feat = torch.zeros(3, 384, device="cuda", dtype=torch.bfloat16)
    W = torch.zeros(2, 4, 384, device="cuda", dtype=torch.bfloat16)
    b = torch.zeros(2, 4, device="cuda", dtype=torch.bfloat16)
    slot = _slot_t([0, 1, 0])
    ext.head_sigmoid_bank(feat, slot, W, b)                     # well-formed
    with pytest.raises(RuntimeError):
        ext.head_sigmoid_bank(feat.float(), slot, W, b)         # dtype
    with pytest.raises(RuntimeError):
        ext.head_sigmoid_bank(feat, slot, W[0], b[0])           # no bank dim
    with pytest.raises(RuntimeError):
        ext.head_sigmoid_bank(feat, slot, W[:, :, :380], b)     # contiguity
    with pytest.raises(RuntimeError):
        ext.head_sigmoid_bank(feat[:, :380].contiguous(), slot, W, b)  # K
    with pytest.raises(RuntimeError):
        ext.head_sigmoid_bank(feat, slot, W, b[:1].contiguous())  # M
    with pytest.raises(RuntimeError):
        ext.head_sigmoid_bank(feat, slot.long(), W, b)          # slot dtype
    with pytest.raises(RuntimeError):
        ext.head_sigmoid_bank(feat, slot[:2].contiguous(), W, b)
    with pytest.raises(RuntimeError):
        ext.head_sigmoid_bank(feat, slot.cpu(), W, b)           # device


# ---------------- gi_proj_bank ----------------

@functools.lru_cache(maxsize=2)
def _proj_case(K, T, N):
    """bf16 inputs for S_MAX streams and M_MAX models and, in float64 on
    the CPU, every stream through every model: ref[m, s] = x[s] @ W[m]^T +
    b[m], and the magnitude sum |x| @ |W[m]|^T + |b[m]| of the error
    bound. The sweep runs (K, T, N) outermost, so each is built once."""
    g = torch.Generator().manual_seed(100000 * K + 100 * T + N)
    x = torch.randn(S_MAX, T, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(M_MAX, N, K, generator=g) * 0.1).to(torch.bfloat16)
    b = (torch.randn(M_MAX, N, generator=g) * 0.1).to(torch.bfloat16)
    x64, W64, b64 = x.double(), W.double(), b.double()
    ref = torch.einsum("stk,mnk->mstn", x64, W64) + b64[:, None, None, :]
    mag = torch.einsum("stk,mnk->mstn", x64.abs(), W64.abs()) \
        + b64.abs()[:, None, None, :]
    return x.cuda(), W.cuda(), b.cuda(), ref, mag


def _check_proj(K, T, S, M, N, slots):
    ext = _ext()
    x, W, b, ref, mag = _proj_case(K, T, N)
    _poison(((S, T, N), torch.bfloat16))
    got = ext.gi_proj_bank(x[:S].contiguous(), _slot_t(slots),
                           W[:M].contiguous(), b[:M].contiguous())
    assert got.shape == (S, T, N) and got.dtype == torch.bfloat16
    got = got.double().cpu()
    for s, m in enumerate(slots):
        # one bf16 ulp of the result + a loose fp32 accumulation bound
        tol = 2.0 ** -7 * ref[m, s].abs() + 2 * K * 2.0 ** -24 * mag[m, s]
        err = (got[s] - ref[m, s]).abs()
        assert bool((err <= tol).all()), (
            s, m, float((err - tol).max()), float(err.max()))


_PROJ_SWEEP = [(K, T, S, M, N)
               for K, T, N in itertools.product([4, 36, 96, 108, 256],
                                                [1, 15, 16, 17, 33],
                                                [384, 768])
               for S, M in itertools.product([1, 3, 17], [1, 3])]


@pytest.mark.parametrize("K,T,S,M,N", _PROJ_SWEEP)
def test_gi_proj_bank_against_float64(K, T, S, M, N):
    _check_proj(K, T, S, M, N, _slots(S, M, "rot"))


@pytest.mark.parametrize("K", [5, 37])
def test_gi_proj_bank_odd_k_takes_element_loads(K):
    """K % 4 != 0: rows are only 2-byte aligned and every fragment element
    is loaded on its own. Same bound."""
    _check_proj(K, 17, 3, 3, 384, _slots(3, 3, "pairs"))


def test_gi_proj_bank_unaligned_base_pointers():
    """K % 8 == 0 says nothing about the base: a view that starts 8 bytes
    into its storage must not be read with 16-byte loads. Same numbers as
    the aligned tensors give."""
    ext = _ext()
    K, T, N, S, M = 96, 17, 384, 3, 3
    x, W, b, _, _ = _proj_case(K, T, N)
    xs, Ws = x[:S].contiguous(), W[:M].contiguous()
    slot = _slot_t([2, 0, 1])
    want = ext.gi_proj_bank(xs, slot, Ws, b)

    def shifted(t, by):
        buf = torch.empty(t.numel() + by, device="cuda", dtype=t.dtype)
        v = buf[by:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 2 * by
        return v

    assert torch.equal(ext.gi_proj_bank(shifted(xs, 4), slot, Ws, b), want)
    assert torch.equal(ext.gi_proj_bank(xs, slot, shifted(Ws, 4), b), want)
    assert torch.equal(ext.gi_proj_bank(shifted(xs, 1), slot, Ws, b), want)


@pytest.mark.parametrize("K", [36, 96, 108])
def test_gi_proj_bank_streams_are_independent_bitwise(K):
    ext = _ext()
    T, N, S, M = 17, 768, 7, 3
    x, W, b, _, _ = _proj_case(K, T, N)
    xs = x[:S].contiguous()
    slots = [s % M for s in range(S)]                  # [0, 1, 2, 0, ...]
    got = ext.gi_proj_bank(xs, _slot_t(slots), W, b)
    zero = _slot_t([0])
    for s, m in enumerate(slots):
        alone = ext.gi_proj_bank(xs[s:s + 1].contiguous(), zero,
                                 W[m:m + 1].contiguous(),
                                 b[m:m + 1].contiguous())
        assert torch.equal(got[s], alone[0]), (s, m)
    # streams and their slots permuted together: the rows permute
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(K))
    assert not torch.equal(perm, torch.arange(S))
    got_p = ext.gi_proj_bank(xs[perm.cuda()].contiguous(),
                             _slot_t([slots[i] for i in perm.tolist()]),
                             W, b)
    assert torch.equal(got_p, got[perm.cuda()])
    # and the slot matters
    assert not torch.equal(got[0], got[1]) and not torch.equal(
        got[0], ext.gi_proj_bank(xs[0:1].contiguous(), zero,
                                 W[1:2].contiguous(),
                                 b[1:2].contiguous())[0])


def test_gi_proj_bank_binding_checks():
    ext = _ext()
    x, W, b, _, _ = _proj_case(96, 16, 384)
    slot = _slot_t([0] * S_MAX)
    ext.gi_proj_bank(x, slot, W, b)                             # well-formed
    with pytest.raises(RuntimeError):
        ext.gi_proj_bank(x.float(), slot, W, b)                 # dtype
    with pytest.raises(RuntimeError):
        ext.gi_proj_bank(x, slot, W.float(), b)
    with pytest.raises(RuntimeError):
        ext.gi_proj_bank(x[:, :, :88], slot, W, b)              # contiguity
    with pytest.raises(RuntimeError):
        ext.gi_proj_bank(x[:, :, :88].contiguous(), slot, W, b)  # K
    with pytest.raises(RuntimeError):
        ext.gi_proj_bank(x, slot, W[0], b[0])                   # no bank dim
    with pytest.raises(RuntimeError):
        ext.gi_proj_bank(x, slot, W, b[:2].contiguous())        # M
    with pytest.raises(RuntimeError):
        ext.gi_proj_bank(x, slot, W[:, :380].contiguous(),
                         b[:, :380].contiguous())               # N % 16
    with pytest.raises(RuntimeError):
        ext.gi_proj_bank(x, slot.long(), W, b)                  # slot dtype
    with pytest.raises(RuntimeError):
        ext.gi_proj_bank(x, slot[:-1].contiguous(), W, b)       # slot length
    with pytest.raises(RuntimeError):
        ext.gi_proj_bank(x, slot.cpu(), W, b)                   # device


# ---------------- BankedFleetPredictor ----------------

F = 96
W32 = 32
SYMS6 = [f"S{i}" for i in range(6)]
SLOTS6 = [0, 1, 2, 0, 2, 1]


def _model(H, L=2, seed=0):
    from fmda_amd.models import BiGRU
    torch.manual_seed(seed)
    return BiGRU(H, F, 4, n_layers=L,
                 spatial_dropout=False).to(torch.bfloat16)


def _tables(S):
    g = torch.Generator().manual_seed(21)
    x_min = torch.rand(S, F, generator=g) * 0.1 + \
        torch.arange(S).float().unsqueeze(1)          # distinct price levels
    x_max = x_min + 0.5 + torch.rand(S, F, generator=g)
    return x_min, x_max


def _history(S, n, seed=11):
    """Raw rows (S, n, F) inside each symbol's own range."""
    g = torch.Generator().manual_seed(seed)
    x_min, x_max = _tables(S)
    u = torch.rand(S, n, F, generator=g)
    return x_min.unsqueeze(1) + u * (x_max - x_min).unsqueeze(1)


@functools.lru_cache(maxsize=None)
def _models3(H=128):
    return tuple(_model(H, seed=k) for k in range(3))


def _bank(models, slots, syms=SYMS6, window=W32, use_graph=True, hist=None):
    from fmda_amd.runtime import BankedFleetPredictor
    x_min, x_max = _tables(len(syms))
    p = BankedFleetPredictor(list(models), syms, slots, x_min, x_max, window,
                             device="cuda:0", dtype=torch.bfloat16,
                             use_graph=use_graph)
    if hist is not None:
        p.warm_start(hist)
    return p


def _probs(res, syms=SYMS6):
    return torch.tensor([res[s]["probabilities"] for s in syms])


def _oracle(models, slots, hist, window):
    """Per slot, the eager model forward over the rows of its symbols."""
    S = hist.shape[0]
    x_min, x_max = _tables(S)
    win = hist[:, -window:]
    x = ((win - x_min.unsqueeze(1)) / (x_max - x_min).unsqueeze(1)
         ).to("cuda", torch.bfloat16)
    out = torch.empty(S, 4)
    with torch.no_grad():
        for m, model in enumerate(models):
            rows = [i for i, k in enumerate(slots) if k == m]
            if rows:
                out[rows] = torch.sigmoid(
                    model.cuda().eval()(x[rows])).float().cpu()
    return out


def test_route_oracle_and_graph_against_eager():
    models = _models3()
    hist = _history(6, 40)
    pg = _bank(models, SLOTS6, hist=hist)
    pe = _bank(models, dict(zip(SYMS6, SLOTS6)), use_graph=False, hist=hist)
    assert pg._gpu_fast and pg.route == "streams_bank"
    assert pe.route == "streams_bank"
    rg = pg.predict_all()
    a, b = _probs(rg), _probs(pe.predict_all())
    assert pg._graph is not None and pg.n_captures == 1
    assert pe._graph is None and pe.n_captures == 0
    assert [rg[s]["model"] for s in SYMS6] == SLOTS6
    ref = _oracle(models, SLOTS6, hist, W32)
    assert a.shape == (6, 4)
    assert torch.allclose(a, ref, atol=2e-2, rtol=0), (a, ref)
    # the same deterministic kernels, captured or not
    assert torch.equal(a, b)
    # the models differ: S0 through model 1 is not S0 through model 0
    other = _oracle(models, [1] * 6, hist, W32)
    assert not torch.allclose(ref[0], other[0], atol=1e-3)


def test_slot_rows_are_the_one_model_bank_bitwise():
    models = _models3()
    hist = _history(6, 40)
    a = _probs(_bank(models, SLOTS6, hist=hist).predict_all())
    for k in range(3):
        one = _probs(_bank([models[k]], [0] * 6, hist=hist).predict_all())
        for i, slot in enumerate(SLOTS6):
            if slot == k:
                assert torch.equal(a[i], one[i]), (k, i)


def test_swap_model_takes_effect_without_recapture():
    models = _models3()
    hist = _history(6, 40)
    p = _bank(models, SLOTS6, hist=hist)
    before = _probs(p.predict_all())
    g = p._graph
    new = _model(128, seed=9)
    p.swap_model(1, new)
    after = _probs(p.predict_all())
    fresh = _probs(_bank([models[0], new, models[2]], SLOTS6,
                         hist=hist).predict_all())
    for i, slot in enumerate(SLOTS6):
        if slot == 1:
            assert not torch.equal(after[i], before[i]), i
            assert torch.equal(after[i], fresh[i]), i
        else:
            assert torch.equal(after[i], before[i]), i
    assert p._graph is g and p.n_captures == 1
    with pytest.raises(ValueError):
        p.swap_model(1, _model(32, seed=9))
    with pytest.raises(ValueError):
        p.swap_model(3, new)
    assert torch.equal(_probs(p.predict_all()), after)


def test_assign_takes_effect_without_recapture():
    models = _models3()
    hist = _history(6, 40)
    p = _bank(models, SLOTS6, hist=hist)
    before = _probs(p.predict_all())
    g = p._graph
    p.assign("S0", 2)
    res = p.predict_all()
    after = _probs(res)
    assert res["S0"]["model"] == 2
    fresh = _probs(_bank(models, [2] + SLOTS6[1:], hist=hist).predict_all())
    assert not torch.equal(after[0], before[0])
    assert torch.equal(after[0], fresh[0])
    for i in range(1, 6):
        assert torch.equal(after[i], before[i]), i
    assert p._graph is g and p.n_captures == 1
    with pytest.raises(ValueError):
        p.assign("S0", 3)
    with pytest.raises(KeyError):
        p.assign("ZZZ", 0)
    assert p._slot_gpu.tolist() == [2] + SLOTS6[1:]
    assert torch.equal(_probs(p.predict_all()), after)


def test_other_hidden_sizes_take_the_grouped_fallback():
    models = _models3(32)
    hist = _history(6, 34)
    p = _bank(models, SLOTS6, hist=hist)
    assert p.route == "grouped" and not p._bank_fast
    res = p.predict_all()
    assert list(res) == SYMS6 and p._graph is None and p.n_captures == 0
    ref = _oracle(models, SLOTS6, hist, W32)
    assert torch.allclose(_probs(res), ref, atol=2e-2, rtol=0)


def test_banked_tick_beats_a_loop_of_fleet_predictors():
    """S = M = 8, window 32: the median of 30 push_rows + predict_all ticks
    (after 5 warm ticks) must be below the median of the same rows pushed
    and predicted through 8 one-symbol FleetPredictors, one per model, one
    after the other: one replay and one sync against eight."""
    from fmda_amd.runtime import FleetPredictor
    S = 8
    syms = [f"S{i}" for i in range(S)]
    models = [_model(128, seed=k) for k in range(S)]
    x_min, x_max = _tables(S)
    hist = _history(S, W32 + 35, seed=4)
    bank = _bank(models, list(range(S)), syms=syms, hist=hist[:, :W32])
    singles = [FleetPredictor(models[i], [syms[i]], x_min[i:i + 1],
                              x_max[i:i + 1], W32, device="cuda:0",
                              dtype=torch.bfloat16, use_graph=True)
               for i in range(S)]
    for i, p in enumerate(singles):
        p.warm_start(hist[i:i + 1, :W32])

    def bank_tick(k):
        bank.push_rows({s: hist[i, k] for i, s in enumerate(syms)})
        return bank.predict_all()

    def loop_tick(k):
        out = {}
        for i, p in enumerate(singles):
            p.push_rows({syms[i]: hist[i, k]})
            out.update(p.predict_all())
        return out

    for k in range(W32, W32 + 5):                        # warm both
        ba, la = bank_tick(k), loop_tick(k)
    # same windows, same models: the two agree (bf16 graph paths)
    assert torch.allclose(_probs(ba, syms), _probs(la, syms), atol=2e-2)
    torch.cuda.synchronize()
    lat = {"bank": [], "loop": []}
    for k in range(W32 + 5, W32 + 35):
        for name, tick in (("bank", bank_tick), ("loop", loop_tick)):
            t0 = time.perf_counter()
            tick(k)
            lat[name].append((time.perf_counter() - t0) * 1000.0)
    p50b = float(np.median(lat["bank"]))
    p50l = float(np.median(lat["loop"]))
    print(f"banked tick p50 {p50b:.3f} ms, {S} fleet predictors p50 "
          f"{p50l:.3f} ms, ratio {p50b / p50l:.3f}")
    assert p50b < p50l, (p50b, p50l)
