"""GPU fleet-predictor tests: the multi-stream batch-1 recurrence, the
batched ingest kernel and the one-replay-per-tick FleetPredictor."""
import functools
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HP = 128
S_MAX = 17


def _ext():
    from fmda_amd.ops import load_extension
    return load_extension()


# ---------------- gru_fwd_streams ----------------

@functools.lru_cache(maxsize=None)
def _streams_case(T, n_dir):
    """Inputs for S_MAX streams and, per stream, what the existing batch-1
    kernel (gru_fwd at B = 1) gives on that stream's slice. Computed once
    per (T, n_dir) and shared by every S of the sweep."""
    ext = _ext()
    g = torch.Generator().manual_seed(1000 * T + n_dir)
    # |gi| < ~1 and |W_hh h| < ~1 keep the gates off saturation
    gi = (torch.randn(S_MAX, T, n_dir * 3 * HP, generator=g) * 0.5
          ).to("cuda", torch.bfloat16)
    w = (torch.randn(n_dir, 3 * HP, HP, generator=g) * 0.08
         ).to("cuda", torch.bfloat16)
    bhh = (torch.randn(n_dir, 3 * HP, generator=g) * 0.1).cuda()
    ref = [ext.gru_fwd(gi[s:s + 1].contiguous(), w, bhh)
           for s in range(S_MAX)]
    ref_out = torch.cat([r[0] for r in ref], dim=0)        # (S, T, D*Hp)
    ref_hl = torch.cat([r[1] for r in ref], dim=1)         # (D, S, Hp)
    assert not torch.isnan(ref_out.float()).any()
    return gi, w, bhh, ref_out, ref_hl


@pytest.mark.parametrize("n_dir", [1, 2])
@pytest.mark.parametrize("T", [1, 2, 3, 32])
@pytest.mark.parametrize("S", [1, 2, 3, 17])
def test_gru_fwd_streams_is_bitwise_the_batch1_kernel(S, T, n_dir):
    ext = _ext()
    gi, w, bhh, ref_out, ref_hl = _streams_case(T, n_dir)
    gi_s = gi[:S].contiguous()
    # the binding allocates its outputs; poison the blocks the caching
    # allocator will hand it, so an unwritten row or a stream writing into
    # a neighbour's slab shows as NaN / a mismatch rather than stale data
    poison = [torch.full((S, T, n_dir * HP), float("nan"), device="cuda",
                         dtype=torch.bfloat16),
              torch.full((n_dir, S, HP), float("nan"), device="cuda")]
    torch.cuda.synchronize()
    del poison
    out, hl = ext.gru_fwd_streams(gi_s, w, bhh)
    assert out.shape == (S, T, n_dir * HP) and out.dtype == torch.bfloat16
    assert hl.shape == (n_dir, S, HP) and hl.dtype == torch.float32
    assert torch.equal(out, ref_out[:S])
    assert torch.equal(hl, ref_hl[:, :S].contiguous())


def test_gru_fwd_streams_binding_checks():
    ext = _ext()
    gi, w, bhh, _, _ = _streams_case(2, 2)
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams(gi.float(), w, bhh)                 # dtype
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams(gi[:, :, :-8], w, bhh)              # contiguity
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams(gi[:, :, :3 * HP].contiguous(), w, bhh)  # shape
    with pytest.raises(RuntimeError):
        ext.gru_fwd_streams(gi, w, bhh.to(torch.bfloat16))
    # above the 150 KB LDS cap nothing is launched: 2*T*392 + 2080 bytes
    t_over = (150 * 1024 - 2080) // (2 * 392) + 1
    big = torch.zeros(1, t_over, 2 * 3 * HP, device="cuda",
                      dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="LDS"):
        ext.gru_fwd_streams(big, w, bhh)


# ---------------- ingest_rows ----------------

def _ingest_case(S, T, F, mask, seed):
    g = torch.Generator().manual_seed(seed)
    rings = torch.rand(S, T, F, generator=g).to("cuda", torch.bfloat16)
    rows = (torch.rand(S, F, generator=g) * 50.0).cuda()
    xmin = (torch.rand(S, F, generator=g) * 10.0).cuda()
    xrng = (0.5 + torch.rand(S, F, generator=g) * 40.0).cuda()
    active = torch.tensor(mask, dtype=torch.int32, device="cuda")
    return rings, rows, active, xmin, xrng


def _check_ingest(S, T, F, mask, seed):
    ext = _ext()
    rings, rows, active, xmin, xrng = _ingest_case(S, T, F, mask, seed)
    before = rings.clone()
    ext.ingest_rows(rings, rows, active, xmin, xrng)
    for s in range(S):
        if mask[s]:
            want = before[s].clone()
            ext.ingest_row(want, rows[s].contiguous(), xmin[s].contiguous(),
                           xrng[s].contiguous())
            assert not torch.equal(want, before[s])
        else:
            want = before[s]
        # bitwise: compare the raw 16-bit patterns
        assert torch.equal(rings[s].view(torch.int16),
                           want.view(torch.int16)), s


def test_ingest_rows_matches_ingest_row_and_skips_inactive():
    _check_ingest(5, 4, 96, [1, 0, 1, 1, 0], seed=1)


def test_ingest_rows_at_the_one_workgroup_bound():
    T, F = 513, 96
    assert (T - 1) * F == 48 * 1024
    _check_ingest(3, T, F, [1, 0, 1], seed=2)
    ext = _ext()
    rings, rows, active, xmin, xrng = _ingest_case(2, T + 1, F, [1, 1], 3)
    before = rings.clone()
    with pytest.raises(RuntimeError, match="bound"):
        ext.ingest_rows(rings, rows, active, xmin, xrng)
    assert torch.equal(rings, before)


def test_ingest_rows_binding_checks():
    ext = _ext()
    rings, rows, active, xmin, xrng = _ingest_case(3, 4, 16, [1, 1, 1], 4)
    with pytest.raises(RuntimeError):
        ext.ingest_rows(rings.float(), rows, active, xmin, xrng)
    with pytest.raises(RuntimeError):
        ext.ingest_rows(rings, rows[:2].contiguous(), active, xmin, xrng)
    with pytest.raises(RuntimeError):
        ext.ingest_rows(rings, rows, active.long(), xmin, xrng)
    with pytest.raises(RuntimeError):
        ext.ingest_rows(rings, rows, active, xmin[0].contiguous(), xrng)
    with pytest.raises(RuntimeError):
        ext.ingest_rows(rings, rows, active, xmin, xrng.t())


# ---------------- FleetPredictor ----------------

F = 96
SYMS6 = [f"S{i}" for i in range(6)]


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


def _fleet(model, syms, window, use_graph=True):
    from fmda_amd.runtime import FleetPredictor
    x_min, x_max = _tables(len(syms))
    return FleetPredictor(model, syms, x_min, x_max, window,
                          device="cuda:0", dtype=torch.bfloat16,
                          use_graph=use_graph)


def _history(S, n, seed=11):
    """Raw rows (S, n, F) inside each symbol's own range."""
    g = torch.Generator().manual_seed(seed)
    x_min, x_max = _tables(S)
    u = torch.rand(S, n, F, generator=g)
    return x_min.unsqueeze(1) + u * (x_max - x_min).unsqueeze(1)


def _probs(res, syms):
    return torch.tensor([res[s]["probabilities"] for s in syms])


def _oracle(model, hist, window):
    S = hist.shape[0]
    x_min, x_max = _tables(S)
    win = hist[:, -window:]
    x_norm = (win - x_min.unsqueeze(1)) / (x_max - x_min).unsqueeze(1)
    with torch.no_grad():
        return torch.sigmoid(model.cuda().eval()(
            x_norm.to("cuda", torch.bfloat16))).float().cpu()


def test_fast_path_matches_eager_and_model_forward():
    m = _model(128)
    hist = _history(6, 40)
    pg = _fleet(m, SYMS6, 32, use_graph=True)
    pe = _fleet(m, SYMS6, 32, use_graph=False)
    assert pg._gpu_fast and pg.route == "streams"
    # warm_start on one, row-by-row partial pushes on the other
    pg.warm_start(hist)
    for k in range(40):
        pe.push_rows({s: hist[i, k] for i, s in enumerate(SYMS6[:3])})
        pe.push_rows({s: hist[i + 3, k] for i, s in enumerate(SYMS6[3:])})
    assert torch.equal(pg._rings_gpu, pe._rings_gpu)
    a = _probs(pg.predict_all(), SYMS6)
    b = _probs(pe.predict_all(), SYMS6)
    ref = _oracle(m, hist, 32)
    assert a.shape == (6, 4)
    assert torch.allclose(a, b, atol=1e-3, rtol=0), (a, b)
    assert torch.allclose(a, ref, atol=2e-2, rtol=0), (a, ref)
    assert torch.allclose(b, ref, atol=2e-2, rtol=0), (b, ref)
    # distinct tables matter: the symbols do not all score alike
    assert not torch.equal(a[0], a[1])

    # a new row for ONE symbol moves that symbol only; the rest replay to
    # the same bits (independent streams, deterministic replay)
    x_min, x_max = _tables(6)
    pg.push_row("S2", x_min[2] + 0.05 * (x_max[2] - x_min[2]))
    a2 = _probs(pg.predict_all(), SYMS6)
    assert not torch.equal(a2[2], a[2])
    for i in (0, 1, 3, 4, 5):
        assert (a2[i] == a[i]).all(), i


@pytest.mark.parametrize("H,env", [(128, "0"), (32, None)])
def test_gru_fwd_route_matches_model_forward(H, env, monkeypatch):
    if env is not None:
        monkeypatch.setenv("FMDA_FLEET_B1", env)
    m = _model(H, seed=3)
    hist = _history(6, 34)
    p = _fleet(m, SYMS6, 32)
    assert p._gpu_fast and p.route == "gru_fwd"
    p.warm_start(hist)
    a = _probs(p.predict_all(), SYMS6)
    ref = _oracle(m, hist, 32)
    assert torch.allclose(a, ref, atol=2e-2, rtol=0), (a, ref)


def test_route_follows_the_cu_count(monkeypatch):
    """One (direction, stream) block per CU: a fleet whose grid needs a
    second round goes to the batch-tiled kernel (the measured crossover);
    FMDA_FLEET_B1=1 still forces the streams kernel. Both score alike."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    S = n_cu // 2 + 1
    syms = [f"S{i}" for i in range(S)]
    m = _model(128, seed=6)
    hist = _history(S, 5)
    ref = _oracle(m, hist, 4)
    monkeypatch.delenv("FMDA_FLEET_B1", raising=False)
    assert _fleet(m, syms[:-1], 4).route == "streams"     # 2*(S-1) <= n_cu
    p = _fleet(m, syms, 4)
    assert p.route == "gru_fwd"
    monkeypatch.setenv("FMDA_FLEET_B1", "1")
    q = _fleet(m, syms, 4)
    assert q.route == "streams"
    for f in (p, q):
        f.warm_start(hist)
        assert torch.allclose(_probs(f.predict_all(), syms), ref,
                              atol=2e-2, rtol=0)


def test_padded_hidden_takes_the_captured_model_fallback():
    m = _model(8, L=1, seed=5)
    p = _fleet(m, SYMS6, 5)
    assert not p._gpu_fast and p.route == "model"
    p.warm_start(_history(6, 6))
    res = p.predict_all()
    assert list(res) == SYMS6 and p._graph is not None
    ref = _oracle(m, _history(6, 6), 5)
    assert torch.allclose(_probs(res, SYMS6), ref, atol=2e-2, rtol=0)


def test_graph_captured_once_partial_tick_does_not_recapture():
    m = _model(128)
    p = _fleet(m, SYMS6, 32)
    p.warm_start(_history(6, 32))
    r0 = p.predict_all()
    g1 = p._graph
    assert g1 is not None and p.n_captures == 1
    x_min, x_max = _tables(6)
    p.push_rows({"S1": x_min[1], "S4": x_max[4]})       # 2 of 6 symbols
    r1 = p.predict_all()
    p.push_rows({s: x_max[i] for i, s in enumerate(SYMS6)})
    p.predict_all()
    assert p._graph is g1 and p.n_captures == 1
    assert list(r1) == SYMS6
    assert r1["S0"]["probabilities"] == r0["S0"]["probabilities"]
    assert r1["S1"]["probabilities"] != r0["S1"]["probabilities"]


def test_fleet_tick_beats_the_serial_loop_it_replaces():
    """S=8, window 32: p50 of 100 push_rows + predict_all ticks must be
    below the p50 of the same 8 rows pushed and predicted through 8
    StreamingPredictors one after the other, in the same process."""
    from fmda_amd.runtime import StreamingPredictor
    S, W = 8, 32
    syms = [f"S{i}" for i in range(S)]
    m = _model(128)
    x_min, x_max = _tables(S)
    hist = _history(S, W + 110, seed=4)
    fleet = _fleet(m, syms, W)
    singles = [StreamingPredictor(m, x_min[i], x_max[i], W, device="cuda:0",
                                  dtype=torch.bfloat16, use_graph=True)
               for i in range(S)]
    fleet.warm_start(hist[:, :W])
    for k in range(W):
        for i, p in enumerate(singles):
            p.push_row(hist[i, k])

    def fleet_tick(k):
        fleet.push_rows({s: hist[i, k] for i, s in enumerate(syms)})
        return fleet.predict_all()

    def serial_tick(k):
        out = {}
        for i, p in enumerate(singles):
            p.push_row(hist[i, k])
            out[syms[i]] = p.predict_window()
        return out

    for k in range(W, W + 10):                           # warm both
        fa, sa = fleet_tick(k), serial_tick(k)
    # same windows, same model: the two agree (bf16 graph paths)
    assert torch.allclose(_probs(fa, syms), _probs(sa, syms), atol=1e-3)
    torch.cuda.synchronize()
    lat = {"fleet": [], "serial": []}
    for k in range(W + 10, W + 110):
        for name, tick in (("fleet", fleet_tick), ("serial", serial_tick)):
            t0 = time.perf_counter()
            tick(k)
            lat[name].append((time.perf_counter() - t0) * 1000.0)
    p50f = float(np.percentile(lat["fleet"], 50))
    p50s = float(np.percentile(lat["serial"], 50))
    print(f"fleet tick p50 {p50f:.3f} ms, serial x{S} p50 {p50s:.3f} ms, "
          f"ratio {p50f / p50s:.3f}")
    assert p50f < p50s, (p50f, p50s)
