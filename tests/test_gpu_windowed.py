"""Windowed table inference on the GPU: the forward recurrence kernels
reading sliding windows straight from a table of per-row projections
(gru_fwd_windows), the normalize_table kernel, and BiGRU.forward_windows
against the materialised-window forward."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}

# (dtype, H, T, B, n_dir, stride): every forward kernel family
CASES = [
    ("fp32", 32, 12, 33, 2, 1),     # generic
    ("fp32", 64, 9, 20, 1, 3),      # generic
    ("bf16", 32, 12, 33, 2, 1),     # generic
    ("bf16", 256, 10, 17, 2, 2),    # generic
    ("bf16", 128, 20, 40, 2, 1),    # v3, ragged last tile
    ("bf16", 128, 20, 19, 1, 1),    # v3
    ("bf16", 512, 8, 16, 2, 1),     # column-split
    ("bf16", 512, 6, 20, 2, 5),     # column-split
    ("bf16", 128, 30, 1, 2, 1),     # batch-1 kernel
    ("bf16", 32, 5, 6, 2, 7),       # stride > T
]


def _ext():
    from fmda_amd.ops import load_extension
    return load_extension()


@functools.lru_cache(maxsize=None)
def _case(dtype, H, T, B, n_dir, stride):
    """Inputs of one case and the materialised-window result, computed once
    and shared (never modified) by the tests below."""
    dt = _DT[dtype]
    g = torch.Generator().manual_seed(1000 * H + 10 * T + B + stride)
    R = (B - 1) * stride + T
    gi_rows = (torch.randn(R, n_dir * 3 * H, generator=g) * 0.5).to(dt).cuda()
    w = (torch.randn(n_dir, 3 * H, H, generator=g) * 0.2).to(dt).cuda()
    bhh = (torch.randn(n_dir, 3 * H, generator=g) * 0.1).cuda()
    dense = gi_rows.unfold(0, T, stride).permute(0, 2, 1).contiguous()
    assert dense.shape == (B, T, n_dir * 3 * H)
    out, hlast = _ext().gru_fwd(dense, w, bhh)
    return gi_rows, w, bhh, out, hlast


def _check(res, out, hlast):
    assert res[0].shape == out.shape and res[1].shape == hlast.shape
    assert res[0].dtype == out.dtype and res[1].dtype == torch.float32
    assert torch.equal(res[0], out), \
        (res[0].float() - out.float()).abs().max()
    assert torch.equal(res[1], hlast), (res[1] - hlast).abs().max()


@pytest.mark.parametrize("dtype,H,T,B,n_dir,stride", CASES)
def test_windows_bitwise_equal_materialised(dtype, H, T, B, n_dir, stride):
    """Same kernel, tiles and arithmetic, only the gi addresses differ."""
    gi_rows, w, bhh, out, hlast = _case(dtype, H, T, B, n_dir, stride)
    _check(_ext().gru_fwd_windows(gi_rows, w, bhh, T, stride), out, hlast)


@pytest.mark.parametrize("case", [("fp32", 64, 9, 20, 1, 3),
                                  ("bf16", 512, 6, 20, 2, 5)])
def test_windows_trailing_rows_ignored(case):
    """Two rows more than (B-1)*stride + T make no further window at
    stride >= 3: B is unchanged and the extra rows are never read."""
    gi_rows, w, bhh, out, hlast = _case(*case)
    T, stride = case[2], case[5]
    longer = torch.cat([gi_rows, torch.full_like(gi_rows[:2], float("nan"))])
    _check(_ext().gru_fwd_windows(longer, w, bhh, T, stride), out, hlast)


def test_windows_accept_row_slice():
    gi_rows, w, bhh, out, hlast = _case("bf16", 128, 20, 40, 2, 1)
    R = gi_rows.shape[0]
    big = torch.zeros(R + 9, gi_rows.shape[1], dtype=gi_rows.dtype,
                      device="cuda")
    big[5:5 + R] = gi_rows
    view = big[5:5 + R]
    assert view.data_ptr() != big.data_ptr()
    _check(_ext().gru_fwd_windows(view, w, bhh, 20, 1), out, hlast)


@pytest.mark.parametrize("dtype,H,T,B,n_dir,stride", CASES)
def test_windows_read_no_row_outside_table(dtype, H, T, B, n_dir, stride):
    """The table sits between NaN rows of one allocation: a read before the
    first or past the last row would poison the outputs."""
    gi_rows, w, bhh, out, hlast = _case(dtype, H, T, B, n_dir, stride)
    R, pad = gi_rows.shape[0], 64
    big = torch.full((R + 2 * pad, gi_rows.shape[1]), float("nan"),
                     dtype=gi_rows.dtype, device="cuda")
    big[pad:pad + R] = gi_rows
    res = _ext().gru_fwd_windows(big[pad:pad + R], w, bhh, T, stride)
    assert torch.isfinite(res[0].float()).all()
    assert torch.isfinite(res[1]).all()
    _check(res, out, hlast)


@pytest.mark.parametrize("shape", [(37, 108), (1, 5)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_normalize_table_matches_batchloader_formula(shape, dtype):
    N, F = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, F, generator=g) * 50.0 + 10.0
    x[torch.rand(N, F, generator=g) < 0.1] = float("nan")
    x[0, 1] = float("nan")
    x[:, 2] = 7.25                       # constant column
    clean = torch.nan_to_num(x, nan=0.0)
    mn = clean.min(dim=0).values
    mx = clean.max(dim=0).values
    # MIN == MAX epsilon rule of ChunkLoader
    eq = mn == mx
    assert bool(eq[2])
    mx[eq & (mx != 0)] += mx[eq & (mx != 0)] * 0.001
    mx[eq & (mx == 0)] += 0.001
    x, mn, mx = x.cuda(), mn.cuda(), mx.cuda()
    want = ((torch.nan_to_num(x, nan=0.0) - mn) / (mx - mn)).to(_DT[dtype])
    got = _ext().normalize_table(x, mn, mx, _DT[dtype])
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.isfinite(want.float()).all()
    assert torch.equal(got, want), (got.float() - want.float()).abs().max()


def _unfolded(table, window, stride):
    return table.unfold(0, window, stride).permute(0, 2, 1).contiguous()


@pytest.mark.parametrize("hidden,layers,bidir,stride", [
    (32, 2, True, 1), (32, 2, True, 3), (8, 1, False, 1)])
def test_forward_windows_fp32_matches_cpu(hidden, layers, bidir, stride):
    """26 windows (stride 1) in chunks of 8: three full chunks and a ragged
    one. Tolerance of test_bigru_model_gpu_matches_cpu (same model)."""
    from fmda_amd.models import BiGRU
    torch.manual_seed(7)
    m = BiGRU(hidden, 24, 4, n_layers=layers, spatial_dropout=False,
              dropout=0.0, bidirectional=bidir).eval()
    table = torch.randn(40, 24)
    window = 15
    with torch.no_grad():
        ref = m(_unfolded(table, window, stride))
    got = m.cuda().forward_windows(table.cuda(), window, stride=stride,
                                   batch_windows=8).cpu()
    assert got.shape == ref.shape
    if stride == 1:
        assert got.shape[0] == 26
    assert torch.allclose(ref, got, atol=5e-4), (ref - got).abs().max()


def test_forward_windows_bf16_no_worse_than_materialised():
    """bf16, H128 L2 F96, table (60, 96), window 20, chunks of 16 windows.
    Oracle: the CPU fp32 model on the unfolded windows. e_mat / e_win are
    the max abs logit errors of the materialised GPU forward and of
    forward_windows: maxima of the same bf16 rounding noise (the two differ
    only in the projection GEMM's shape), so e_win <= 2 * e_mat; an
    addressing mistake gives O(1) errors. Measured values are recorded in
    profiles/windowed_eval.md."""
    from fmda_amd.models import BiGRU
    torch.manual_seed(9)
    m = BiGRU(128, 96, 4, n_layers=2, spatial_dropout=False,
              dropout=0.0).eval()
    table = torch.rand(60, 96)
    window = 20
    wins = _unfolded(table, window, 1)
    with torch.no_grad():
        ref = m(wins)
        m.cuda()
        mat = m(wins.cuda().bfloat16()).float().cpu()
    win = m.forward_windows(table.cuda().bfloat16(), window,
                            batch_windows=16).float().cpu()
    assert win.shape == ref.shape == (41, 4)
    e_mat = float((mat - ref).abs().max())
    e_win = float((win - ref).abs().max())
    print(f"windowed bf16: e_mat={e_mat:.6g} e_win={e_win:.6g}")
    assert e_mat > 0.0
    assert e_win <= 2 * e_mat, (e_win, e_mat)


def test_bad_arguments_are_rejected_cleanly():
    from fmda_amd.models import BiGRU
    gi_rows, w, bhh, _, _ = _case("bf16", 32, 12, 33, 2, 1)
    ext = _ext()
    with pytest.raises(RuntimeError):
        ext.gru_fwd_windows(gi_rows, w, bhh, 12, 0)
    with pytest.raises(RuntimeError):
        ext.gru_fwd_windows(gi_rows, w, bhh, gi_rows.shape[0] + 1, 1)
    with pytest.raises(RuntimeError):
        ext.gru_fwd_windows(gi_rows[:, :-8], w, bhh, 12, 1)
    m = BiGRU(32, 24, 4, n_layers=1, spatial_dropout=False).cuda().train()
    with pytest.raises(AssertionError):
        m.forward_windows(torch.randn(40, 24, device="cuda"), 15)
    torch.cuda.synchronize()


def test_windowed_chunk_evaluation_on_gpu_matches_dataloader_path():
    """The train driver's helper on a GPU model: every chunk normalised by
    normalize_table equals BatchLoader's CPU normalisation bit for bit
    (both are correctly rounded fp32), and the 5-tuple equals
    evaluate_model over the materialised batches on the same model."""
    import numpy as np
    from fmda_amd.config import DataConfig
    from fmda_amd.data import BatchLoader, SyntheticMarket
    from fmda_amd.models import BiGRU
    from fmda_amd.train import (chunk_batches, evaluate_chunks_windowed,
                                make_epoch_sets)
    dcfg = DataConfig(n_rows=260, chunk_size=60, window=10, seed=2,
                      n_features=16)
    market = SyntheticMarket(dcfg.n_rows, seed=dcfg.seed)
    X = market.X[:, :16]
    for indices, norms in make_epoch_sets(market, dcfg)[0]:
        bl = BatchLoader(indices, norms, X, market.Y, dcfg.window)
        ids = torch.tensor(list(indices)) - 1
        got = _ext().normalize_table(X[ids].contiguous().cuda(),
                                     norms[0][0].cuda(), norms[1][0].cuda(),
                                     torch.float32)
        assert torch.equal(got.cpu(), bl.x)

    torch.manual_seed(11)
    model = BiGRU(8, 16, 4, n_layers=1, spatial_dropout=False,
                  dropout=0.0).cuda()
    with torch.no_grad():
        model.linear.bias.add_(0.05)
    model.add_device(torch.device("cuda"))
    train_set = make_epoch_sets(market, dcfg)[0]
    want = model.evaluate_model(chunk_batches(market, train_set, dcfg, 7))
    train_set = make_epoch_sets(market, dcfg)[0]
    got = evaluate_chunks_windowed(model, market, train_set, dcfg, 7)
    assert want[3].shape[0] > 60          # more than one chunk
    assert 0 < int(want[3].sum()) < want[3].numel()
    assert torch.equal(got[4], want[4])
    assert torch.equal(got[3], want[3])
    for g, w in zip(got[:3], want[:3]):
        assert np.allclose(g, w, rtol=1e-12, atol=1e-15)
