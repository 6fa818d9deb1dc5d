"""Windowed table training on the GPU: the window_batch kernel (window
gather + input dropout in one write pass) against indexing and the existing
dropout kernels on the materialised batch, BiGRU.forward_features_windows /
train_windows against the materialised-window step, and resume of the train
driver's windowed_train path. Every comparison is exact."""
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}

# (N, F, T, B). With V = 8 bf16 / 4 fp32 elements per 16-byte vector:
SHAPES = [
    (40, 108, 7, 5),     # 216-byte rows, T*F % 8 = 4: element-wise path
    (11, 5, 3, 4),       # T*F = 15: vectors straddle windows, and a tail
    (9, 8, 9, 1),        # one window = the whole table; 16-byte rows
    (300, 108, 30, 64),  # T*F % 8 == 0, rows 8-byte aligned: 8-byte loads
    # further load widths the launcher can pick
    (20, 6, 4, 7),       # 12-byte bf16 rows: 4-byte loads
    (20, 3, 8, 7),       # 6-byte bf16 rows, T*F % 8 == 0: element loads
    (50, 16, 5, 600),    # more than one block of 256 threads, 16-byte loads
]
PS = [0.003, 0.25, 0.5]
SEEDS = [7, -0x1234567890ABCDEF]


def _ext():
    from fmda_amd.ops import load_extension
    return load_extension()


@functools.lru_cache(maxsize=None)
def _case(dtype, N, F, T, B):
    """Table, starts (unsorted, repeated, with both 0 and N - T) and the
    indexed gather; computed once, shared and never modified."""
    g = torch.Generator().manual_seed(1000 * N + 10 * F + T + B)
    table = (torch.rand(N, F, generator=g) + 0.25).to(_DT[dtype]).cuda()
    starts = torch.randint(0, N - T + 1, (B,), generator=g)
    starts[0] = N - T
    if B >= 2:
        starts[1] = 0
    if B >= 4:
        starts[-1] = starts[2]
    starts = starts.cuda()
    want = table[starts[:, None] + torch.arange(T, device="cuda")].contiguous()
    assert want.shape == (B, T, F)
    return table, starts, want


def _embed(table, front, back=64):
    """The table inside one NaN-filled allocation, `front` elements from
    its start and with `back` NaN rows behind: a view with a storage
    offset whose every out-of-table neighbour is NaN."""
    N, F = table.shape
    flat = torch.full((front + (N + back) * F,), float("nan"),
                      dtype=table.dtype, device="cuda")
    view = flat[front:front + N * F].view(N, F)
    view.copy_(table)
    assert view.storage_offset() == front and view.stride() == (F, 1)
    return view


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("N,F,T,B", SHAPES)
def test_gather_equals_indexing(dtype, N, F, T, B):
    table, starts, want = _case(dtype, N, F, T, B)
    got = _ext().window_batch(table, starts, T, 0.0, 0, False)
    assert got.dtype == table.dtype and got.is_contiguous()
    assert torch.equal(got, want)
    # spatial is ignored without dropout
    assert torch.equal(_ext().window_batch(table, starts, T, 0.0, 5, True),
                       want)


@pytest.mark.parametrize("spatial", [False, True])
@pytest.mark.parametrize("N,F,T,B", SHAPES)
def test_dropout_equals_dropout_kernels_on_gather(N, F, T, B, spatial):
    """Same seed, same drop_params, same draw: bit for bit the existing
    kernels on the materialised batch."""
    table, starts, gathered = _case("bf16", N, F, T, B)
    ext = _ext()
    oracle = ext.spatial_dropout_fused if spatial else ext.dropout_fused
    for p in PS:
        for seed in SEEDS:
            want = oracle(gathered, p, seed)
            got = ext.window_batch(table, starts, T, p, seed, spatial)
            assert torch.equal(got, want), (p, seed)
            if p == 0.5:
                # neither all kept nor all dropped (the data has no zeros)
                zeros = int((got == 0).sum())
                assert 0 < zeros < got.numel(), (p, seed, zeros)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("N,F,T,pad_rows", [
    (40, 108, 7, 64), (40, 108, 7, 65),      # element-wise path
    (70, 108, 30, 64), (70, 108, 30, 65),    # 65 rows: base moves by F*2 B
    (9, 8, 9, 64), (9, 8, 9, 65),
])
def test_no_read_outside_the_table(dtype, N, F, T, pad_rows):
    """NaN rows on both sides of a row-slice view, windows at both ends of
    the table: a read outside the table would put a NaN (dropped: NaN * 0
    is still NaN for kept ones) into the output."""
    g = torch.Generator().manual_seed(N + F + T)
    table = (torch.rand(N, F, generator=g) + 0.25).to(_DT[dtype]).cuda()
    view = _embed(table, pad_rows * F)
    starts = torch.tensor([0, N - T, N - T, 0, (N - T) // 2]).cuda()
    want = table[starts[:, None] + torch.arange(T, device="cuda")]
    ext = _ext()
    got = ext.window_batch(view, starts, T, 0.0, 0, False)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    if dtype == "bf16":
        for spatial in (False, True):
            got = ext.window_batch(view, starts, T, 0.25, 3, spatial)
            oracle = (ext.spatial_dropout_fused if spatial
                      else ext.dropout_fused)
            assert bool(torch.isfinite(got).all())
            assert torch.equal(got, oracle(want.contiguous(), 0.25, 3))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("front", [1, 2, 3, 4, 8])
def test_load_width_follows_base_alignment(dtype, front):
    """16-byte rows (bf16 F = 8, fp32 F = 4) whose base sits `front`
    elements into the allocation: the rows allow 16-byte loads, the base
    address does not, down to a single element."""
    F = 8 if dtype == "bf16" else 4
    N, T = 21, 6
    g = torch.Generator().manual_seed(front)
    table = (torch.rand(N, F, generator=g) + 0.25).to(_DT[dtype]).cuda()
    view = _embed(table, front)
    starts = torch.tensor([N - T, 0, 5, 5, 1, 0, N - T]).cuda()
    want = table[starts[:, None] + torch.arange(T, device="cuda")]
    got = _ext().window_batch(view, starts, T, 0.0, 0, False)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_binding_rejects_bad_calls():
    ext = _ext()
    table, starts, _ = _case("bf16", 11, 5, 3, 4)
    t32 = table.float()
    bad = (RuntimeError, TypeError, ValueError)
    with pytest.raises(bad):
        ext.window_batch(t32, starts, 3, 0.5, 1, False)    # fp32 dropout
    with pytest.raises(bad):
        ext.window_batch(table, starts, 12, 0.0, 0, False)  # window > N
    with pytest.raises(bad):
        ext.window_batch(table, starts, 0, 0.0, 0, False)
    with pytest.raises(bad):
        ext.window_batch(table, starts.int(), 3, 0.0, 0, False)
    with pytest.raises(bad):
        ext.window_batch(table, starts.cpu(), 3, 0.0, 0, False)
    with pytest.raises(bad):
        ext.window_batch(table.cpu(), starts, 3, 0.0, 0, False)
    with pytest.raises(bad):
        ext.window_batch(table, starts[:0], 3, 0.0, 0, False)  # B = 0
    with pytest.raises(bad):
        ext.window_batch(table[:, :4], starts, 3, 0.0, 0, False)  # pitch
    with pytest.raises(bad):
        ext.window_batch(table.half(), starts, 3, 0.0, 0, False)
    with pytest.raises(bad):
        ext.window_batch(table, starts, 3, 1.0, 0, False)


@pytest.mark.parametrize("bad_starts", [[9], [-1], [0, 8, 9], [0, -1, 3]])
def test_interface_rejects_out_of_range_cpu_starts(bad_starts):
    from fmda_amd.ops.interface import window_batch
    table, _, _ = _case("bf16", 11, 5, 3, 4)      # N - T = 8
    with pytest.raises(ValueError):
        window_batch(table, torch.tensor(bad_starts), 3, p=0.5)
    with pytest.raises(ValueError):
        window_batch(table, torch.tensor([0]), 12)
    with pytest.raises(TypeError):
        window_batch(table, torch.tensor([0], dtype=torch.int32), 3)


def test_interface_paths_agree(monkeypatch):
    """CPU starts are uploaded; fp32 with p > 0 gathers with the kernel and
    takes torch's dropout; FMDA_NATIVE_GLUE=0 gives the same bits."""
    from fmda_amd.ops.interface import window_batch
    table, starts, want = _case("bf16", 300, 108, 30, 64)
    ext = _ext()
    assert torch.equal(window_batch(table, starts.cpu(), 30), want)
    for spatial in (False, True):
        oracle = ext.spatial_dropout_fused if spatial else ext.dropout_fused
        got = window_batch(table, starts, 30, p=0.5, spatial=spatial, seed=9)
        assert torch.equal(got, oracle(want, 0.5, 9))
        torch.manual_seed(4)
        a = window_batch(table, starts, 30, p=0.5, spatial=spatial)
        monkeypatch.setenv("FMDA_NATIVE_GLUE", "0")
        torch.manual_seed(4)
        b = window_batch(table, starts, 30, p=0.5, spatial=spatial)
        assert torch.equal(
            window_batch(table, starts, 30, p=0.5, spatial=spatial, seed=9),
            got)
        monkeypatch.delenv("FMDA_NATIVE_GLUE")
        assert torch.equal(a, b)
    t32, s32, w32 = _case("fp32", 300, 108, 30, 64)
    got = window_batch(t32, s32, 30, p=0.5)
    kept = got != 0
    assert 0 < int(kept.sum()) < got.numel()
    assert torch.equal(got[kept], (w32 * 2.0)[kept])


# --------------------------------------------------------------------- #
# model level
# --------------------------------------------------------------------- #

def _model(dtype, p, spatial=False, seed=3):
    from fmda_amd.models import BiGRU
    from fmda_amd.optim import FusedClipAdam
    torch.manual_seed(seed)
    dev = torch.device("cuda")
    model = BiGRU(32, 12, 4, n_layers=2, dropout=p, clip=0.25,
                  spatial_dropout=spatial).to(dev)
    model.add_loss_fn(nn.BCEWithLogitsLoss(
        weight=torch.tensor([1.0, 2.0, 0.5, 1.5], device=dev),
        pos_weight=torch.tensor([3.0, 1.0, 2.0, 0.75], device=dev)))
    model.add_optimizer(FusedClipAdam(model.parameters(), lr=1e-3,
                                      clip=model.clip))
    model.add_device(dev)
    return model


@functools.lru_cache(maxsize=None)
def _train_table(dtype):
    g = torch.Generator().manual_seed(21)
    table = torch.rand(80, 12, generator=g).to(_DT[dtype]).cuda()
    targets = (torch.rand(80, 4, generator=g) < 0.4).float().cuda()
    return table, targets


@pytest.mark.parametrize("spatial", [False, True])
def test_forward_features_windows_equals_materialised(spatial):
    model = _model("bf16", 0.5, spatial).train()
    table, _ = _train_table("bf16")
    g = torch.Generator().manual_seed(2)
    starts = torch.randint(0, 80 - 8 + 1, (16,), generator=g).cuda()
    x = table[starts[:, None] + torch.arange(8, device="cuda")]
    for s in (0, 1):
        torch.manual_seed(s)
        got = model.forward_features_windows(table, starts, 8)
        torch.manual_seed(s)
        want = model.forward_features(x)
        assert got.shape == (16, 96)
        assert torch.equal(got, want), s
    # eval mode: a plain gather
    model.eval()
    with torch.no_grad():
        assert torch.equal(model.forward_features_windows(table, starts, 8),
                           model.forward_features(x))


@pytest.mark.parametrize("dtype,p", [("bf16", 0.5), ("fp32", 0.0)])
def test_train_windows_equals_hand_loop(dtype, p):
    """train_windows against the benched step written out by hand over the
    unfolded table: forward_features, fused_head_loss, backward,
    FusedClipAdam.step. 73 windows in batches of 16: a last batch of 9."""
    from fmda_amd.ops.interface import fused_head_loss
    table, targets = _train_table(dtype)
    window, batch = 8, 16

    a = _model(dtype, p)
    torch.manual_seed(17)
    _, _, losses_a, _ = a.train_windows(table, targets, window, batch)

    b = _model(dtype, p).train()
    wins = table.unfold(0, window, 1).permute(0, 2, 1).contiguous()
    torch.manual_seed(17)
    losses_b = []
    for b0 in range(0, wins.shape[0], batch):
        y = targets[window - 1 + b0:window - 1 + b0 + batch]
        b.optimizer.zero_grad()
        feats = b.forward_features(wins[b0:b0 + batch])
        loss, _ = fused_head_loss(feats, b.linear.weight, b.linear.bias, y,
                                  b.loss_fn.weight, b.loss_fn.pos_weight)
        loss.backward()
        b.optimizer.step()
        losses_b.append(loss.detach())
    losses_b = torch.stack(losses_b).cpu().numpy()

    assert len(losses_a) == len(losses_b) == 5
    assert [float(v) for v in losses_a] == [float(v) for v in losses_b]
    fresh = _model(dtype, p)
    for (k, va), vb, v0 in zip(a.state_dict().items(),
                               b.state_dict().values(),
                               fresh.state_dict().values()):
        assert torch.equal(va, vb), k
        if not k.startswith("loss_fn."):
            assert not torch.equal(va, v0), k     # it did train


def test_train_resume_through_fused_path(tmp_path):
    """train(2 epochs) == train(1) + resume(1 more) with windowed_train on
    the GPU, bit for bit; the sidecar carries FusedClipAdam's state."""
    from fmda_amd.config import DataConfig, ModelConfig, TrainConfig
    from fmda_amd.optim import FusedClipAdam
    from fmda_amd.train import train
    mcfg = ModelConfig(hidden_size=32, n_features=16, n_layers=2,
                       spatial_dropout=False, dropout=0.25)
    dcfg = DataConfig(n_rows=330, chunk_size=60, window=10, seed=3,
                      n_features=16)

    def run(name, epochs, resume=None):
        tcfg = TrainConfig(batch_size=16, epochs=epochs, device="cuda",
                           dtype="bf16", windowed_train=True)
        ck = str(tmp_path / f"{name}.pt")
        model, hist = train(mcfg, dcfg, tcfg, checkpoint_path=ck,
                            norm_params_path=str(tmp_path / f"{name}.np"),
                            log=lambda s: None, resume=resume)
        return model, hist, ck

    model_a, hist_a, _ = run("a", 2)
    assert isinstance(model_a.optimizer, FusedClipAdam)
    _, _, ck_b = run("b", 1)
    ts = torch.load(ck_b + ".train_state.pt", weights_only=False)
    assert set(ts["optimizer"]) == {"step", "m", "v"}
    assert ts["optimizer"]["step"] > 0
    model_b, hist_b, _ = run("b", 2, resume=ck_b)
    assert [r["epoch"] for r in hist_a] == [1, 2]
    assert [r["epoch"] for r in hist_b] == [2]
    assert hist_a[1]["train_loss"] == hist_b[0]["train_loss"]
    sa, sb = model_a.state_dict(), model_b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
