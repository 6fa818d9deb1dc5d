"""Windowed table training on CPU: BiGRU.train_windows and the train
driver's windowed_train switch against the default path (BatchLoader ->
DataLoader -> train_model), ops.interface.window_batch on CPU tensors, and
the command-line flags."""
import json

import pytest
import torch
import torch.nn as nn

from fmda_amd.config import DataConfig, ModelConfig, TrainConfig
from fmda_amd.data import SyntheticMarket
from fmda_amd.models import BiGRU
from fmda_amd.ops.interface import window_batch
from fmda_amd.train import (build_parser, chunk_batches, configs_from_args,
                            make_epoch_sets, train, train_chunks_windowed)


def _trainable(n_features=12, hidden=8, dropout=0.0):
    torch.manual_seed(11)
    model = BiGRU(hidden, n_features, 4, n_layers=1, spatial_dropout=False,
                  dropout=dropout)
    model.add_loss_fn(nn.BCEWithLogitsLoss())
    model.add_optimizer(torch.optim.Adam(model.parameters(), lr=1e-3))
    model.add_device(torch.device("cpu"))
    return model


def _record_batches(model):
    """Every (input, target) batch a training run of `model` forms, in
    order: inputs from the forward call (the training loops call
    model.forward directly), targets from the loss call."""
    xs, ys = [], []
    inner = model.forward

    def forward(input_seq, hidden=None):
        xs.append(input_seq.detach().clone())
        return inner(input_seq, hidden)
    model.forward = forward
    model.loss_fn.register_forward_pre_hook(
        lambda mod, args: ys.append(args[1].detach().clone()))
    return xs, ys


def test_train_windowed_equals_default_path(tmp_path):
    """train() with windowed_train gives the default path's history and a
    bit-identical final state_dict on CPU: same batches, same step.

    dropout must be 0.0 here: every DataLoader iterator of the default path
    draws a base seed from the global RNG, the windowed path has no
    DataLoader, so with dropout on the two paths would consume the RNG
    differently and draw different masks.

    11 chunks of 60 rows, 8 of them for training; chunk 0 has 41 windows,
    so batches of 4 leave a final partial batch of 1."""
    mcfg = ModelConfig(hidden_size=8, n_features=16, spatial_dropout=False,
                       dropout=0.0)
    dcfg = DataConfig(n_rows=660, chunk_size=60, window=10, seed=3,
                      n_features=16)

    def run(windowed, name):
        lines = []
        tcfg = TrainConfig(batch_size=4, epochs=2, windowed_train=windowed)
        model, history = train(
            mcfg, dcfg, tcfg, checkpoint_path=str(tmp_path / f"{name}.pt"),
            norm_params_path=str(tmp_path / f"{name}.np"), log=lines.append)
        test = next(json.loads(s) for s in lines if "test_acc" in s)
        return model.state_dict(), history, test

    assert TrainConfig().windowed_train is False
    sd0, h0, t0 = run(False, "default")
    sd1, h1, t1 = run(True, "windowed")
    assert len(h0) == len(h1) == 2
    for r0, r1 in zip(h0, h1):
        assert set(r0) == set(r1)
        for k in r0:
            if k != "sec":
                assert r0[k] == r1[k], k
    assert t0 == t1
    assert sd0.keys() == sd1.keys()
    for k in sd0:
        assert torch.equal(sd0[k], sd1[k]), k


def test_train_windows_forms_chunk_batches():
    """Batches never span chunks, the last partial batch of a chunk is
    kept, targets are the last-timestep rows: exactly chunk_batches'."""
    window, batch = 10, 7
    dcfg = DataConfig(n_rows=330, chunk_size=60, window=window, seed=3,
                      n_features=12)
    market = SyntheticMarket(dcfg.n_rows, seed=dcfg.seed)
    train_set, _, _ = make_epoch_sets(market, dcfg)
    train_set = list(train_set)
    assert len(train_set) >= 2
    want = list(chunk_batches(market, train_set, dcfg, batch))
    # 41 / 60 windows per chunk: both leave a partial batch at batch 7
    assert any(x.shape[0] not in (batch,) for x, _ in want)

    model = _trainable()
    xs, ys = _record_batches(model)
    tcfg = TrainConfig(batch_size=batch, windowed_train=True)
    out = train_chunks_windowed(model, market, train_set, dcfg, tcfg)
    assert len(out) == 4 and out[3].shape == (4,)
    assert len(xs) == len(ys) == len(want)
    for x, y, (wx, wy) in zip(xs, ys, want):
        assert torch.equal(x, wx)
        assert torch.equal(y, wy.squeeze(1))


def test_train_windows_returns_per_batch_lists():
    model = _trainable()
    torch.manual_seed(0)
    table = torch.rand(30, 12)
    targets = (torch.rand(30, 4) < 0.4).float()
    accs, hams, losses, fbetas = model.train_windows(table, targets, 8, 5)
    # 23 windows in batches of 5: 5 batches, the last of 3
    assert len(accs) == len(hams) == len(losses) == len(fbetas) == 5
    assert all(isinstance(a, float) for a in accs + hams)
    assert all(f.shape == (4,) for f in fbetas)
    assert model.train_windows(table[:7], targets[:7], 8, 5) == ([], [], [],
                                                                  [])


def test_train_windows_shuffle_visits_every_window_once():
    window, n = 6, 40
    # row i holds the value i: a window is identified by its first element
    table = torch.arange(n, dtype=torch.float32)[:, None].repeat(1, 12) / n
    targets = (torch.arange(n)[:, None] % torch.tensor([2, 3, 4, 5])
               == 0).float()

    def order(seed, shuffle=True):
        model = _trainable()
        xs, ys = _record_batches(model)
        torch.manual_seed(seed)
        model.train_windows(table, targets, window, 8, shuffle=shuffle)
        starts = torch.cat([(x[:, 0, 0] * n).round().long() for x in xs])
        # the target of a window is the row of its last timestep
        assert torch.equal(torch.cat(ys), targets[starts + window - 1])
        return starts

    a = order(5)
    assert torch.equal(a.sort().values, torch.arange(n - window + 1))
    assert torch.equal(order(5), a)
    assert not torch.equal(a, order(5, shuffle=False))
    assert torch.equal(order(5, shuffle=False), torch.arange(n - window + 1))


def test_window_batch_cpu_gather():
    torch.manual_seed(1)
    table = torch.randn(11, 5)
    starts = torch.tensor([8, 0, 3, 3])
    got = window_batch(table, starts, 3)
    assert torch.equal(got, table[starts[:, None] + torch.arange(3)])
    assert got.shape == (4, 3, 5)


def test_window_batch_cpu_spatial_dropout_drops_whole_channels():
    torch.manual_seed(2)
    table = torch.rand(40, 16) + 0.5          # no zeros in the data
    starts = torch.tensor([0, 33, 7, 7, 12, 20, 1, 30])
    p, T = 0.5, 7
    got = window_batch(table, starts, T, p=p, spatial=True)
    want = table[starts[:, None] + torch.arange(T)] / (1 - p)
    dropped = (got == 0).all(dim=1)           # (B, F): zero over all of t
    kept = torch.isclose(got, want).all(dim=1)
    assert bool((dropped ^ kept).all())
    assert 0 < int(dropped.sum()) < dropped.numel()


@pytest.mark.parametrize("bad", [[-1], [0, 9], [8, 9, 0], [2 ** 40]])
def test_window_batch_cpu_rejects_out_of_range_starts(bad):
    table = torch.randn(11, 5)               # N - T = 8
    with pytest.raises(ValueError):
        window_batch(table, torch.tensor(bad), 3)
    with pytest.raises(ValueError):
        window_batch(table, torch.tensor([0]), 12)     # window > N


def test_cli_flags_set_train_config():
    args = build_parser().parse_args(
        ["--windowed-train", "--dtype", "bf16", "--batch", "64"])
    _, _, tcfg = configs_from_args(args)
    assert tcfg.windowed_train is True and tcfg.dtype == "bf16"
    assert tcfg.batch_size == 64
    _, _, tcfg = configs_from_args(build_parser().parse_args([]))
    assert tcfg.windowed_train is False and tcfg.dtype == "fp32"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--dtype", "fp16"])
