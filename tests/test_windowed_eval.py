"""Windowed table inference on CPU: BiGRU.forward_windows /
evaluate_windows and the train driver's windowed_eval switch against the
materialised-window path (BatchLoader -> DataLoader -> evaluate_model)."""
import json

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from fmda_amd.config import DataConfig, ModelConfig, TrainConfig
from fmda_amd.data import BatchLoader, ChunkLoader, SyntheticMarket
from fmda_amd.models import BiGRU
from fmda_amd.train import train


def _model(hidden=8, n_features=12, layers=2):
    torch.manual_seed(11)
    return BiGRU(hidden, n_features, 4, n_layers=layers,
                 spatial_dropout=False, dropout=0.0).eval()


@pytest.mark.parametrize("stride,batch_windows", [(1, 4), (2, 4), (1, 64)])
def test_forward_windows_cpu_equals_forward_on_unfolded(stride, batch_windows):
    """Same batches through the same CPU kernels: bitwise equal. 14 (stride
    1) / 7 (stride 2) windows in chunks of 4 leave a ragged last chunk."""
    model = _model()
    torch.manual_seed(5)
    table = torch.randn(23, 12)
    window = 10
    got = model.forward_windows(table, window, stride=stride,
                                batch_windows=batch_windows)
    wins = table.unfold(0, window, stride).permute(0, 2, 1).contiguous()
    assert got.shape == (wins.shape[0], 4)
    assert wins.shape[0] % batch_windows != 0
    with torch.no_grad():
        want = torch.cat([model(wins[i:i + batch_windows])
                          for i in range(0, wins.shape[0], batch_windows)])
    assert torch.equal(got, want)
    # row i is the single-window forward of window i (different batching:
    # close, not necessarily bitwise)
    with torch.no_grad():
        one = model(table[3 * stride:3 * stride + window][None])
    assert torch.allclose(got[3], one[0], atol=1e-6)


def test_forward_windows_rejects_bad_calls():
    model = _model()
    table = torch.randn(23, 12)
    with pytest.raises(AssertionError):
        model.train().forward_windows(table, 10)
    model.eval()
    with pytest.raises(AssertionError):
        model.forward_windows(table[:5], 10)      # shorter than a window
    with pytest.raises(AssertionError):
        model.forward_windows(table, 10, stride=0)
    with pytest.raises(AssertionError):
        model.forward_windows(table[:, :7], 10)   # wrong feature count


@pytest.mark.parametrize("batch_size", [4, 7])
def test_evaluate_windows_matches_evaluate_model(batch_size):
    window = 10
    market = SyntheticMarket(260, seed=2)
    X = market.X[:, :16]
    chunks = ChunkLoader(X, 60, window)
    indices, norms = chunks[1]
    bl = BatchLoader(indices, norms, X, market.Y, window)
    model = _model(hidden=8, n_features=16, layers=1)
    model.add_device(torch.device("cpu"))
    # bias the head so that predictions are not all-negative
    with torch.no_grad():
        model.linear.bias.add_(0.05)

    want = model.evaluate_model(
        DataLoader(bl, batch_size=batch_size, shuffle=False))
    got = model.evaluate_windows(bl.x, bl.y, window, batch_size)

    # 60 windows: full batches of 4, a ragged last batch of 7
    assert got[3].shape == (len(bl), 4) == (60, 4)
    assert 0 < int(got[3].sum()) < got[3].numel()   # not a trivial case
    assert torch.equal(got[3], want[3])
    assert torch.equal(got[4], want[4])
    for g, w in zip(got[:3], want[:3]):
        assert np.allclose(g, w, rtol=1e-12, atol=1e-15)


def test_train_windowed_eval_logs_same_metrics(tmp_path):
    # 12 chunks of 60 rows: 9 train, 2 validation, 1 test
    mcfg = ModelConfig(hidden_size=8, n_features=16, spatial_dropout=False,
                       dropout=0.2)
    dcfg = DataConfig(n_rows=660, chunk_size=60, window=10, seed=3,
                      n_features=16)

    def run(windowed, name):
        lines = []
        tcfg = TrainConfig(batch_size=4, epochs=1, windowed_eval=windowed)
        train(mcfg, dcfg, tcfg, checkpoint_path=str(tmp_path / f"{name}.pt"),
              norm_params_path=str(tmp_path / f"{name}.np"),
              log=lines.append)
        recs = [json.loads(s) for s in lines]
        epoch = next(r for r in recs if "val_acc" in r)
        test = next(r for r in recs if "test_acc" in r)
        return epoch, test

    assert TrainConfig().windowed_eval is False
    e0, t0 = run(False, "default")
    e1, t1 = run(True, "windowed")
    for k in ("train_loss", "val_acc", "val_hamming", "val_acc3"):
        assert e0[k] == e1[k], k
    assert t0 == t1
    assert t0["test_acc"] is not None
