"""Time the fused window gather + dropout and the windowed training epoch.

Part 1, one training batch (B windows of T x F, bf16, dropout p), one build,
one process:
  (a) window_batch   the kernel: dropped batch written straight from the table
  (b) unfold         table.unfold + .contiguous() + dropout_fused, all on the
                     device (a gather pass, then a read-and-write pass)
  (c) loader         BatchLoader -> DataLoader -> host-to-device copy, what
                     the default training driver does per batch (sequences/s)

Part 2, the training part of one train.py-style epoch over the same chunks:
  default    model.train_model(chunk_batches(...)): DataLoader, fp32 input,
             eager loss, clip_grad_norm_ + torch.optim.Adam
  windowed   train_chunks_windowed(...): tables on the device in bf16,
             window_batch, fused_head_loss, FusedClipAdam

Every path is warmed up, a repeat ends in a device synchronise, the paths
alternate inside every repeat, and median / min / max are reported. Prints
one JSON line; profiles/windowed_train.md holds the prediction and a run.

Run on a GPU: python scripts/bench_window_batch.py
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from fmda_amd.config import DataConfig, TrainConfig  # noqa: E402
from fmda_amd.data import BatchLoader, SyntheticMarket  # noqa: E402
from fmda_amd.models import BiGRU  # noqa: E402
from fmda_amd.ops import load_extension  # noqa: E402
from fmda_amd.optim import FusedClipAdam  # noqa: E402
from fmda_amd.train import (chunk_batches, class_weights,  # noqa: E402
                            make_epoch_sets, train_chunks_windowed)


def timed(fn, inner=1):
    """Seconds per call of `inner` back-to-back calls ending in one device
    synchronise."""
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def spread(xs, scale=1.0):
    return {"median": statistics.median(xs) * scale, "min": min(xs) * scale,
            "max": max(xs) * scale, "n": len(xs)}


def bench_batch(args):
    ext = load_extension()
    B, T, F, p = args.batch, args.seq_len, args.features, args.p
    n_rows = B + T - 1
    torch.manual_seed(0)
    raw = torch.rand(n_rows, F)
    table = raw.cuda().bfloat16()
    starts = torch.arange(B, device="cuda")
    perm = torch.randperm(B).cuda()

    def fused():
        return ext.window_batch(table, starts, T, p, 1, False)

    def fused_shuffled():
        return ext.window_batch(table, perm, T, p, 1, False)

    def unfold():
        x = table.unfold(0, T, 1).permute(0, 2, 1).contiguous()
        return ext.dropout_fused(x, p, 1)

    assert torch.equal(fused(), unfold())
    for fn in (fused, fused_shuffled, unfold):
        timed(fn, args.warmup)
    t = {"window_batch": [], "window_batch_shuffled": [], "unfold": []}
    for _ in range(args.repeats):
        t["window_batch"].append(timed(fused, args.inner))
        t["window_batch_shuffled"].append(timed(fused_shuffled, args.inner))
        t["unfold"].append(timed(unfold, args.inner))

    # (c) the default driver's per-batch input path
    Y = torch.zeros(n_rows, 4)
    norms = (raw.min(dim=0).values[None], raw.max(dim=0).values[None])
    bl = BatchLoader(range(1, n_rows + 1), norms, raw, Y, T)
    assert len(bl) == B

    def loader():
        for x, y in DataLoader(bl, batch_size=B, shuffle=False):
            x.cuda(), y.cuda()

    timed(loader)
    t["loader"] = [timed(loader) for _ in range(args.loader_repeats)]
    out = {k + "_ms": spread(v, 1e3) for k, v in t.items()}
    out_bytes = B * T * F * 2
    for k, v in t.items():
        out[k + "_seq_per_s"] = B / statistics.median(v)
    out["window_batch_write_GBps"] = \
        out_bytes / statistics.median(t["window_batch"]) / 1e9
    out["batch_bytes"] = out_bytes
    return out


def bench_epoch(args):
    dcfg = DataConfig(n_rows=args.rows, chunk_size=args.chunk_size,
                      window=args.seq_len, seed=3, n_features=args.features)
    market = SyntheticMarket(dcfg.n_rows, seed=dcfg.seed)
    weight, pos_weight = class_weights(market.Y)
    dev = torch.device("cuda")

    def make(windowed):
        torch.manual_seed(0)
        model = BiGRU(args.hidden, args.features, 4, n_layers=args.layers,
                      spatial_dropout=False, dropout=args.p).to(dev)
        model.add_loss_fn(nn.BCEWithLogitsLoss(
            weight=weight.to(dev), pos_weight=pos_weight.to(dev)))
        model.add_optimizer(
            FusedClipAdam(model.parameters(), lr=1e-3, clip=model.clip)
            if windowed else torch.optim.Adam(model.parameters(), lr=1e-3))
        model.add_device(dev)
        return model

    m_def, m_win = make(False), make(True)
    tcfg = TrainConfig(batch_size=args.epoch_batch, device="cuda",
                       dtype="bf16", windowed_train=True)
    train_set = list(make_epoch_sets(market, dcfg)[0])
    n_windows = sum(len(ind) - dcfg.window + 1 for ind, _ in train_set)

    def default():
        m_def.train_model(chunk_batches(market, train_set, dcfg,
                                        tcfg.batch_size))

    def windowed():
        train_chunks_windowed(m_win, market, train_set, dcfg, tcfg)

    timed(default), timed(windowed)
    t_def, t_win = [], []
    for _ in range(args.epoch_repeats):
        t_def.append(timed(default))
        t_win.append(timed(windowed))
    return {"epoch_windows": n_windows, "epoch_chunks": len(train_set),
            "epoch_batch": tcfg.batch_size,
            "default_epoch_s": spread(t_def), "windowed_epoch_s": spread(t_win),
            "default_seq_per_s": n_windows / statistics.median(t_def),
            "windowed_seq_per_s": n_windows / statistics.median(t_win),
            "epoch_speedup": statistics.median(t_def)
            / statistics.median(t_win)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--seq-len", type=int, default=120)
    ap.add_argument("--features", type=int, default=108)
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10,
                    help="calls per timed repeat (one synchronise each)")
    ap.add_argument("--loader-repeats", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--chunk-size", type=int, default=5000)
    ap.add_argument("--epoch-batch", type=int, default=4096)
    ap.add_argument("--epoch-repeats", type=int, default=3)
    ap.add_argument("--skip-epoch", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"

    rec = {"batch": args.batch, "seq_len": args.seq_len,
           "features": args.features, "p": args.p, "dtype": "bf16",
           "hidden": args.hidden, "layers": args.layers,
           "repeats": args.repeats, "warmup": args.warmup,
           "inner": args.inner,
           "device": f"{torch.cuda.get_device_name(0)} "
                     f"({torch.cuda.get_device_properties(0).gcnArchName})"}
    rec.update(bench_batch(args))
    if not args.skip_epoch:
        rec.update(bench_epoch(args))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
