"""Fleet serving demo: one model scores several instruments per tick.

A synthetic market per symbol (one seed each, so price levels and ranges
differ), a per-symbol min/max table, `warm_start` from each symbol's
history, then a few live ticks through the message bus: every tick pushes
one new row per symbol and one `predict_timestamp` message scores the
whole fleet.

  python examples/fleet_demo.py                    # CPU oracle path
  python examples/fleet_demo.py --device cuda      # one captured graph
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from fmda_amd.data import SyntheticMarket  # noqa: E402
from fmda_amd.models import BiGRU  # noqa: E402
from fmda_amd.runtime import FleetPredictor, MessageBus  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--symbols", type=int, default=4)
    ap.add_argument("--window", type=int, default=30)
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=128)
    a = ap.parse_args()

    syms = [f"SYM{i}" for i in range(a.symbols)]
    n = a.window + a.ticks
    tables = torch.stack([SyntheticMarket(n_rows=n + 60, seed=100 + i).X[-n:]
                          * (1.0 + i) for i in range(a.symbols)])  # (S, n, F)
    x_min = tables.amin(dim=1)
    x_max = tables.amax(dim=1)

    cuda = a.device.startswith("cuda")
    device = "cuda:0" if a.device == "cuda" else a.device
    dtype = torch.bfloat16 if cuda else torch.float32
    torch.manual_seed(0)
    model = BiGRU(a.hidden, tables.shape[2], 4, n_layers=2,
                  spatial_dropout=False).to(dtype)
    bus = MessageBus()
    fleet = FleetPredictor(model, syms, x_min, x_max, a.window, bus=bus,
                           stale_after=1e12, device=device, dtype=dtype)
    fleet.warm_start(tables[:, :a.window])
    print(f"fleet of {len(syms)} on {device}: route={fleet.route}, "
          f"window_full={all(fleet.window_full().values())}")

    for k in range(a.ticks):
        ts = 1_000_000.0 + 300.0 * k
        fleet.push_rows({s: tables[i, a.window + k]
                         for i, s in enumerate(syms)}, ts=ts)
        bus.publish("predict_timestamp", {"Timestamp": ts})
    fleet.run(timeout=0)

    topic = bus.topic("prediction")
    n_pred = topic.end_offset()
    for k in range(n_pred - len(syms), n_pred):
        m = topic.read(k, timeout=0)
        probs = ", ".join(f"{p:.3f}" for p in m["probabilities"])
        print(f"  {m['symbol']} @ {m['timestamp']:.0f}: [{probs}] "
              f"{m['pred_labels']}")
    print(f"{n_pred} predictions published in {fleet.n_predictions} "
          "fleet ticks")
    assert n_pred == a.ticks * len(syms)


if __name__ == "__main__":
    main()
