"""Fleet predict tick latency against fleet size (needs an MI355X).

Flagship serving shape: window 120, F=96, 2-layer H=128 biGRU, bf16. For
each fleet size S it times `push_rows` (one row for every symbol) +
`predict_all` on

  fleet    FleetPredictor on the route it picks itself
  streams  FleetPredictor built under FMDA_FLEET_B1=1: gru_fwd_streams
  tiled    FleetPredictor built under FMDA_FLEET_B1=0: the batch-tiled
           gru_fwd at B = S
  serial   S StreamingPredictors pushed and predicted one after the other
           (what the engine offered before the fleet path)

The contenders of one S live in one process and take turns tick by tick,
so drift of the shared host hits all of them alike. Latencies are host
wall clock around work that ends in a stream synchronise; slicing the
tick's rows out of the history is outside the timed region for all.

  python scripts/bench_fleet_predict.py --S 64              # one size
  python scripts/bench_fleet_predict.py --sweep             # all sizes

--sweep runs every S in a fresh child process under its own time limit and
stops at the first child that fails or times out. One JSON line per S.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SWEEP = [1, 8, 32, 64, 128, 129, 256]
WINDOW, F, H, L = 120, 96, 128, 2


def _pct(xs, q):
    import numpy as np
    return round(float(np.percentile(xs, q)), 4)


def measure(S, modes, ticks, warmup):
    import torch

    from fmda_amd.models import BiGRU
    from fmda_amd.runtime import FleetPredictor, StreamingPredictor

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.manual_seed(0)
    model = BiGRU(H, F, 4, n_layers=L,
                  spatial_dropout=False).to(torch.bfloat16)
    g = torch.Generator().manual_seed(1)
    x_min = torch.rand(S, F, generator=g)
    x_max = x_min + 0.5 + torch.rand(S, F, generator=g)
    n_rows = WINDOW + warmup + ticks
    hist = x_min.unsqueeze(1) + torch.rand(S, n_rows, F, generator=g) \
        * (x_max - x_min).unsqueeze(1)
    syms = [f"S{i}" for i in range(S)]
    kw = dict(device="cuda:0", dtype=torch.bfloat16, use_graph=True)

    contenders = {}
    for mode in modes:
        if mode == "serial":
            ps = [StreamingPredictor(model, x_min[i], x_max[i], WINDOW, **kw)
                  for i in range(S)]
            for k in range(WINDOW):
                for i, p in enumerate(ps):
                    p.push_row(hist[i, k])
            contenders[mode] = ps
        else:
            os.environ.pop("FMDA_FLEET_B1", None)
            if mode != "fleet":
                os.environ["FMDA_FLEET_B1"] = "0" if mode == "tiled" else "1"
            fp = FleetPredictor(model, syms, x_min, x_max, WINDOW, **kw)
            os.environ.pop("FMDA_FLEET_B1", None)
            assert fp._gpu_fast
            if mode != "fleet":
                assert fp.route == ("gru_fwd" if mode == "tiled"
                                    else "streams")
            fp.warm_start(hist[:, :WINDOW])
            contenders[mode] = fp
    torch.cuda.synchronize()

    def tick(mode, k):
        c = contenders[mode]
        rows = list(hist[:, k])
        if mode == "serial":
            # per instrument: its row, then its prediction
            t0 = time.perf_counter()
            for p, r in zip(c, rows):
                p.push_row(r)
                p.predict_window()
            return (time.perf_counter() - t0) * 1000.0, None
        rows = dict(zip(syms, rows))
        t0 = time.perf_counter()
        c.push_rows(rows)
        t1 = time.perf_counter()
        out = c.predict_all()
        t2 = time.perf_counter()
        assert len(out) == S
        return (t2 - t0) * 1000.0, (t2 - t1) * 1000.0

    lat = {m: [] for m in modes}
    pred = {m: [] for m in modes}
    for k in range(WINDOW, n_rows):
        for m in modes:
            full, p = tick(m, k)
            if k >= WINDOW + warmup:
                lat[m].append(full)
                if p is not None:
                    pred[m].append(p)
    res = {"S": S, "window": WINDOW, "F": F, "H": H, "L": L,
           "ticks": ticks, "warmup": warmup}
    for m in modes:
        res[m] = {"tick_p50_ms": _pct(lat[m], 50),
                  "tick_p99_ms": _pct(lat[m], 99)}
        if m != "serial":
            res[m]["route"] = contenders[m].route
        if pred[m]:
            res[m]["predict_p50_ms"] = _pct(pred[m], 50)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--modes", default="fleet,streams,tiled,serial")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--step-timeout", type=float, default=150.0)
    a = ap.parse_args()
    modes = [m for m in a.modes.split(",") if m]
    assert set(modes) <= {"fleet", "streams", "tiled", "serial"}, modes
    if not a.sweep:
        print(json.dumps(measure(a.S, modes, a.ticks, a.warmup)), flush=True)
        return 0
    for S in SWEEP:
        cmd = [sys.executable, os.path.abspath(__file__), "--S", str(S),
               "--modes", a.modes, "--ticks", str(a.ticks),
               "--warmup", str(a.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"S={S}: timed out after {a.step_timeout}s; stopping",
                  file=sys.stderr)
            return 124
        if rc != 0:
            print(f"S={S}: exit status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
