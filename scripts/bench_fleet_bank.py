"""Banked fleet tick latency against fleet size S and bank size M (needs an
MI355X).

Flagship serving shape: window 120, F=96, 2-layer H=128 biGRU, bf16. For
each (S, M) it times `push_rows` (one row for every symbol) + `predict_all`
on

  bank   BankedFleetPredictor, M models, symbol i on slot i % M
  fleet  FleetPredictor with ONE model at the same S, on the route it picks
         itself (what the banked tick costs over the single-model tick)
  loop   M FleetPredictors, one per model, each with the symbols of its
         slot, pushed and predicted one after the other (what serving M
         models costs without the bank)

The contenders of one (S, M) live in one process and take turns tick by
tick, so drift of the shared host hits all of them alike. Latencies are
host wall clock around work that ends in a stream synchronise; slicing the
tick's rows out of the history is outside the timed region for all.

  python scripts/bench_fleet_bank.py --S 64 --M 8          # one point
  python scripts/bench_fleet_bank.py --sweep               # all points

--sweep runs every point in a fresh child process under its own time limit
and stops at the first child that fails or times out. One JSON line per
point. M = 1 and M = S are in the sweep at every S.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SWEEP_S = [8, 64]
WINDOW, F, H, L = 120, 96, 128, 2


def sweep_points():
    return [(S, M) for S in SWEEP_S for M in sorted({1, 8, S})]


def _pct(xs, q):
    import numpy as np
    return round(float(np.percentile(xs, q)), 4)


def measure(S, M, modes, ticks, warmup):
    import torch

    from fmda_amd.models import BiGRU
    from fmda_amd.runtime import BankedFleetPredictor, FleetPredictor

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    assert 1 <= M <= S
    models = []
    for k in range(M):
        torch.manual_seed(k)
        models.append(BiGRU(H, F, 4, n_layers=L,
                            spatial_dropout=False).to(torch.bfloat16))
    g = torch.Generator().manual_seed(1)
    x_min = torch.rand(S, F, generator=g)
    x_max = x_min + 0.5 + torch.rand(S, F, generator=g)
    n_rows = WINDOW + warmup + ticks
    hist = x_min.unsqueeze(1) + torch.rand(S, n_rows, F, generator=g) \
        * (x_max - x_min).unsqueeze(1)
    syms = [f"S{i}" for i in range(S)]
    slots = [i % M for i in range(S)]
    kw = dict(device="cuda:0", dtype=torch.bfloat16, use_graph=True)

    contenders = {}
    for mode in modes:
        if mode == "bank":
            p = BankedFleetPredictor(models, syms, slots, x_min, x_max,
                                     WINDOW, **kw)
            assert p.route == "streams_bank"
            p.warm_start(hist[:, :WINDOW])
            contenders[mode] = p
        elif mode == "fleet":
            p = FleetPredictor(models[0], syms, x_min, x_max, WINDOW, **kw)
            assert p._gpu_fast
            p.warm_start(hist[:, :WINDOW])
            contenders[mode] = p
        else:
            groups = []
            for m in range(M):
                rows = [i for i in range(S) if slots[i] == m]
                p = FleetPredictor(models[m], [syms[i] for i in rows],
                                   x_min[rows], x_max[rows], WINDOW, **kw)
                p.warm_start(hist[rows, :WINDOW])
                groups.append((rows, p))
            contenders[mode] = groups
    torch.cuda.synchronize()

    def tick(mode, k):
        c = contenders[mode]
        rows = list(hist[:, k])
        if mode == "loop":
            per = [({syms[i]: rows[i] for i in idx}, p) for idx, p in c]
            n = 0
            t0 = time.perf_counter()
            for r, p in per:
                p.push_rows(r)
                n += len(p.predict_all())
            dt = (time.perf_counter() - t0) * 1000.0
            assert n == S
            return dt, None
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
    res = {"S": S, "M": M, "window": WINDOW, "F": F, "H": H, "L": L,
           "ticks": ticks, "warmup": warmup}
    for m in modes:
        res[m] = {"tick_p50_ms": _pct(lat[m], 50),
                  "tick_p99_ms": _pct(lat[m], 99)}
        if m != "loop":
            res[m]["route"] = contenders[m].route
        if pred[m]:
            res[m]["predict_p50_ms"] = _pct(pred[m], 50)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--M", type=int, default=8)
    ap.add_argument("--modes", default="bank,fleet,loop")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--step-timeout", type=float, default=150.0)
    a = ap.parse_args()
    modes = [m for m in a.modes.split(",") if m]
    assert set(modes) <= {"bank", "fleet", "loop"}, modes
    if not a.sweep:
        print(json.dumps(measure(a.S, a.M, modes, a.ticks, a.warmup)),
              flush=True)
        return 0
    for S, M in sweep_points():
        cmd = [sys.executable, os.path.abspath(__file__), "--S", str(S),
               "--M", str(M), "--modes", a.modes, "--ticks", str(a.ticks),
               "--warmup", str(a.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"S={S} M={M}: timed out after {a.step_timeout}s; "
                  "stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"S={S} M={M}: exit status {rc}; stopping",
                  file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
