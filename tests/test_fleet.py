"""FleetPredictor on the CPU (the oracle path): one model, S instruments,
each with its own window and normalisation table, scored in one forward."""
import threading

import pytest
import torch

from fmda_amd.models import BiGRU
from fmda_amd.runtime import FleetPredictor, MessageBus, StreamingPredictor

SYMS = ["AAA", "BBB", "CCC"]
F = 12
W = 8
NOW = 1_000_000.0


def _tables():
    g = torch.Generator().manual_seed(3)
    x_min = torch.rand(len(SYMS), F, generator=g) * 10.0
    x_max = x_min + 0.5 + torch.rand(len(SYMS), F, generator=g) * 5.0
    return x_min, x_max


def _model(H):
    torch.manual_seed(H)
    return BiGRU(H, F, 4, n_layers=2, spatial_dropout=False, dropout=0.0)


def _fleet(model, **kw):
    x_min, x_max = _tables()
    kw.setdefault("use_graph", False)
    return FleetPredictor(model, SYMS, x_min, x_max, W, **kw)


def _rows(seed, n):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(F, generator=g) * 12.0 for _ in range(n)]


@pytest.mark.parametrize("H", [16, 128])
def test_per_symbol_equivalence_with_single_predictors(H):
    """Interleaved and partial push_rows: each symbol's result must be what
    an independent StreamingPredictor fed that symbol's stream gives.
    atol 1e-6: ATen's batch-S against batch-1 GRU differs by 6e-8 on these
    shapes (measured), so the bound is about 16x that."""
    model = _model(H)
    x_min, x_max = _tables()
    fleet = _fleet(model)
    singles = [StreamingPredictor(model, x_min[i], x_max[i], W,
                                  use_graph=False) for i in range(3)]
    streams = [_rows(10 + i, 14) for i in range(3)]
    pos = [0, 0, 0]

    def tick(which):
        rows = {}
        for i in which:
            r = streams[i][pos[i]]
            pos[i] += 1
            rows[SYMS[i]] = r
            singles[i].push_row(r.clone())
        fleet.push_rows(rows)

    # different lengths per symbol, partial ticks, one single-row form
    for which in ([0, 1, 2], [0], [1, 2], [0, 1, 2], [2], [0, 1, 2],
                  [0, 1], [0, 1, 2], [0, 1, 2], [1], [0, 1, 2], [0, 2],
                  [0, 1, 2]):
        tick(which)
    r = streams[1][pos[1]]
    fleet.push_row(SYMS[1], r)
    singles[1].push_row(r.clone())
    assert fleet.count == [p.ring.count for p in singles]
    assert min(fleet.count) >= W

    got = fleet.predict_all()
    assert list(got) == SYMS
    for i, s in enumerate(SYMS):
        want = singles[i].predict_window()
        a = torch.tensor(got[s]["probabilities"])
        b = torch.tensor(want["probabilities"])
        assert torch.allclose(a, b, atol=1e-6, rtol=0), (s, a, b)
        assert got[s]["pred_indices"] == want["pred_indices"]
        assert got[s]["pred_labels"] == want["pred_labels"]
        assert got[s]["prob_threshold"] == want["prob_threshold"]
        assert set(got[s]) == set(want)


def test_not_yet_full_symbols_are_left_out_then_appear():
    fleet = _fleet(_model(16))
    rows = _rows(1, W)
    for r in rows[:-1]:
        fleet.push_rows({s: r for s in SYMS})
    assert fleet.predict_all() == {}
    fleet.push_rows({"AAA": rows[-1], "CCC": rows[-1]})
    assert list(fleet.predict_all()) == ["AAA", "CCC"]
    assert fleet.window_full() == {"AAA": True, "BBB": False, "CCC": True}
    fleet.push_row("BBB", rows[-1])
    assert list(fleet.predict_all()) == SYMS


def test_unknown_symbol_raises_and_changes_nothing():
    fleet = _fleet(_model(16))
    before = fleet.rings.clone()
    with pytest.raises(KeyError):
        fleet.push_rows({"AAA": torch.zeros(F), "ZZZ": torch.zeros(F)})
    with pytest.raises(KeyError):
        fleet.push_row("ZZZ", torch.zeros(F))
    assert fleet.count == [0, 0, 0]
    assert torch.equal(fleet.rings, before)


def test_broadcast_table_and_degenerate_range_clamp():
    x_min = torch.zeros(F)
    x_max = torch.ones(F)
    x_max[3] = 0.0                       # MIN == MAX column
    fleet = FleetPredictor(_model(16), SYMS, x_min, x_max, W,
                           use_graph=False)
    assert fleet.x_rng.shape == (3, F)
    assert float(fleet.x_rng[:, 3].max()) == pytest.approx(1e-6)
    fleet.warm_start(torch.zeros(3, W, F))
    probs = fleet.predict_all()["BBB"]["probabilities"]
    assert all(p == p for p in probs)    # no NaN from the 0/0 column


def test_warm_start_equals_row_by_row_pushes():
    model = _model(16)
    a, b = _fleet(model), _fleet(model)
    g = torch.Generator().manual_seed(5)
    hist = torch.rand(3, W + 3, F, generator=g) * 12.0
    a.warm_start(hist)
    for k in range(hist.shape[1]):
        for i, s in enumerate(SYMS):
            b.push_row(s, hist[i, k])
    assert torch.equal(a.rings, b.rings)
    assert a.count == b.count == [W + 3] * 3
    pa, pb = a.predict_all(), b.predict_all()
    assert pa == pb and list(pa) == SYMS
    with pytest.raises(ValueError):
        a.warm_start(torch.zeros(2, 4, F))


def _full_fleet(**kw):
    bus = MessageBus()
    fleet = _fleet(_model(16), bus=bus, **kw)
    for k, r in enumerate(_rows(2, W)):
        fleet.push_rows({s: r + i for i, s in enumerate(SYMS)}, ts=NOW + k)
    return fleet, bus


def test_handle_timestamp_stale_publishes_nothing():
    fleet, bus = _full_fleet(stale_after=240.0)
    assert fleet.handle_timestamp({"Timestamp": NOW - 1000}, now=NOW) is None
    assert bus.topic("prediction").end_offset() == 0
    assert fleet.n_stale == 1 and fleet.n_predictions == 0


def test_handle_timestamp_publishes_symbol_and_timestamp():
    fleet, bus = _full_fleet()
    ts = NOW + W - 1                      # every symbol's row has landed
    out = fleet.handle_timestamp({"Timestamp": ts}, now=ts)
    assert list(out) == SYMS and fleet.n_retries == 0
    topic = bus.topic("prediction")
    assert topic.end_offset() == 3
    msgs = [topic.read(k, timeout=0) for k in range(3)]
    assert [m["symbol"] for m in msgs] == SYMS
    for m in msgs:
        assert m["timestamp"] == ts
        assert m["probabilities"] == out[m["symbol"]]["probabilities"]
        assert len(m["probabilities"]) == 4


def test_lagging_symbol_dropped_after_one_retry_others_publish():
    fleet, bus = _full_fleet(settle_delay=0.0)
    ts = NOW + 100
    row = _rows(9, 1)[0]
    fleet.push_rows({"AAA": row, "CCC": row}, ts=ts)    # BBB lags
    out = fleet.handle_timestamp({"Timestamp": ts}, now=ts)
    assert list(out) == ["AAA", "CCC"]
    assert fleet.n_retries == 1
    assert fleet.n_dropped_missing == {"AAA": 0, "BBB": 1, "CCC": 0}
    assert bus.topic("prediction").end_offset() == 2
    res = fleet.score_timestamp({"Timestamp": ts}, now=ts)
    assert res["dropped"] == ["BBB"] and not res["stale"]
    assert fleet.n_dropped_missing["BBB"] == 2 and fleet.n_retries == 2


def test_push_during_settle_sleep_satisfies_the_retry(monkeypatch):
    """The settle sleep is outside the lock: a push_rows that lands while
    handle_timestamp waits must be seen by the retry. The sleep is replaced
    by a hook that does the push from another thread and joins it, so the
    test neither waits nor depends on timing; a sleep under the lock would
    deadlock the join (bounded by its timeout) and fail the asserts."""
    import fmda_amd.runtime.fleet as fleet_mod

    fleet, bus = _full_fleet(settle_delay=0.25)
    ts = NOW + 100
    row = _rows(9, 1)[0]
    fleet.push_rows({"AAA": row, "CCC": row}, ts=ts)    # BBB lags
    slept = []

    def fake_sleep(dt):
        slept.append(dt)
        t = threading.Thread(
            target=lambda: fleet.push_row("BBB", row, ts=ts))
        t.start()
        t.join(timeout=5)
        assert not t.is_alive(), "push_rows blocked during the settle sleep"

    monkeypatch.setattr(fleet_mod.time, "sleep", fake_sleep)
    out = fleet.handle_timestamp({"Timestamp": ts}, now=ts)
    assert slept == [0.25]                 # one retry, one sleep
    assert list(out) == SYMS
    assert fleet.n_retries == 1
    assert fleet.n_dropped_missing == {s: 0 for s in SYMS}
    assert bus.topic("prediction").end_offset() == 3


def test_run_consumes_the_timestamp_topic():
    fleet, bus = _full_fleet(stale_after=1e12)
    bus.publish("predict_timestamp", {"Timestamp": NOW + W - 1})
    bus.publish("predict_timestamp", {"Timestamp": NOW + W - 1})
    assert fleet.run(timeout=0) == 2
    assert bus.topic("prediction").end_offset() == 6
    assert fleet.run(timeout=0) == 0


def test_cuda_only_paths_are_not_taken_on_cpu():
    fleet = _fleet(_model(128))
    assert not fleet._gpu_fast and fleet.route == "model"


# ---------------- serving surface ----------------

def _client(**kw):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from fmda_amd.serve import create_fleet_app
    kw.setdefault("stale_after", 1e12)
    fleet = _fleet(_model(16), **kw)
    return TestClient(create_fleet_app(fleet)), fleet


def test_serve_round_trip():
    client, fleet = _client()
    r = client.get("/healthz").json()
    assert r["symbols"] == SYMS and r["window"] == W
    assert r["device"] == "cpu"
    assert r["window_full"] == {s: False for s in SYMS}

    r = client.post("/timestamp", json={"Timestamp": NOW}).json()
    assert r["ok"] is False and r["not_full"] == SYMS

    rows = _rows(4, W)
    for k, row in enumerate(rows):
        body = {"rows": {s: (row + i).tolist() for i, s in enumerate(SYMS)},
                "ts": NOW + k}
        r = client.post("/ingest", json=body)
        assert r.status_code == 200 and r.json()["ok"]
    assert r.json()["window_full"] == {s: True for s in SYMS}
    assert client.get("/healthz").json()["window_full"]["BBB"] is True

    ts = NOW + W - 1
    r = client.post("/timestamp", json={"Timestamp": ts}).json()
    assert r["ok"] and sorted(r["predictions"]) == SYMS
    assert r["predictions"]["BBB"]["symbol"] == "BBB"
    assert r["predictions"]["BBB"]["timestamp"] == ts

    allp = client.get("/prediction/latest").json()["predictions"]
    assert sorted(allp) == SYMS
    one = client.get("/prediction/latest", params={"symbol": "CCC"}).json()
    assert one["prediction"]["probabilities"] == \
        r["predictions"]["CCC"]["probabilities"]
    # the app serves what the predictor computes
    assert fleet.predict_all()["CCC"]["probabilities"] == \
        one["prediction"]["probabilities"]

    assert client.get("/prediction/latest",
                      params={"symbol": "ZZZ"}).status_code == 404
    assert client.post("/ingest",
                       json={"rows": {"ZZZ": [0.0] * F}}).status_code == 404


def test_serve_metrics_have_both_drop_counters():
    pytest.importorskip("prometheus_client")
    client, fleet = _client(stale_after=240.0)
    rows = _rows(4, W)
    for k, row in enumerate(rows):
        client.post("/ingest", json={"rows": {s: row.tolist() for s in SYMS},
                                     "ts": NOW + k})
    # a stale message (wall clock is far past NOW) ...
    assert client.post("/timestamp",
                       json={"Timestamp": NOW}).json()["reason"] == "stale"
    # ... and a tick for which only AAA's row landed
    import time
    ts = time.time()
    client.post("/ingest", json={"rows": {"AAA": rows[0].tolist()},
                                 "ts": ts})
    r = client.post("/timestamp", json={"Timestamp": ts}).json()
    assert sorted(r["predictions"]) == ["AAA"]
    assert r["dropped"] == ["BBB", "CCC"]
    text = client.get("/metrics").text
    assert "fmda_fleet_stale_dropped_total 1.0" in text
    assert "fmda_fleet_settle_dropped_total 2.0" in text
    assert 'fmda_fleet_rows_ingested_total{symbol="AAA"} %.1f' % (W + 1) \
        in text
    assert 'fmda_fleet_rows_ingested_total{symbol="BBB"} %.1f' % W in text
    assert 'fmda_fleet_predictions_total{symbol="AAA"} 1.0' in text
    assert 'fmda_fleet_predictions_total{symbol="BBB"}' not in text


def test_concurrent_ingest_and_timestamp():
    """Handlers run on a threadpool: hammer push_rows and handle_timestamp
    concurrently; the lock must keep counts and results consistent."""
    fleet = _fleet(_model(16), stale_after=1e12)
    errs = []

    def ingest(k):
        try:
            for i in range(50):
                fleet.push_rows({s: torch.rand(F) for s in SYMS[k:]},
                                ts=NOW + i)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    def predict():
        try:
            for _ in range(50):
                out = fleet.handle_timestamp({"Timestamp": NOW}, now=NOW)
                for v in out.values():
                    assert len(v["probabilities"]) == 4
        except Exception as e:  # pragma: no cover
            errs.append(e)

    threads = [threading.Thread(target=ingest, args=(k,)) for k in range(2)]
    threads += [threading.Thread(target=predict) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not errs
    assert fleet.count == [50, 100, 100]
    assert list(fleet.predict_all()) == SYMS
