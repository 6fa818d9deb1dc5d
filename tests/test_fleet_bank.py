"""BankedFleetPredictor on the CPU (the oracle path): a bank of models, one
slot per symbol, `assign` and `swap_model` between ticks."""
import pytest
import torch

from fmda_amd.models import BiGRU
from fmda_amd.runtime import BankedFleetPredictor, FleetPredictor, MessageBus

SYMS = [f"S{i}" for i in range(6)]
SLOTS = [0, 1, 2, 0, 2, 1]
F = 12
W = 8
H = 16
NOW = 1_000_000.0


def _tables(S=len(SYMS)):
    g = torch.Generator().manual_seed(3)
    x_min = torch.rand(S, F, generator=g) * 10.0
    x_max = x_min + 0.5 + torch.rand(S, F, generator=g) * 5.0
    return x_min, x_max


def _model(seed, hidden=H, **kw):
    torch.manual_seed(seed)
    return BiGRU(hidden, F, 4, n_layers=2, spatial_dropout=False,
                 dropout=0.0, **kw)


def _history(n=W + 2, S=len(SYMS)):
    g = torch.Generator().manual_seed(5)
    return torch.rand(S, n, F, generator=g) * 12.0


def _bank(models, slots=SLOTS, syms=SYMS, **kw):
    x_min, x_max = _tables(len(syms))
    kw.setdefault("use_graph", False)
    return BankedFleetPredictor(models, syms, slots, x_min, x_max, W, **kw)


def _probs(res, syms=SYMS):
    return torch.tensor([res[s]["probabilities"] for s in syms])


def _alone(model, hist, i):
    """sigmoid(model(window)) of symbol i, computed on its own."""
    x_min, x_max = _tables(hist.shape[0])
    win = hist[i, -W:]
    x = (win - x_min[i]) / (x_max[i] - x_min[i]).clamp(min=1e-6)
    with torch.no_grad():
        return torch.sigmoid(model.eval()(x.unsqueeze(0)))[0]


def test_one_model_bank_is_the_fleet_predictor():
    model = _model(0)
    x_min, x_max = _tables()
    fleet = FleetPredictor(model, SYMS, x_min, x_max, W, use_graph=False)
    bank = _bank([model], [0] * 6)
    assert bank.route == "grouped" and not bank._gpu_fast
    hist = _history()
    for k in range(hist.shape[1]):           # the same pushes, partial ticks
        for p in (fleet, bank):
            p.push_rows({s: hist[i, k] for i, s in enumerate(SYMS[:4])})
            p.push_rows({s: hist[i + 4, k] for i, s in enumerate(SYMS[4:])})
    a, b = fleet.predict_all(), bank.predict_all()
    assert list(a) == list(b) == SYMS
    assert torch.equal(_probs(a), _probs(b))
    for s in SYMS:
        assert b[s]["model"] == 0
        assert {k: v for k, v in b[s].items() if k != "model"} == a[s]


def test_each_symbol_matches_its_own_model_alone():
    models = [_model(k) for k in range(3)]
    bank = _bank(models, dict(zip(SYMS, SLOTS)))      # the mapping form
    hist = _history()
    bank.warm_start(hist)
    res = bank.predict_all()
    got = _probs(res)
    for i, s in enumerate(SYMS):
        want = _alone(models[SLOTS[i]], hist, i)
        assert torch.allclose(got[i], want, atol=1e-5, rtol=0), (s, got[i],
                                                                 want)
        assert res[s]["model"] == SLOTS[i]
    # the models differ, so the slot matters
    assert not torch.allclose(got[0], _alone(models[1], hist, 0), atol=1e-5)


def test_assign_moves_exactly_one_symbol():
    models = [_model(k) for k in range(3)]
    bank = _bank(models)
    hist = _history()
    bank.warm_start(hist)
    before = _probs(bank.predict_all())
    bank.assign("S0", 2)
    assert bank.model_of()["S0"] == 2
    res = bank.predict_all()
    after = _probs(res)
    assert res["S0"]["model"] == 2
    assert torch.allclose(after[0], _alone(models[2], hist, 0), atol=1e-5,
                          rtol=0)
    assert not torch.equal(after[0], before[0])
    # the groups of slots 0 and 2 changed size: same model, same windows,
    # and ATen's GRU at another batch size differs in the last bits (6e-8,
    # see test_fleet.py); slot 1's group runs exactly as before
    for i in (2, 3, 4):
        assert torch.allclose(after[i], before[i], atol=1e-6, rtol=0), i
    for i in (1, 5):
        assert torch.equal(after[i], before[i]), i
    # equal to a predictor constructed with that mapping
    fresh = _bank(models, [2, 1, 2, 0, 2, 1])
    fresh.warm_start(hist)
    assert torch.equal(_probs(fresh.predict_all()), after)


def test_swap_model_moves_exactly_the_slots_symbols():
    models = [_model(k) for k in range(3)]
    bank = _bank(models)
    hist = _history()
    bank.warm_start(hist)
    before = _probs(bank.predict_all())
    new = _model(7)
    bank.swap_model(1, new)
    after = _probs(bank.predict_all())
    for i, k in enumerate(SLOTS):
        if k == 1:
            assert not torch.equal(after[i], before[i]), i
            assert torch.allclose(after[i], _alone(new, hist, i), atol=1e-5,
                                  rtol=0)
        else:
            assert torch.equal(after[i], before[i]), i
    fresh = _bank([models[0], new, models[2]])
    fresh.warm_start(hist)
    assert torch.equal(_probs(fresh.predict_all()), after)
    assert bank.n_captures == 0


def test_validation_errors_leave_state_untouched():
    models = [_model(k) for k in range(3)]
    x_min, x_max = _tables()
    with pytest.raises(ValueError, match="hidden_size"):
        _bank(models[:2] + [_model(2, hidden=32)])
    with pytest.raises(ValueError, match="n_directions"):
        _bank(models[:2] + [_model(2, bidirectional=False)])
    with pytest.raises(ValueError):
        _bank([])
    with pytest.raises(ValueError):
        _bank(models, [0, 1, 3, 0, 2, 1])             # slot out of range
    with pytest.raises(ValueError):
        _bank(models, [0, 1, 2])                      # one slot per symbol
    with pytest.raises(ValueError):
        _bank(models, {s: 0 for s in SYMS[:5]})       # S5 has no slot

    bank = _bank(models)
    hist = _history()
    bank.warm_start(hist)
    before = _probs(bank.predict_all())
    for bad in (3, -1, 1.0, True, None):
        with pytest.raises(ValueError):
            bank.assign("S0", bad)
        with pytest.raises(ValueError):
            bank.swap_model(bad, _model(9))
    with pytest.raises(KeyError):
        bank.assign("ZZZ", 0)
    with pytest.raises(ValueError, match="hidden_size"):
        bank.swap_model(1, _model(9, hidden=32))
    assert bank.model_of() == dict(zip(SYMS, SLOTS))
    assert all(a is b for a, b in zip(bank.models, models))
    assert torch.equal(_probs(bank.predict_all()), before)


def test_score_timestamp_publishes_the_model_slot():
    bus = MessageBus()
    bank = _bank([_model(k) for k in range(3)], bus=bus)
    hist = _history(W)
    for k in range(W):
        bank.push_rows({s: hist[i, k] for i, s in enumerate(SYMS)},
                       ts=NOW + k)
    ts = NOW + W - 1
    res = bank.score_timestamp({"Timestamp": ts}, now=ts)
    assert not res["stale"] and list(res["predictions"]) == SYMS
    topic = bus.topic("prediction")
    assert topic.end_offset() == 6
    msgs = [topic.read(k, timeout=0) for k in range(6)]
    assert [m["symbol"] for m in msgs] == SYMS
    assert [m["model"] for m in msgs] == SLOTS
    assert all(m["timestamp"] == ts for m in msgs)


def test_assign_through_the_app():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from fmda_amd.serve import create_fleet_app
    models = [_model(k) for k in range(3)]
    bank = _bank(models, stale_after=1e12)
    client = TestClient(create_fleet_app(bank))
    r = client.get("/healthz").json()
    assert r["symbols"] == SYMS and r["route"] == "grouped"
    assert r["model_of"] == dict(zip(SYMS, SLOTS))

    hist = _history(W)
    for k in range(W):
        body = {"rows": {s: hist[i, k].tolist() for i, s in enumerate(SYMS)},
                "ts": NOW + k}
        assert client.post("/ingest", json=body).status_code == 200
    ts = NOW + W - 1
    r0 = client.post("/timestamp", json={"Timestamp": ts}).json()
    assert r0["ok"] and r0["predictions"]["S0"]["model"] == 0

    r = client.post("/assign", json={"symbol": "S0", "slot": 2})
    assert r.status_code == 200 and r.json()["model_of"]["S0"] == 2
    assert client.get("/healthz").json()["model_of"]["S0"] == 2
    r1 = client.post("/timestamp", json={"Timestamp": ts}).json()
    assert r1["predictions"]["S0"]["model"] == 2
    assert r1["predictions"]["S0"]["probabilities"] != \
        r0["predictions"]["S0"]["probabilities"]
    assert r1["predictions"]["S1"] == r0["predictions"]["S1"]

    assert client.post("/assign",
                       json={"symbol": "ZZZ", "slot": 0}).status_code == 404
    assert client.post("/assign",
                       json={"symbol": "S0", "slot": 9}).status_code == 422
    assert client.post("/assign", json={"symbol": "S0"}).status_code == 422
    assert bank.model_of()["S0"] == 2

    # a plain fleet app has no such route
    x_min, x_max = _tables()
    plain = TestClient(create_fleet_app(
        FleetPredictor(models[0], SYMS, x_min, x_max, W, use_graph=False)))
    assert plain.post("/assign",
                      json={"symbol": "S0", "slot": 0}).status_code == 404
    assert "model_of" not in plain.get("/healthz").json()
