"""HTTP serving surface for the streaming predictor.

The reference publishes predictions to a Kafka `prediction` topic for
downstream consumers (predict.py:193-197). This module puts the same
predictor behind a FastAPI app for deployments where consumers pull over
HTTP instead of subscribing to a topic:

- POST /ingest        {"row": [108 floats], "Timestamp": t}  -> ring push
- POST /timestamp     {"Timestamp": t}  -> run the predict step (stale
                      messages are dropped exactly like predict.py:135)
- GET  /prediction/latest               -> last prediction dict
- GET  /healthz                         -> liveness + model/config info
- GET  /metrics                         -> Prometheus exposition

Run: uvicorn "fmda_amd.serve:build_app_from_artifacts(...)" or see
`create_app` for wiring an existing StreamingPredictor. On an MI355X the
predictor's batch-1 step is the hipGraph-captured HIP engine path.

`create_fleet_app` / `build_fleet_app_from_artifacts` are the same surface
for a FleetPredictor: many symbols, one model, one captured tick.
"""
import time
from typing import Optional

import torch

try:
    from prometheus_client import (CONTENT_TYPE_LATEST, CollectorRegistry,
                                   Counter, Histogram, generate_latest)
    _PROM = True
except ImportError:  # pragma: no cover
    _PROM = False

from .runtime.fleet import FleetPredictor
from .runtime.fleet_bank import BankedFleetPredictor
from .runtime.streaming import StreamingPredictor


def create_app(predictor: StreamingPredictor):
    from fastapi import FastAPI
    from fastapi.responses import Response

    app = FastAPI(title="fmda_amd streaming predictor")
    state = {"latest": None, "n_ingested": 0}

    if _PROM:
        # per-app registry: multiple app instances (tests, multi-model
        # deployments) must not collide in the global default registry
        reg = CollectorRegistry()
        c_pred = Counter("fmda_predictions_total",
                         "prediction steps served", registry=reg)
        c_stale = Counter("fmda_stale_dropped_total",
                          "timestamp messages dropped as stale", registry=reg)
        c_rows = Counter("fmda_rows_ingested_total", "feature rows pushed",
                         registry=reg)
        h_lat = Histogram(
            "fmda_predict_latency_seconds", "predict step wall latency",
            buckets=(1e-4, 2.5e-4, 5e-4, 1e-3, 2.5e-3, 5e-3, 1e-2, 5e-2),
            registry=reg)

    @app.post("/ingest")
    def ingest(msg: dict):
        row = torch.tensor(msg["row"], dtype=torch.float32)
        predictor.push_row(row)
        state["n_ingested"] += 1
        if _PROM:
            c_rows.inc()
        return {"ok": True, "rows": state["n_ingested"],
                "window_full": predictor.ring.full}

    @app.post("/timestamp")
    def timestamp(msg: dict):
        t0 = time.perf_counter()
        pred = predictor.handle_timestamp(msg)
        if pred is None:
            if _PROM and predictor.ring.full:
                c_stale.inc()
            return {"ok": False,
                    "reason": ("stale" if predictor.ring.full
                               else "window_not_full")}
        state["latest"] = pred
        if _PROM:
            c_pred.inc()
            h_lat.observe(time.perf_counter() - t0)
        return {"ok": True, "prediction": pred}

    @app.get("/prediction/latest")
    def latest():
        return {"prediction": state["latest"]}

    @app.get("/healthz")
    def healthz():
        return {"ok": True,
                "device": str(predictor.device),
                "window": predictor.window,
                "n_features": predictor.n_features,
                "hipgraph": predictor._use_graph,
                "n_predictions": predictor.n_predictions}

    @app.get("/metrics")
    def metrics():
        if not _PROM:  # pragma: no cover
            return Response("prometheus_client not installed",
                            media_type="text/plain")
        return Response(generate_latest(reg),
                        media_type=CONTENT_TYPE_LATEST)

    return app


def build_app_from_artifacts(checkpoint: str = "model_params.pt",
                             norm_params: str = "norm_params",
                             window: int = 30,
                             device: Optional[str] = None):
    """App factory from the reference-format artifacts (the same pair
    predict.py loads at :104 and :110-122)."""
    from .data.norm import load_norm_params
    from .models.checkpoint import load_checkpoint

    model = load_checkpoint(checkpoint)
    _, x_min, x_max = load_norm_params(norm_params)
    if device is None:
        device = "cuda:0" if torch.cuda.is_available() else "cpu"
    dtype = torch.bfloat16 if device.startswith("cuda") else torch.float32
    if dtype is torch.bfloat16:
        model = model.to(dtype)
    pred = StreamingPredictor(model, x_min, x_max, window, device=device,
                              dtype=dtype)
    return create_app(pred)


def create_fleet_app(predictor: FleetPredictor):
    """The multi-instrument surface: one model, S symbols, one tick.

    - POST /ingest        {"rows": {symbol: [floats]}, "ts": optional}
    - POST /timestamp     {"Timestamp": t}  -> score the whole fleet
    - GET  /prediction/latest[?symbol=X]    -> last prediction per symbol
    - GET  /healthz                         -> symbols, window, device,
                                               per-symbol window_full
    - GET  /metrics                         -> Prometheus exposition

    A BankedFleetPredictor (a bank of models, one slot per symbol) is
    served unchanged and adds:
    - POST /assign        {"symbol": s, "slot": k}  -> score s with model k
    - GET  /healthz also reports the symbol -> slot map ("model_of")
    """
    from fastapi import FastAPI, HTTPException
    from fastapi.responses import Response

    app = FastAPI(title="fmda_amd fleet predictor")
    latest = {}

    if _PROM:
        reg = CollectorRegistry()   # per app, as in create_app
        c_pred = Counter("fmda_fleet_predictions_total",
                         "predictions served", ["symbol"], registry=reg)
        c_rows = Counter("fmda_fleet_rows_ingested_total",
                         "feature rows pushed", ["symbol"], registry=reg)
        c_stale = Counter("fmda_fleet_stale_dropped_total",
                          "timestamp messages dropped as stale",
                          registry=reg)
        c_settle = Counter("fmda_fleet_settle_dropped_total",
                           "symbols dropped from a tick because their row "
                           "had not landed after the settle retry",
                           registry=reg)
        h_lat = Histogram(
            "fmda_fleet_tick_latency_seconds", "fleet tick wall latency",
            buckets=(1e-4, 2.5e-4, 5e-4, 1e-3, 2.5e-3, 5e-3, 1e-2, 5e-2),
            registry=reg)

    @app.post("/ingest")
    def ingest(msg: dict):
        rows = {s: torch.tensor(r, dtype=torch.float32)
                for s, r in msg["rows"].items()}
        try:
            predictor.push_rows(rows, ts=msg.get("ts"))
        except KeyError as e:
            raise HTTPException(status_code=404, detail=str(e.args[0]))
        if _PROM:
            for s in rows:
                c_rows.labels(symbol=s).inc()
        return {"ok": True, "window_full": predictor.window_full()}

    @app.post("/timestamp")
    def timestamp(msg: dict):
        t0 = time.perf_counter()
        res = predictor.score_timestamp(msg)
        if res["stale"]:
            if _PROM:
                c_stale.inc()
            return {"ok": False, "reason": "stale"}
        preds = res["predictions"]
        latest.update(preds)
        if _PROM:
            c_settle.inc(len(res["dropped"]))
            for s in preds:
                c_pred.labels(symbol=s).inc()
            if preds:
                h_lat.observe(time.perf_counter() - t0)
        return {"ok": bool(preds), "predictions": preds,
                "dropped": res["dropped"], "not_full": res["not_full"]}

    @app.get("/prediction/latest")
    def latest_prediction(symbol: Optional[str] = None):
        if symbol is None:
            return {"predictions": dict(latest)}
        if symbol not in predictor.symbols:
            raise HTTPException(status_code=404,
                                detail=f"unknown symbol {symbol!r}")
        return {"prediction": latest.get(symbol)}

    banked = isinstance(predictor, BankedFleetPredictor)

    @app.get("/healthz")
    def healthz():
        res = {"ok": True,
               "symbols": list(predictor.symbols),
               "device": str(predictor.device),
               "window": predictor.window,
               "n_features": predictor.n_features,
               "route": predictor.route,
               "window_full": predictor.window_full(),
               "n_predictions": predictor.n_predictions}
        if banked:
            res["model_of"] = predictor.model_of()
            res["n_models"] = len(predictor.models)
        return res

    if banked:
        @app.post("/assign")
        def assign(msg: dict):
            if "symbol" not in msg or "slot" not in msg:
                raise HTTPException(status_code=422,
                                    detail="need symbol and slot")
            try:
                predictor.assign(msg["symbol"], msg["slot"])
            except KeyError as e:
                raise HTTPException(status_code=404, detail=str(e.args[0]))
            except ValueError as e:
                raise HTTPException(status_code=422, detail=str(e))
            return {"ok": True, "model_of": predictor.model_of()}

    @app.get("/metrics")
    def metrics():
        if not _PROM:  # pragma: no cover
            return Response("prometheus_client not installed",
                            media_type="text/plain")
        return Response(generate_latest(reg),
                        media_type=CONTENT_TYPE_LATEST)

    return app


def build_fleet_app_from_artifacts(checkpoint: str = "model_params.pt",
                                   norm_params: str = "norm_params",
                                   symbols=(),
                                   window: int = 30,
                                   device: Optional[str] = None):
    """Fleet app factory from the reference-format artifacts; the one
    norm_params table is applied to every symbol."""
    from .data.norm import load_norm_params
    from .models.checkpoint import load_checkpoint

    model = load_checkpoint(checkpoint)
    _, x_min, x_max = load_norm_params(norm_params)
    if device is None:
        device = "cuda:0" if torch.cuda.is_available() else "cpu"
    dtype = torch.bfloat16 if device.startswith("cuda") else torch.float32
    if dtype is torch.bfloat16:
        model = model.to(dtype)
    pred = FleetPredictor(model, list(symbols), x_min, x_max, window,
                          device=device, dtype=dtype)
    return create_fleet_app(pred)
