"""Fleet streaming predictor: one model, many instruments, one tick.

StreamingPredictor serves a single instrument: one ring, one (x_min, x_max)
table, one captured batch-1 graph whose recurrence runs 2 blocks on a
256-CU device. FleetPredictor keeps S rings side by side, each with its own
normalisation table (price levels differ per ticker), and scores all of
them in ONE captured graph replay:

  push_rows   -> one H2D copy of the staged rows + active mask and one
                 `ingest_rows` launch (block s shifts + normalises ring s,
                 inactive symbols are left untouched)
  predict_all -> per layer one gi GEMM over the (S*T, F_in) view and one
                 `gru_fwd_streams` launch on a (n_dir, S) grid — the
                 batch-1 LDS-resident recurrence, one block per
                 (direction, stream) — then pool_concat_infer and
                 head_sigmoid at B = S, and the (S, C) probabilities copied
                 to pinned host memory inside the graph.

Path selection mirrors StreamingPredictor: the GPU-resident fast path needs
CUDA, bf16 and an unpadded hidden size; H == 128 within the LDS cap takes
`gru_fwd_streams` while its (n_dir, S) grid fits the device's CUs in one
round, larger fleets and other unpadded sizes take the batch-tiled
`gru_fwd` at B = S (FMDA_FLEET_B1=0 forces that route, =1 forces the
streams kernel where it is eligible, for A/B runs). Everything else (padded H, fp32,
CPU) runs sigmoid(model(x)) on an (S, W, F) batch assembled from host
rings; the CPU path is the oracle.
"""
import os
import threading
import time
from typing import Dict, Iterable, List, Optional, Sequence

import torch

from ..features import TARGET_NAMES
from ..models.bigru import BiGRU
from .bus import MessageBus

_INGEST_BOUND = 48 * 1024       # (T-1)*F one-workgroup bound of the kernels
_B1_LDS_CAP = 150 * 1024        # LDS residency cap of the batch-1 recurrence


def _b1_lds_bytes(T: int, Hp: int = 128) -> int:
    return 2 * T * (3 * Hp + 8) + 2 * 2 * (Hp + 8) + 4 * 3 * Hp


class FleetPredictor:
    def __init__(self, model: BiGRU, symbols: Sequence[str],
                 x_min: torch.Tensor, x_max: torch.Tensor, window: int,
                 bus: Optional[MessageBus] = None,
                 prob_threshold: float = 0.5, stale_after: float = 240.0,
                 device: str = "cpu", dtype: torch.dtype = torch.float32,
                 use_graph: Optional[bool] = None,
                 settle_delay: float = 0.0):
        self.symbols: List[str] = list(symbols)
        if not self.symbols:
            raise ValueError("FleetPredictor needs at least one symbol")
        if len(set(self.symbols)) != len(self.symbols):
            raise ValueError("FleetPredictor symbols must be unique")
        self._index = {s: i for i, s in enumerate(self.symbols)}
        S = len(self.symbols)
        self.model = model.eval().to(device)
        self.window = window
        self.n_features = F = model.n_features
        self.bus = bus or MessageBus()
        self.prob_threshold = prob_threshold
        self.stale_after = stale_after
        self.settle_delay = settle_delay
        self.device = torch.device(device)
        self.dtype = dtype
        self.y_fields: List[str] = list(TARGET_NAMES)

        x_min = torch.as_tensor(x_min).float()
        x_max = torch.as_tensor(x_max).float()
        if x_min.dim() == 1:
            x_min = x_min.unsqueeze(0).expand(S, F)
        if x_max.dim() == 1:
            x_max = x_max.unsqueeze(0).expand(S, F)
        if tuple(x_min.shape) != (S, F) or tuple(x_max.shape) != (S, F):
            raise ValueError(
                f"x_min / x_max must be ({F},) or ({S}, {F}), got "
                f"{tuple(x_min.shape)} / {tuple(x_max.shape)}")
        self.x_min = x_min.clone()
        # same degenerate-range clamp as StreamingPredictor
        self.x_rng = (x_max - x_min).clamp(min=1e-6)

        # per-symbol state, guarded by _lock (serve handlers run on a
        # threadpool); the settle sleep of handle_timestamp stays outside
        self._lock = threading.Lock()
        self.count = [0] * S
        self.last_row_ts: List[Optional[float]] = [None] * S
        self.n_dropped_missing: Dict[str, int] = {s: 0 for s in self.symbols}
        self.n_retries = 0
        self.n_stale = 0
        self.n_predictions = 0
        self.n_captures = 0

        self._graph = None
        self._use_graph = (self.device.type == "cuda"
                           if use_graph is None else use_graph)
        self._static_out = None
        self._pinned_out = None

        self._gpu_fast = False
        self.route = "model"
        if self.device.type == "cuda" and dtype == torch.bfloat16:
            from ..ops.interface import _pad_h
            H = model.hidden_size
            if _pad_h(H) == H and (window - 1) * F <= _INGEST_BOUND:
                self._gpu_fast = True
                # one (direction, stream) block per CU: while the grid
                # fits the device in one round the S streams cost the
                # latency of one. A second round doubles the recurrence,
                # and from there the batch-tiled kernel measured faster
                # (profiles/fleet_predict.md: 129 and 256 bidirectional
                # streams on 256 CUs), so the route follows the CU count.
                n_cu = torch.cuda.get_device_properties(
                    self.device).multi_processor_count
                # FMDA_FLEET_B1=0 / =1 force either side for A/B runs.
                force = os.environ.get("FMDA_FLEET_B1", "")
                b1 = (H == 128 and _b1_lds_bytes(window) <= _B1_LDS_CAP
                      and force != "0"
                      and (force == "1"
                           or S * model.n_directions <= n_cu))
                self.route = "streams" if b1 else "gru_fwd"
        if self._gpu_fast:
            dev = self.device
            self._rings_gpu = torch.zeros(S, window, F, device=dev,
                                          dtype=torch.bfloat16)
            self._rows_pin = torch.zeros(S, F, pin_memory=True)
            self._active_pin = torch.zeros(S, dtype=torch.int32,
                                           pin_memory=True)
            self._rows_gpu = torch.zeros(S, F, device=dev)
            self._active_gpu = torch.zeros(S, dtype=torch.int32, device=dev)
            self._xmin_gpu = self.x_min.contiguous().to(dev)
            self._xrng_gpu = self.x_rng.contiguous().to(dev)
            # the staging buffers are rewritten every tick: the previous
            # tick's H2D copies must have left them first
            self._h2d_done = torch.cuda.Event()
            self._h2d_pending = False
        else:
            self.rings = torch.zeros(S, window, F)
            self._static_in = torch.zeros(S, window, F, device=self.device,
                                          dtype=self.dtype)

    # ---------------- bookkeeping ----------------

    def _idx(self, symbol: str) -> int:
        try:
            return self._index[symbol]
        except KeyError:
            raise KeyError(f"unknown symbol {symbol!r}") from None

    def window_full(self) -> Dict[str, bool]:
        with self._lock:
            return {s: self.count[i] >= self.window
                    for i, s in enumerate(self.symbols)}

    # ---------------- feature ingestion ----------------

    def push_rows(self, rows: Dict[str, torch.Tensor],
                  ts: Optional[float] = None) -> None:
        """Ingest one raw (unnormalized) row for each of the given symbols;
        the other symbols' windows do not move."""
        idx = [self._idx(s) for s in rows]     # KeyError before any change
        if not idx:
            return
        # a handful of tensor ops whatever the fleet size: per-symbol
        # indexing of the staging buffers costs microseconds per symbol
        vals = torch.stack([torch.as_tensor(r) for r in rows.values()]
                           ).float().reshape(len(idx), self.n_features)
        with self._lock:
            if self._gpu_fast:
                from ..ops import load_extension
                ext = load_extension()
                if self._h2d_pending:
                    self._h2d_done.synchronize()
                idx_t = torch.tensor(idx)
                self._rows_pin.index_copy_(0, idx_t, vals)
                self._active_pin.zero_()
                self._active_pin.index_fill_(0, idx_t, 1)
                self._rows_gpu.copy_(self._rows_pin, non_blocking=True)
                self._active_gpu.copy_(self._active_pin, non_blocking=True)
                self._h2d_done.record()
                self._h2d_pending = True
                ext.ingest_rows(self._rings_gpu, self._rows_gpu,
                                self._active_gpu, self._xmin_gpu,
                                self._xrng_gpu)
            else:
                for i, v in zip(idx, vals):
                    self.rings[i] = torch.roll(self.rings[i], -1, dims=0)
                    self.rings[i, -1] = v
            # published AFTER the rows are in (or enqueued for) the rings
            for i in idx:
                self.count[i] += 1
                if ts is not None:
                    self.last_row_ts[i] = ts

    def push_row(self, symbol: str, row: torch.Tensor,
                 ts: Optional[float] = None) -> None:
        self.push_rows({symbol: row}, ts=ts)

    def warm_start(self, history: torch.Tensor) -> None:
        """Apply history (S, n, F) as n all-active ticks, oldest first: n
        ingest launches instead of S*n. Equivalent to pushing the rows one
        at a time."""
        S, F = len(self.symbols), self.n_features
        history = torch.as_tensor(history).float()
        if history.dim() != 3 or history.shape[0] != S \
                or history.shape[2] != F:
            raise ValueError(f"history must be ({S}, n, {F}), got "
                             f"{tuple(history.shape)}")
        n = history.shape[1]
        with self._lock:
            if self._gpu_fast:
                from ..ops import load_extension
                ext = load_extension()
                ticks = history.to(self.device).transpose(0, 1).contiguous()
                on = torch.ones(S, dtype=torch.int32, device=self.device)
                for k in range(n):
                    ext.ingest_rows(self._rings_gpu, ticks[k], on,
                                    self._xmin_gpu, self._xrng_gpu)
            else:
                for k in range(n):
                    self.rings = torch.roll(self.rings, -1, dims=1)
                    self.rings[:, -1] = history[:, k]
            for i in range(S):
                self.count[i] += n

    # ---------------- the batch-S step ----------------

    def _fast_forward(self) -> torch.Tensor:
        """Direct-kernel forward over the S GPU rings: per layer one gi
        GEMM over the (S*T, F_in) view + one recurrence launch, then fused
        pool/concat and fused head+sigmoid at B = S. Returns (S, C) fp32."""
        from ..ops import load_extension
        from ..ops.interface import (_layer_params, _packed_inference_weights,
                                     _pad_h)
        ext = load_extension()
        m = self.model
        H = m.hidden_size
        Hp = _pad_h(H)
        D = m.n_directions
        S, T = len(self.symbols), self.window
        inp = self._rings_gpu.view(S * T, -1)
        out = hl = None
        for layer in range(m.n_layers):
            w_ih, b_ih, w_hh, b_hh = _packed_inference_weights(
                m.gru, layer, _layer_params(m.gru, layer, D), Hp, H,
                self.dtype)
            gi = torch.addmm(b_ih, inp, w_ih.t()).view(S, T, -1)
            if self.route == "streams":
                out, hl = ext.gru_fwd_streams(gi, w_hh, b_hh)
            else:
                out, hl = ext.gru_fwd(gi, w_hh, b_hh)
            inp = out.view(S * T, -1)
        feat = ext.pool_concat_infer(out, hl, H)
        if not hasattr(self, "_head_wb"):
            self._head_wb = (m.linear.weight.to(self.dtype).contiguous(),
                             m.linear.bias.to(self.dtype).contiguous())
        return ext.head_sigmoid(feat, *self._head_wb)

    def _capture_graph(self) -> None:
        fwd = (self._fast_forward if self._gpu_fast else
               lambda: torch.sigmoid(self.model(self._static_in)))
        # warmup on a side stream (required before capture)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(3):
                fwd()
        torch.cuda.current_stream().wait_stream(s)
        self._pinned_out = None
        self.n_captures += 1
        if self._gpu_fast:
            # the D2H probs copy is captured INTO the graph (pinned dst):
            # one replay + one stream sync per tick, as the single predictor
            pin = torch.zeros(len(self.symbols), self.model.output_size,
                              dtype=torch.float32, pin_memory=True)
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g), torch.no_grad():
                    self._static_out = fwd()
                    pin.copy_(self._static_out, non_blocking=True)
                self._graph = g
                self._pinned_out = pin
                return
            except RuntimeError:
                pass  # D2H capture unsupported: plain graph below
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), torch.no_grad():
            self._static_out = fwd()
        self._graph = g

    def _probs_locked(self) -> List[List[float]]:
        """(S, C) probabilities of all rings as nested lists."""
        if self._gpu_fast and self._use_graph:
            if self._graph is None:
                self._capture_graph()
            self._graph.replay()
            torch.cuda.current_stream().synchronize()
            if self._pinned_out is not None:
                return self._pinned_out.tolist()
            return self._static_out.cpu().tolist()
        if self._gpu_fast:
            with torch.no_grad():
                return self._fast_forward().cpu().tolist()
        x_norm = (self.rings - self.x_min.unsqueeze(1)) \
            / self.x_rng.unsqueeze(1)
        if self._use_graph:
            if self._graph is None:
                self._capture_graph()
            self._static_in.copy_(x_norm.to(self.device, self.dtype))
            self._graph.replay()
            return self._static_out.float().cpu().tolist()
        with torch.no_grad():
            x = x_norm.to(self.device, self.dtype)
            return torch.sigmoid(self.model(x)).float().cpu().tolist()

    def _predict_locked(self, only: Optional[Iterable[int]] = None
                        ) -> Dict[str, Dict]:
        want = range(len(self.symbols)) if only is None else only
        ready = [i for i in want if self.count[i] >= self.window]
        if not ready:
            return {}
        probs = self._probs_locked()
        self.n_predictions += 1
        res = {}
        for i in ready:
            pl = probs[i]
            idx = [k for k, v in enumerate(pl) if v > self.prob_threshold]
            res[self.symbols[i]] = {
                "probabilities": pl,
                "prob_threshold": self.prob_threshold,
                "pred_indices": idx,
                "pred_labels": [self.y_fields[k] for k in idx]}
        return res

    def predict_all(self) -> Dict[str, Dict]:
        """Score every symbol whose window is full: one forward (one graph
        replay and one stream sync on the GPU) for the whole fleet. Values
        have the shape of StreamingPredictor.predict_window()."""
        with self._lock:
            return self._predict_locked()

    # ---------------- message loop ----------------

    def score_timestamp(self, msg: Dict, now: Optional[float] = None) -> Dict:
        """Process one predict_timestamp message for the whole fleet and
        say what became of it: {"stale": bool, "predictions": {symbol:
        dict}, "dropped": [symbols still lagging after the settle retry],
        "not_full": [symbols whose window is not full yet]}. Predictions
        are published to the `prediction` topic, one message per symbol."""
        ts = float(msg["Timestamp"])
        now = time.time() if now is None else now
        res = {"stale": False, "predictions": {}, "dropped": [],
               "not_full": []}
        if ts <= now - self.stale_after:    # stale filter (predict.py:135)
            with self._lock:
                self.n_stale += 1
            res["stale"] = True
            return res

        def lagging():
            return [i for i, t in enumerate(self.last_row_ts)
                    if t is not None and t < ts]

        # delayed-data tolerance (predict.py:141-157) for the fleet: if any
        # symbol's row has not landed, wait ONCE for the settle delay
        # (outside the lock, so concurrent push_rows can satisfy the
        # retry), then score the symbols that are ready and drop the rest
        with self._lock:
            retry = bool(lagging())
            if retry:
                self.n_retries += 1
        if retry and self.settle_delay > 0:
            time.sleep(self.settle_delay)
        with self._lock:
            late = set(lagging()) if retry else set()
            for i in sorted(late):
                self.n_dropped_missing[self.symbols[i]] += 1
                res["dropped"].append(self.symbols[i])
            keep = [i for i in range(len(self.symbols)) if i not in late]
            res["not_full"] = [self.symbols[i] for i in keep
                               if self.count[i] < self.window]
            preds = self._predict_locked(keep)
        for sym, pred in preds.items():
            pred["symbol"] = sym
            pred["timestamp"] = ts
            self.bus.publish("prediction", pred)
        res["predictions"] = preds
        return res

    def handle_timestamp(self, msg: Dict, now: Optional[float] = None
                         ) -> Optional[Dict[str, Dict]]:
        """One predict_timestamp message scores the whole fleet; returns
        {symbol: published prediction} or None if the message was stale."""
        res = self.score_timestamp(msg, now=now)
        return None if res["stale"] else res["predictions"]

    def run(self, max_messages: Optional[int] = None,
            timeout: Optional[float] = 1.0) -> int:
        """Consume predict_timestamp messages until the topic drains (or
        max_messages). The consumer offset persists across calls."""
        topic = self.bus.topic("predict_timestamp")
        if not hasattr(self, "_offset"):
            self._offset = 0
        n = 0
        while True:
            msg = topic.read(self._offset, timeout=timeout)
            if msg is None:
                break
            self._offset += 1
            self.handle_timestamp(msg)
            n += 1
            if max_messages is not None and n >= max_messages:
                break
        return n
