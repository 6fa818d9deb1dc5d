"""Fleet predictor with a bank of models: per-instrument weights, hot swap.

FleetPredictor scores S instruments in one captured tick, all through one
BiGRU. BankedFleetPredictor keeps M models of one shape side by side and a
symbol -> slot map: one model per symbol or per asset class, or a challenger
beside the champion on a few symbols, still in ONE graph replay and one
stream sync per tick.

  predict_all -> per layer one `gi_proj_bank` (the grouped input projection:
                 stream s through W_ih[slot[s]]) and one
                 `gru_fwd_streams_bank` (the batch-1 recurrence, block
                 (d, s) on W_hh[slot[s]]), then pool_concat_infer and
                 `head_sigmoid_bank`, and the (S, C) probabilities copied to
                 pinned host memory inside the graph.

The kernels read the slot of a stream from a device int32 (S) tensor and
the weights from per-layer bank tensors built once; the captured graph only
ever sees their storage. `assign` rewrites one entry of the slot tensor and
`swap_model` copies a model's packed weights into its bank slot in place,
so both take effect on the next tick without a capture.

The GPU fast path (route "streams_bank") needs what FleetPredictor's needs
(CUDA, bf16, unpadded H, the ingest bound) plus H == 128 within the batch-1
LDS cap; it is taken whatever the CU count. Every other case (route
"grouped") groups the symbols by slot and runs sigmoid(model_m(x[rows]))
per group, uncaptured; on the CPU that is the oracle.
"""
import operator
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Union

import torch

from ..models.bigru import BiGRU
from .bus import MessageBus
from .fleet import _B1_LDS_CAP, FleetPredictor, _b1_lds_bytes

_SHAPE_FIELDS = ("hidden_size", "n_features", "n_layers", "n_directions",
                 "output_size")


def _check_same_shape(ref: BiGRU, model: BiGRU, what: str) -> None:
    for f in _SHAPE_FIELDS:
        if getattr(model, f) != getattr(ref, f):
            raise ValueError(
                f"{what}: {f} = {getattr(model, f)} does not match the "
                f"bank's {getattr(ref, f)}")


class BankedFleetPredictor(FleetPredictor):
    def __init__(self, models: Sequence[BiGRU], symbols: Sequence[str],
                 model_of: Union[Mapping[str, int], Sequence[int]],
                 x_min: torch.Tensor, x_max: torch.Tensor, window: int,
                 bus: Optional[MessageBus] = None,
                 prob_threshold: float = 0.5, stale_after: float = 240.0,
                 device: str = "cpu", dtype: torch.dtype = torch.float32,
                 use_graph: Optional[bool] = None,
                 settle_delay: float = 0.0):
        models = list(models)
        if not models:
            raise ValueError("BankedFleetPredictor needs at least one model")
        for k, m in enumerate(models[1:], start=1):
            _check_same_shape(models[0], m, f"models[{k}]")
        super().__init__(models[0], symbols, x_min, x_max, window, bus=bus,
                         prob_threshold=prob_threshold,
                         stale_after=stale_after, device=device, dtype=dtype,
                         use_graph=use_graph, settle_delay=settle_delay)
        self.models: List[BiGRU] = [m.eval().to(device) for m in models]
        S, M = len(self.symbols), len(self.models)
        if isinstance(model_of, Mapping):
            missing = [s for s in self.symbols if s not in model_of]
            if missing:
                raise ValueError(f"model_of has no slot for {missing}")
            slots = [model_of[s] for s in self.symbols]
        else:
            slots = list(model_of)
            if len(slots) != S:
                raise ValueError(
                    f"model_of must give {S} slots, got {len(slots)}")
        self._slot_of: List[int] = [self._check_slot(k) for k in slots]

        # FleetPredictor chose the ingestion side (_gpu_fast: GPU rings and
        # the ingest kernel); the banked kernels add H == 128 and the LDS
        # cap. A second round of blocks on a large fleet still replaces M
        # launches, so there is no CU-count crossover here.
        self._bank_fast = (self._gpu_fast and models[0].hidden_size == 128
                           and _b1_lds_bytes(window) <= _B1_LDS_CAP)
        self.route = "streams_bank" if self._bank_fast else "grouped"
        if self._bank_fast:
            packs = [self._packed(m) for m in self.models]
            n_layers = models[0].n_layers
            # per layer (w_ih (M, N, K), b_ih (M, N), w_hh (M, D, 3Hp, Hp),
            # b_hh (M, D, 3Hp)) and the heads (W (M, C, 3H), b (M, C))
            self._banks = [tuple(torch.stack([p[l][j] for p in packs])
                                 for j in range(4))
                           for l in range(n_layers)]
            self._head_bank = tuple(torch.stack([p[n_layers][j]
                                                 for p in packs])
                                    for j in range(2))
            self._slot_gpu = torch.tensor(self._slot_of, dtype=torch.int32,
                                          device=self.device)

    # ---------------- the bank ----------------

    def _check_slot(self, slot) -> int:
        try:
            k = None if isinstance(slot, bool) else operator.index(slot)
        except TypeError:
            k = None
        if k is None or not 0 <= k < len(self.models):
            raise ValueError(f"slot {slot!r} is not an index in "
                             f"[0, {len(self.models)})")
        return k

    def _packed(self, model: BiGRU):
        """Packed weights of one model in the layouts the bank stacks: per
        layer (w_ih, b_ih, w_hh, b_hh), then (head W, head b)."""
        from ..ops.interface import (_layer_params, _packed_inference_weights,
                                     _pad_h)
        H, D = model.hidden_size, model.n_directions
        with torch.no_grad():
            layers = [_packed_inference_weights(
                model.gru, l, _layer_params(model.gru, l, D), _pad_h(H), H,
                self.dtype) for l in range(model.n_layers)]
            head = (model.linear.weight.to(self.dtype).contiguous(),
                    model.linear.bias.to(self.dtype).contiguous())
        return layers + [head]

    def model_of(self) -> Dict[str, int]:
        with self._lock:
            return dict(zip(self.symbols, self._slot_of))

    def assign(self, symbol: str, slot: int) -> None:
        """Score `symbol` with the model in `slot` from the next tick on.
        On the GPU this rewrites one entry of the device slot tensor, which
        the captured graph reads through a fixed pointer: no re-capture."""
        i = self._idx(symbol)                 # KeyError before any change
        slot = self._check_slot(slot)
        with self._lock:
            self._slot_of[i] = slot
            if self._bank_fast:
                self._slot_gpu[i] = slot

    def swap_model(self, slot: int, model: BiGRU) -> None:
        """Replace the model in `slot`; the next predict_all uses it. On
        the GPU its packed weights are copied into the bank slot in place,
        on the current stream, so the captured graph stays as it is."""
        slot = self._check_slot(slot)
        # the rings, the banks and the graph are built to the bank's shape
        _check_same_shape(self.models[0], model, "swap_model")
        with self._lock:
            model = model.eval().to(self.device)
            if self._bank_fast:
                pack = self._packed(model)
                for bank, new in zip(self._banks, pack):
                    for dst, src in zip(bank, new):
                        dst[slot].copy_(src)
                for dst, src in zip(self._head_bank, pack[-1]):
                    dst[slot].copy_(src)
            self.models[slot] = model
            if slot == 0:
                self.model = model

    # ---------------- the batch-S step ----------------

    def _fast_forward(self) -> torch.Tensor:
        """Direct-kernel forward over the S GPU rings with per-stream
        weights: per layer one grouped projection + one recurrence launch,
        then fused pool/concat and the banked head. Returns (S, C) fp32."""
        from ..ops import load_extension
        ext = load_extension()
        slot = self._slot_gpu
        inp = self._rings_gpu
        out = hl = None
        for w_ih, b_ih, w_hh, b_hh in self._banks:
            gi = ext.gi_proj_bank(inp, slot, w_ih, b_ih)
            out, hl = ext.gru_fwd_streams_bank(gi, slot, w_hh, b_hh)
            inp = out
        feat = ext.pool_concat_infer(out, hl, self.models[0].hidden_size)
        return ext.head_sigmoid_bank(feat, slot, *self._head_bank)

    def _grouped_probs(self) -> List[List[float]]:
        """The fallback and the oracle: one eager forward per slot over the
        rows of the symbols assigned to it."""
        if self._gpu_fast:
            x = self._rings_gpu
        else:
            x = ((self.rings - self.x_min.unsqueeze(1))
                 / self.x_rng.unsqueeze(1)).to(self.device, self.dtype)
        S = len(self.symbols)
        probs = torch.empty(S, self.models[0].output_size)
        with torch.no_grad():
            for m, model in enumerate(self.models):
                rows = [i for i, k in enumerate(self._slot_of) if k == m]
                if not rows:
                    continue
                xm = x if len(rows) == S else x[rows]
                probs[rows] = torch.sigmoid(model(xm)).float().cpu()
        return probs.tolist()

    def _probs_locked(self) -> List[List[float]]:
        if self._bank_fast:
            # FleetPredictor's captured / eager fast path over the banked
            # _fast_forward above
            return super()._probs_locked()
        return self._grouped_probs()

    def _predict_locked(self, only: Optional[Iterable[int]] = None
                        ) -> Dict[str, Dict]:
        res = super()._predict_locked(only)
        for sym, pred in res.items():
            pred["model"] = self._slot_of[self._index[sym]]
        return res
