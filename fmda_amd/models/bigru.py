"""BiGRU model with the reference-compatible public API.

The class signature, parameter names/shapes, checkpoint format and the
train/evaluate loop semantics match the reference `BiGRU`
(biGRU_model.py:8-286): state_dict keys are `gru.weight_ih_l{k}[...]` /
`linear.weight` / `linear.bias`, so the reference `model_params.pt` loads
directly.

Execution paths:
- CPU: PyTorch's own GRU kernels (ATen) — also the golden reference.
- CUDA (ROCm/MI355X): the fmda_amd HIP engine — time-batched input
  projections on MFMA (rocBLAS GEMM) + hand-written persistent CDNA4
  recurrence kernels; no MIOpen RNN, no cuDNN. The HIP extension is
  REQUIRED on GPU: the model raises rather than falling back silently.
"""
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..metrics import batch_metrics


class BiGRU(nn.Module):
    """BiDirectional GRU model (API of reference biGRU_model.py:8-61).

    Parameters
    ----------
    hidden_size: number of features in the hidden state.
    n_features: number of input features.
    output_size: number of classes.
    n_layers: number of stacked recurrent layers.
    clip: max norm of the gradients.
    dropout: probability of an element to be zeroed.
    spatial_dropout: whether to use spatial (per-feature-channel) dropout.
    bidirectional: whether to use the bidirectional GRU.
    """

    def __init__(self, hidden_size, n_features, output_size, n_layers=1,
                 clip=50, dropout=0.2, spatial_dropout=True,
                 bidirectional=True):
        super().__init__()
        self.hidden_size = hidden_size
        self.n_features = n_features
        self.output_size = output_size
        self.n_layers = n_layers
        self.clip = clip
        self.dropout_p = dropout
        self.spatial_dropout = spatial_dropout
        self.bidirectional = bidirectional
        self.n_directions = 2 if bidirectional else 1

        self.dropout = nn.Dropout(self.dropout_p)
        if self.spatial_dropout:
            self.spatial_dropout1d = nn.Dropout2d(self.dropout_p)

        # nn.GRU is the parameter container (state_dict-compatible with the
        # reference) and the CPU execution path. Its forward is NEVER called
        # on a GPU tensor: the CUDA path runs the fmda_amd HIP engine with
        # these same weights.
        self.gru = nn.GRU(self.n_features, self.hidden_size,
                          num_layers=self.n_layers,
                          dropout=(0 if n_layers == 1 else self.dropout_p),
                          batch_first=True, bidirectional=self.bidirectional)

        # Linear head input is hidden_size * 3: concat of summed-last-hidden,
        # max pooling and avg pooling (biGRU_model.py:58-60).
        self.linear = nn.Linear(self.hidden_size * 3, self.output_size)

    # ------------------------------------------------------------------ #

    def forward(self, input_seq: torch.Tensor,
                hidden: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Forward pass; returns (B, output_size) logits
        (semantics of biGRU_model.py:63-138)."""
        return self._head(self.forward_features(input_seq, hidden))

    def _head(self, concat_out: torch.Tensor) -> torch.Tensor:
        """Linear head on the pooled (B, 3H) features -> logits."""
        if concat_out.dtype != self.linear.weight.dtype:
            # bf16 compute path with fp32 master weights: cast the head.
            return F.linear(concat_out, self.linear.weight.to(concat_out.dtype),
                            self.linear.bias.to(concat_out.dtype))
        return self.linear(concat_out)

    def forward_features(self, input_seq: torch.Tensor,
                         hidden: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Everything before the linear head: returns the pooled concat
        (B, 3H) feature vector — the input of the reference's linear head
        (biGRU_model.py:133-137). Used by the fused head+loss kernel."""
        return self._features_after_dropout(
            self._input_dropout(input_seq), hidden)

    def _input_dropout(self, input_seq: torch.Tensor) -> torch.Tensor:
        """Input (spatial) dropout of forward_features
        (biGRU_model.py:87-94)."""
        if self.spatial_dropout:
            if (self.training and input_seq.is_cuda
                    and input_seq.dtype == torch.bfloat16
                    and self.dropout_p > 0):
                # channel-mask HIP kernel: Dropout2d semantics without the
                # permute(0,2,1) round trips (biGRU_model.py:87-94)
                from ..ops.interface import fused_spatial_dropout
                input_seq = fused_spatial_dropout(input_seq, self.dropout_p)
            else:
                # Dropout2d over (B, F, T): zeroes whole feature channels.
                input_seq = input_seq.permute(0, 2, 1)
                input_seq = self.spatial_dropout1d(input_seq)
                input_seq = input_seq.permute(0, 2, 1)
        elif (self.training and input_seq.is_cuda
              and input_seq.dtype == torch.bfloat16 and self.dropout_p > 0):
            from ..ops.interface import fused_dropout
            input_seq = fused_dropout(input_seq, self.dropout_p)
        else:
            input_seq = self.dropout(input_seq)
        return input_seq

    def _features_after_dropout(self, input_seq: torch.Tensor,
                                hidden: Optional[torch.Tensor] = None
                                ) -> torch.Tensor:
        """forward_features from the already dropped input on: the GRU
        stack and the pooled concat."""
        if input_seq.is_cuda:
            from ..ops.interface import (bigru_stack_features,
                                         pooled_features_native)
            if pooled_features_native(input_seq, self.hidden_size):
                # the whole feature path in one HIP kernel each way, from
                # the top layer's raw fp32 final state: no h_n, no casts,
                # no direction sum, no cats (same bits as _pool_concat);
                # in training the top layer's BPTT kernel builds its d_out
                # from the feature gradient itself (fused_pool_bwd_native)
                return bigru_stack_features(
                    input_seq, self.gru, self.n_layers, self.bidirectional,
                    self.dropout_p, self.training, hidden)
            gru_out, h_n = self._gru_hip(input_seq, hidden)
        else:
            gru_out, h_n = self.gru(input_seq, hidden)
        return self._pool_concat(gru_out, h_n)

    def _pool_concat(self, gru_out: torch.Tensor,
                     h_n: torch.Tensor) -> torch.Tensor:
        """3-way pooling head (biGRU_model.py:108-137): concat of the
        direction-summed last hidden state, max pool and avg pool over time
        of gru_out (B, T, D*H) -> (B, 3H)."""
        batch_size = gru_out.size(0)
        input_length = gru_out.size(1)
        hidden_v = h_n.view(self.n_layers, self.n_directions, batch_size,
                            self.hidden_size)
        last_hidden = hidden_v[-1].sum(dim=0)

        if gru_out.is_cuda and self.hidden_size % 2 == 0:
            # fused direction-sum + max/avg pooling HIP kernel (pairs
            # columns; odd H takes the eager path below)
            from ..ops.interface import dirsum_pool
            max_pool, avg_pool = dirsum_pool(gru_out, self.n_directions)
        else:
            if self.bidirectional:
                gru_out = (gru_out[:, :, :self.hidden_size]
                           + gru_out[:, :, self.hidden_size:])
            max_pool = gru_out.max(dim=1).values
            avg_pool = gru_out.sum(dim=1) / float(input_length)

        return torch.cat([last_hidden, max_pool, avg_pool], dim=1)

    def _gru_hip(self, x: torch.Tensor, hidden: Optional[torch.Tensor]):
        """CUDA path: MFMA input projections + persistent HIP recurrence."""
        from ..ops.interface import bigru_stack
        return bigru_stack(x, self.gru, self.n_layers, self.bidirectional,
                           self.dropout_p, self.training, hidden)

    # ------------------------ windowed inference ----------------------- #

    def forward_windows(self, table: torch.Tensor, window: int,
                        stride: int = 1,
                        batch_windows: int = 4096) -> torch.Tensor:
        """Logits (n_windows, output_size) of every sliding window of a
        normalised (N, F) table: row i is what
        forward(table[i*stride : i*stride + window][None]) returns in eval
        mode. On the GPU the layer-0 input projections are computed once
        per table row and shared by all windows that contain the row; the
        windows are never materialised. `batch_windows` windows run per
        launch, so layer outputs stay bounded. On CPU the table is unfolded
        and goes through the ordinary forward, in the same batches."""
        assert not self.training, "forward_windows is inference only: " \
            "call model.eval() first"
        assert table.dim() == 2 and table.size(1) == self.n_features, \
            f"table must be (N, {self.n_features})"
        assert window >= 1 and stride >= 1 and batch_windows >= 1
        assert table.size(0) >= window, "table shorter than one window"
        n_windows = (table.size(0) - window) // stride + 1
        logits = []
        with torch.no_grad():
            gi_rows = None
            if table.is_cuda:
                from ..ops.interface import (bigru_stack_windows,
                                             table_projections)
                gi_rows = table_projections(table, self.gru,
                                            self.bidirectional)
            for w0 in range(0, n_windows, batch_windows):
                nb = min(batch_windows, n_windows - w0)
                r0 = w0 * stride
                r1 = r0 + (nb - 1) * stride + window
                if gi_rows is not None:
                    gru_out, h_n = bigru_stack_windows(
                        table[r0:r1], self.gru, self.n_layers,
                        self.bidirectional, window, stride,
                        gi_rows=gi_rows[r0:r1])
                    logits.append(self._head(self._pool_concat(gru_out, h_n)))
                else:
                    x = table[r0:r1].unfold(0, window, stride)
                    logits.append(self.forward(
                        x.permute(0, 2, 1).contiguous()))
        return torch.cat(logits, dim=0)

    def window_batch_metrics(self, table: torch.Tensor,
                             targets: torch.Tensor, window: int,
                             batch_size: int):
        """Per-batch metrics of the stride-1 windows of one normalised
        (N, F) table, batched like a sequential DataLoader over the
        windows: (accuracies, hamming losses, fbetas, pred, target), the
        first three with one entry per consecutive group of `batch_size`
        windows. The target of a window is the targets row of its last
        timestep. A table shorter than one window has no batches."""
        self.eval()
        empty = torch.LongTensor()
        if table.size(0) < window:
            return [], [], [], empty, empty
        table = table.to(self.device)
        # CPU (the oracle path) forms exactly the DataLoader's batches; the
        # GPU shares projections across larger launches
        bw = max(batch_size, 4096) if table.is_cuda else batch_size
        logits = self.forward_windows(table, window, batch_windows=bw)
        pred_all = torch.sigmoid(logits) > 0.5
        target_all = targets[window - 1:window - 1 + pred_all.size(0)].to(
            self.device)
        accuracies, hamm_losses, fbetas_list = [], [], []
        for b0 in range(0, pred_all.size(0), batch_size):
            acc, ham, fbeta = batch_metrics(target_all[b0:b0 + batch_size],
                                            pred_all[b0:b0 + batch_size],
                                            beta=0.5)
            accuracies.append(float(acc))
            hamm_losses.append(float(ham))
            fbetas_list.append(fbeta.cpu().numpy())
        return (accuracies, hamm_losses, fbetas_list,
                pred_all.cpu().type(torch.LongTensor),
                target_all.cpu().type(torch.LongTensor))

    def evaluate_windows(self, table: torch.Tensor, targets: torch.Tensor,
                         window: int, batch_size: int):
        """evaluate_model over the stride-1 windows of one normalised
        (N, F) table without materialising them: the same 5-tuple (mean
        accuracy, mean Hamming loss, mean per-class fbeta, pred_total,
        target_total) as evaluate_model over a sequential
        DataLoader(BatchLoader(...), batch_size)."""
        accs, hams, fbetas, pred_total, target_total = \
            self.window_batch_metrics(table, targets, window, batch_size)
        return (np.mean(accs), np.mean(hams), np.mean(fbetas, axis=0),
                pred_total, target_total)

    # ---------------------- reference training API --------------------- #

    def add_loss_fn(self, loss_fn):
        """Add loss function to the model (biGRU_model.py:141-145)."""
        self.loss_fn = loss_fn

    def add_optimizer(self, optimizer):
        """Add optimizer to the model (biGRU_model.py:148-152)."""
        self.optimizer = optimizer

    def add_device(self, device=torch.device('cpu')):
        """Specify the device (biGRU_model.py:155-159)."""
        self.device = device

    def forward_features_windows(self, table: torch.Tensor,
                                 starts: torch.Tensor,
                                 window: int) -> torch.Tensor:
        """forward_features of the batch of windows
        table[starts[b] : starts[b] + window] of a normalised (N, F) table.
        In training mode on the bf16 GPU path the batch is written already
        dropped by one kernel (ops.interface.window_batch with this model's
        dropout_p / spatial_dropout); the result equals
        forward_features(table[starts[:, None] + arange(window)]) bit for
        bit under the same RNG state. Every other case gathers and takes
        forward_features' own input dropout. `starts`: int64, validated
        here if it lives on the CPU, trusted if on the table's device."""
        from ..ops.interface import window_batch
        assert table.dim() == 2 and table.size(1) == self.n_features, \
            f"table must be (N, {self.n_features})"
        if (self.training and self.dropout_p > 0 and table.is_cuda
                and table.dtype == torch.bfloat16):
            x = window_batch(table, starts, window, p=self.dropout_p,
                             spatial=self.spatial_dropout)
        else:
            x = self._input_dropout(window_batch(table, starts, window))
        return self._features_after_dropout(x)

    def _loss_weights(self):
        """(weight, pos_weight) of the attached BCEWithLogitsLoss as the
        fused head+loss kernel takes them (ones where the loss has none)."""
        ones = None
        out = []
        for name in ("weight", "pos_weight"):
            w = getattr(self.loss_fn, name, None)
            if w is None:
                if ones is None:
                    ones = torch.ones(self.output_size, device=self.device)
                w = ones
            out.append(w)
        return out

    def train_windows(self, table: torch.Tensor, targets: torch.Tensor,
                      window: int, batch_size: int, shuffle: bool = False):
        """Train on the stride-1 windows of one normalised (N, F) table
        that stays on the device: the training counterpart of
        window_batch_metrics. Batches are groups of `batch_size`
        consecutive windows (the last partial one is kept), as a sequential
        DataLoader over the windows forms them; shuffle=True permutes the
        windows first (torch.randperm on the CPU generator). The target of
        a window is the targets row of its last timestep.

        On the GPU a step is forward_features_windows -> fused_head_loss
        (weights of self.loss_fn) -> backward -> optimizer, where a
        FusedClipAdam clips by itself and any other optimizer is preceded
        by clip_grad_norm_. On CPU a step is train_model's, on the
        gathered windows. Returns the per-batch lists (accuracies, Hamming
        losses, losses, fbetas); a table shorter than one window has no
        batches. Losses and metrics stay on the device until the table is
        done."""
        from ..optim import FusedClipAdam
        self.train()
        if table.size(0) < window:
            return [], [], [], []
        table = table.to(self.device)
        targets = targets.to(self.device)
        n_windows = table.size(0) - window + 1
        order = (torch.randperm(n_windows) if shuffle
                 else torch.arange(n_windows))
        # built here from [0, n_windows): valid by construction, so the
        # per-batch slices go to window_batch as device tensors
        order = order.to(self.device)
        fused = table.is_cuda
        if fused:
            from ..ops.interface import fused_head_loss
            wgt, pw = self._loss_weights()
        losses, accs, hams, fbetas = [], [], [], []
        for b0 in range(0, n_windows, batch_size):
            starts = order[b0:b0 + batch_size]
            target = targets[starts + (window - 1)]
            self.optimizer.zero_grad()
            if fused:
                feats = self.forward_features_windows(table, starts, window)
                loss, pred = fused_head_loss(feats, self.linear.weight,
                                             self.linear.bias, target, wgt,
                                             pw)
            else:
                idx = starts[:, None] + torch.arange(window)
                pred = self.forward(table[idx])
                loss = self.loss_fn(pred, target)
            loss.backward()
            losses.append(loss.detach())
            if not isinstance(self.optimizer, FusedClipAdam):
                nn.utils.clip_grad_norm_(self.parameters(), self.clip)
            self.optimizer.step()

            pred = torch.sigmoid(pred.detach()) > 0.5
            acc, ham, fbeta = batch_metrics(target, pred, beta=0.5)
            accs.append(acc)
            hams.append(ham)
            fbetas.append(fbeta)
        # one transfer per table instead of three syncs per step
        losses = torch.stack(losses).cpu().numpy()
        accs = torch.stack(accs).cpu().numpy()
        hams = torch.stack(hams).cpu().numpy()
        fbetas = torch.stack(fbetas).cpu().numpy()
        return ([float(a) for a in accs], [float(h) for h in hams],
                list(losses), list(fbetas))

    def train_model(self, train_iterator):
        """One training epoch; returns (mean accuracy, mean Hamming loss,
        mean loss, mean per-class fbeta[beta=0.5]) like
        biGRU_model.py:162-224."""
        self.train()
        losses, accuracies, hamm_losses, fbetas_list = [], [], [], []

        for input_seq, target in train_iterator:
            target = target.squeeze(1)
            input_seq = input_seq.to(self.device)
            target = target.to(self.device)

            self.optimizer.zero_grad()
            pred = self.forward(input_seq)
            loss = self.loss_fn(pred, target)
            loss.backward()
            losses.append(loss.detach().cpu().numpy())

            nn.utils.clip_grad_norm_(self.parameters(), self.clip)
            self.optimizer.step()

            pred = torch.sigmoid(pred) > 0.5
            acc, ham, fbeta = batch_metrics(target.detach(), pred.detach(),
                                            beta=0.5)
            accuracies.append(float(acc))
            hamm_losses.append(float(ham))
            fbetas_list.append(fbeta.cpu().numpy())

        return (np.mean(accuracies), np.mean(hamm_losses), np.mean(losses),
                np.mean(fbetas_list, axis=0))

    def evaluate_model(self, eval_iterator):
        """One evaluation epoch; returns (mean accuracy, mean Hamming loss,
        mean per-class fbeta, pred_total, target_total) like
        biGRU_model.py:227-286."""
        self.eval()
        accuracies, hamm_losses, fbetas_list = [], [], []
        pred_total = torch.LongTensor()
        target_total = torch.LongTensor()

        with torch.no_grad():
            for input_seq, target in eval_iterator:
                target = target.squeeze(1)
                input_seq = input_seq.to(self.device)
                target = target.to(self.device)

                pred = self.forward(input_seq)
                pred = torch.sigmoid(pred) > 0.5

                acc, ham, fbeta = batch_metrics(target, pred, beta=0.5)
                accuracies.append(float(acc))
                hamm_losses.append(float(ham))
                fbetas_list.append(fbeta.cpu().numpy())

                pred_total = torch.cat(
                    [pred_total, pred.cpu().type(torch.LongTensor)], dim=0)
                target_total = torch.cat(
                    [target_total, target.cpu().type(torch.LongTensor)], dim=0)

        return (np.mean(accuracies), np.mean(hamm_losses),
                np.mean(fbetas_list, axis=0), pred_total, target_total)
