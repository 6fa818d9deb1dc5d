"""A training step is bitwise reproducible on the GPU: the same weights,
batch and dropout seed give the same loss, logits, gradients and updated
parameters every time. Cross-block sums (bias grads, loss, grad norm) go
through per-block partials summed in a fixed order, never float atomics.

Shapes: more than one batch tile with a ragged last tile, on each backward
kernel family — fp32 H=32 (generic), bf16 H=128 (hot path), bf16 H=512 with
two 256-row batch groups (column-split)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _step(model0, x, y, wgt, pw):
    from fmda_amd.ops.interface import fused_head_loss
    from fmda_amd.optim import FusedClipAdam
    model = copy.deepcopy(model0)
    model.train()
    # clip far below the gradient norm, so the norm reduction decides the
    # update of every parameter
    opt = FusedClipAdam(model.parameters(), lr=1e-3, clip=1e-3)
    torch.manual_seed(11)  # dropout seeds
    feats = model.forward_features(x)
    loss, logits = fused_head_loss(feats, model.linear.weight,
                                   model.linear.bias, y, wgt, pw)
    loss.backward()
    grads = [p.grad.clone() for p in model.parameters()]
    opt.step()
    torch.cuda.synchronize()
    return ([loss.detach(), logits.detach()] + grads
            + [p.detach() for p in model.parameters()] + [opt.last_norm2])


@pytest.mark.parametrize("H,L,T,B,dtype", [
    (32, 1, 9, 70, torch.float32),
    (128, 2, 12, 70, torch.bfloat16),
    (512, 1, 4, 300, torch.bfloat16),
])
def test_train_step_bitwise_reproducible(H, L, T, B, dtype):
    from fmda_amd.models import BiGRU
    torch.manual_seed(3)
    model = BiGRU(H, 24, 4, n_layers=L, spatial_dropout=False,
                  dropout=0.5).cuda()
    g = torch.Generator().manual_seed(4)
    x = torch.rand(B, T, 24, generator=g).to("cuda", dtype)
    y = (torch.rand(B, 4, generator=g) < 0.25).float().cuda()
    wgt = torch.tensor([4.0, 6.0, 4.0, 6.0], device="cuda")
    pw = torch.tensor([3.0, 5.0, 3.0, 5.0], device="cuda")
    ref = _step(model, x, y, wgt, pw)
    assert all(torch.isfinite(t.float()).all() for t in ref)
    assert float(ref[-1]) > 1e-6  # clipping engaged (norm >> clip)
    for _ in range(3):
        cur = _step(model, x, y, wgt, pw)
        for i, (a, b) in enumerate(zip(ref, cur)):
            assert torch.equal(a, b), (i, (a.float() - b.float()).abs().max())
