"""FusedClipAdam vs torch clip_grad_norm_ + Adam (same math)."""
import pytest
import torch
import torch.nn as nn

from fmda_amd.optim import FusedClipAdam


def _models(device="cpu"):
    torch.manual_seed(0)
    m1 = nn.Sequential(nn.Linear(13, 7), nn.Tanh(), nn.Linear(7, 3)).to(device)
    m2 = nn.Sequential(nn.Linear(13, 7), nn.Tanh(), nn.Linear(7, 3)).to(device)
    m2.load_state_dict(m1.state_dict())
    return m1, m2


def _run_pair(device, clip, steps=5, tol=1e-6):
    m1, m2 = _models(device)
    o1 = FusedClipAdam(m1.parameters(), lr=1e-2, clip=clip)
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-2)
    g = torch.Generator().manual_seed(3)
    for i in range(steps):
        x = torch.randn(32, 13, generator=g).to(device)
        y = torch.randn(32, 3, generator=g).to(device)
        for m, o in ((m1, o1), (m2, o2)):
            o.zero_grad()
            loss = ((m(x) - y) ** 2).mean() * 40  # large grads -> clip active
            loss.backward()
            if o is o2 and clip > 0:
                nn.utils.clip_grad_norm_(m2.parameters(), clip)
            o.step()
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.allclose(p1, p2, atol=tol), (p1 - p2).abs().max()


def test_eager_fallback_matches_torch_with_clip():
    _run_pair("cpu", clip=0.05)


def test_eager_fallback_matches_torch_no_clip():
    _run_pair("cpu", clip=0.0)


@pytest.mark.gpu
def test_fused_kernel_matches_torch_with_clip():
    _run_pair("cuda", clip=0.05, tol=1e-5)


@pytest.mark.gpu
def test_fused_kernel_matches_torch_no_clip():
    _run_pair("cuda", clip=0.0, tol=1e-5)


# ---------------------------------------------------------------------------
# Chunk edges, the launch-grid cap, last_norm2, grad-pointer re-patching and
# the state round trip, against clip_grad_norm_ + torch.optim.Adam on fp64
# CPU copies.
# ---------------------------------------------------------------------------

_CHUNK_EDGE_SIZES = [1, 4095, 4096, 4097, 3 * 4096 + 5]


def _params_and_grads(sizes, steps, gscale, seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g) for n in sizes]
    gs = [[torch.randn(n, generator=g) * gscale for n in sizes]
          for _ in range(steps)]
    return ps, gs


def _fp64_reference(ps, gs, lr, clip):
    """Parameters after len(gs) steps, and the squared global grad norm
    (before clipping) of every step, all in fp64."""
    ref = [torch.nn.Parameter(p.double().clone()) for p in ps]
    opt = torch.optim.Adam(ref, lr=lr)
    norm2 = []
    for step_g in gs:
        for p, gr in zip(ref, step_g):
            p.grad = gr.double().clone()
        norm2.append(sum(float((gr.double() ** 2).sum()) for gr in step_g))
        if clip > 0:
            nn.utils.clip_grad_norm_(ref, clip)
        opt.step()
    return [p.detach() for p in ref], norm2


def _check_against_reference(opt, params, ref, norm2_got, norm2_ref, clip):
    for p, r in zip(params, ref):
        err = (p.detach().double().cpu() - r).abs().max()
        assert err <= 1e-5, (p.numel(), float(err))
    if clip > 0:
        # all terms non-negative; the per-thread serial, wave, block and
        # partial sums add fewer than 100 roundings of 2^-24 each (6e-6),
        # so rtol 1e-5 carries about 2x margin
        for got, want in zip(norm2_got, norm2_ref):
            assert abs(got - want) <= 1e-5 * want, (got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("fresh_grads", [True, False],
                         ids=["fresh_grad_tensors", "reused_grad_tensors"])
@pytest.mark.parametrize("clip,gscale", [(0.05, 1.0), (50.0, 1e-3)],
                         ids=["clip_active", "clip_inactive"])
def test_fused_adam_chunk_edges(clip, gscale, fresh_grads):
    """One optimizer over parameters of 1, 4095, 4096, 4097 and 3*4096+5
    elements (1..4 chunks, ragged last chunks). fresh_grads assigns new grad
    tensors after zero_grad(set_to_none=True) every step (pointer re-patch +
    double-buffered staging); otherwise the same grad tensors are refilled
    in place and the table is patched once."""
    steps, lr = 3, 1e-2
    ps, gs = _params_and_grads(_CHUNK_EDGE_SIZES, steps, gscale)
    ref, norm2_ref = _fp64_reference(ps, gs, lr, clip)
    if clip == 50.0:
        assert max(norm2_ref) ** 0.5 < clip      # really inactive

    params = [torch.nn.Parameter(p.clone().cuda()) for p in ps]
    opt = FusedClipAdam(params, lr=lr, clip=clip)
    norm2_got, keep = [], []
    for step_g in gs:
        if fresh_grads:
            opt.zero_grad(set_to_none=True)
            for p, gr in zip(params, step_g):
                p.grad = gr.cuda()
            keep.append([p.grad for p in params])  # no address reuse
        else:
            for p, gr in zip(params, step_g):
                if p.grad is None:
                    p.grad = torch.empty_like(p)
                p.grad.copy_(gr)
        ptrs_before = opt._ptrs
        opt.step()
        if not fresh_grads and ptrs_before is not None:
            assert opt._ptrs == ptrs_before
        norm2_got.append(float(opt.last_norm2))
    _check_against_reference(opt, params, ref, norm2_got, norm2_ref, clip)


@pytest.mark.gpu
def test_fused_adam_grid_stride_over_2048_chunks():
    """2049*4096+7 elements = 2050 chunks > the 2048-block grid cap: blocks
    0 and 1 take a second chunk in both kernels."""
    n, lr, clip = 2049 * 4096 + 7, 1e-2, 0.05
    ps, gs = _params_and_grads([n], 1, 1.0, seed=1)
    ref, norm2_ref = _fp64_reference(ps, gs, lr, clip)
    p = torch.nn.Parameter(ps[0].clone().cuda())
    opt = FusedClipAdam([p], lr=lr, clip=clip)
    p.grad = gs[0][0].cuda()
    opt.step()
    assert opt._chunks.shape[0] == 2050
    _check_against_reference(opt, [p], ref, [float(opt.last_norm2)],
                             norm2_ref, clip)


@pytest.mark.gpu
def test_fused_adam_state_dict_round_trip_bitwise():
    """2 steps, state_dict -> load_state_dict into a new optimizer, 1 more
    step: bitwise equal to 3 uninterrupted steps."""
    lr, clip = 1e-2, 0.05
    ps, gs = _params_and_grads(_CHUNK_EDGE_SIZES, 3, 1.0, seed=2)

    def run(interrupt):
        params = [torch.nn.Parameter(p.clone().cuda()) for p in ps]
        opt = FusedClipAdam(params, lr=lr, clip=clip)
        for i, step_g in enumerate(gs):
            if interrupt and i == 2:
                sd = {k: ([t.clone() for t in v] if isinstance(v, list)
                          else v) for k, v in opt.state_dict().items()}
                opt = FusedClipAdam(params, lr=lr, clip=clip)
                opt.load_state_dict(sd)
            opt.zero_grad(set_to_none=True)
            for p, gr in zip(params, step_g):
                p.grad = gr.cuda()
            opt.step()
        return [p.detach().clone() for p in params]

    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)
