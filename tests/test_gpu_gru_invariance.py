"""Exact (bitwise) row-independence and direction symmetry of the recurrence
kernels.

Batch rows are independent in the math, and in every kernel the order in
which an output element is accumulated depends only on its own row (the
MFMA / dot-product K order, the time loop). So each per-row output must be
bit-identical wherever the row sits in the batch: first or last tile, full
or partial tile, either side of a 256-row group. A tolerance test cannot
see an error confined to one row of a partial tile, or one leaked through
the dead-row clamp of the LDS staging; `torch.equal` can.

Comparisons stay within one kernel variant (same dtype, H, h0-or-not) and
B >= 2, so the batch-1 kernel is never one side of a comparison.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

# dtype, H, B, T
VARIANTS = [
    ("bf16", 128, 37, 5),    # v3
    ("bf16", 32, 37, 5),     # W resident in LDS
    ("bf16", 256, 37, 5),    # streamed W
    ("bf16", 512, 37, 5),    # column-split (no h0) / batch-parallel (h0)
    ("bf16", 512, 261, 3),   # crosses a 256-row batch group
    ("fp32", 16, 37, 5),
]
IDS = [f"{d}-H{h}-B{b}" for d, h, b, _ in VARIANTS]


def _ext():
    from fmda_amd.ops import load_extension
    return load_extension()


def _inputs(dtype, H, B, T, use_h0, seed=71):
    n_dir = 2
    g = torch.Generator().manual_seed(seed)
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    d = {
        "gi": (torch.randn(B, T, n_dir * 3 * H, generator=g) * 0.5).to(td),
        "w": (torch.randn(n_dir, 3 * H, H, generator=g) * 0.1).to(td),
        "bhh": torch.randn(n_dir, 3 * H, generator=g) * 0.1,
        "h0": (torch.randn(n_dir, B, H, generator=g) * 0.5
               if use_h0 else None),
        "dout": torch.randn(B, T, n_dir * H, generator=g).to(td),
        "dhT": torch.randn(n_dir, B, H, generator=g),
    }
    return {k: (v.cuda() if v is not None else None) for k, v in d.items()}


def _fwd(d, idx):
    h0 = d["h0"][:, idx].contiguous() if d["h0"] is not None else None
    out, hlast = _ext().gru_fwd(d["gi"][idx].contiguous(), d["w"], d["bhh"],
                                h0)[:2]
    return out, hlast


def _bwd(d, idx, out_rows):
    h0 = d["h0"][:, idx].contiguous() if d["h0"] is not None else None
    res = _ext().gru_bwd(d["gi"][idx].contiguous(), d["w"], d["bhh"],
                         out_rows.contiguous(), d["dout"][idx].contiguous(),
                         d["dhT"][:, idx].contiguous(), 0.0, 0, h0)
    return res[0], res[2]        # dgi, dh0


def _row_orders(B):
    ident = torch.arange(B, device="cuda")
    rev = torch.arange(B - 1, -1, -1, device="cuda")
    # the last 5 rows, then the first 2: a 7-row batch (B=37: rows
    # 32..36 of the partial second tile followed by rows 0, 1)
    sub = torch.cat([ident[B - 5:], ident[:2]])
    return ident, rev, sub


@pytest.mark.parametrize("use_h0", [False, True], ids=["zero_h0", "h0"])
@pytest.mark.parametrize("dtype,H,B,T", VARIANTS, ids=IDS)
def test_gru_rows_bitwise_independent_of_batch_position(dtype, H, B, T,
                                                        use_h0):
    d = _inputs(dtype, H, B, T, use_h0)
    ident, rev, sub = _row_orders(B)
    out_a, hl_a = _fwd(d, ident)
    dgi_a, dh0_a = _bwd(d, ident, out_a)
    assert torch.isfinite(out_a.float()).all()
    assert torch.isfinite(dgi_a.float()).all() and torch.isfinite(dh0_a).all()
    for name, idx in (("reversed", rev), ("sub-batch", sub)):
        out_x, hl_x = _fwd(d, idx)
        # out_x[i] is row idx[i] of the full batch
        assert torch.equal(out_x, out_a[idx]), (name, "out")
        assert torch.equal(hl_x, hl_a[:, idx]), (name, "hlast")
        dgi_x, dh0_x = _bwd(d, idx, out_a[idx])
        assert torch.equal(dgi_x, dgi_a[idx]), (name, "dgi")
        assert torch.equal(dh0_x, dh0_a[:, idx]), (name, "dh0")


@pytest.mark.parametrize("use_h0", [False, True], ids=["zero_h0", "h0"])
@pytest.mark.parametrize("dtype,H,B,T", VARIANTS, ids=IDS)
def test_gru_direction_symmetry_bitwise(dtype, H, B, T, use_h0):
    """Swap the two directions' gi blocks, w, bhh (and h0) and flip the
    inputs along T: direction 1 then runs exactly the sequence direction 0
    ran before, so its output is the time-flip of the other's."""
    d = _inputs(dtype, H, B, T, use_h0, seed=72)
    ident = torch.arange(B, device="cuda")
    out, hl = _fwd(d, ident)
    G = 3 * H
    sw = dict(d)
    sw["gi"] = torch.cat([d["gi"][..., G:], d["gi"][..., :G]],
                         dim=-1).flip(1).contiguous()
    sw["w"] = d["w"].flip(0).contiguous()
    sw["bhh"] = d["bhh"].flip(0).contiguous()
    if use_h0:
        sw["h0"] = d["h0"].flip(0).contiguous()
    out_s, hl_s = _fwd(sw, ident)
    assert torch.equal(out_s[..., H:], out[..., :H].flip(1))
    assert torch.equal(out_s[..., :H], out[..., H:].flip(1))
    assert torch.equal(hl_s, hl.flip(0))
