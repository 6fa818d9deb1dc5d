"""CPU self-tests of the host oracles in tests/oracles.py (no GPU)."""
import numpy as np
import torch

import oracles as orc


def test_mix64_known_answers():
    assert orc.mix64(0) == 0xE220A8397B1DCDAF
    assert orc.mix64(1) == 0x910A2DEC89025CC1


def test_mix64_numpy_matches_python_ints():
    xs = [0, 1, 2, 0xFFFFFFFFFFFFFFFF, 1 << 63, 0x9E3779B97F4A7C15,
          123456789012345678]
    got = orc.mix64_np(np.array(xs, dtype=np.uint64))
    assert [int(g) for g in got] == [orc.mix64(x) for x in xs]


def test_drop_params_double_scale():
    thr, scale = orc.drop_params(0.6)
    assert thr == 153 and float(scale) == 2.5
    # the float expression the launchers used to evaluate is one ulp off
    assert float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.6))) != 2.5
    assert orc.drop_params(0.3)[0] == 76
    assert float(orc.drop_params(0.8)[1]) == 5.0
    assert orc.drop_params(0.5) == (128, np.float32(2.0))


def test_dropout_ref_rounding_tie_example():
    """bf16 130/128 times 2.5 is an exact rounding tie: RNE keeps the even
    pattern 16418 (the one-ulp-high float scale would give 16419)."""
    x = torch.tensor([130.0 / 128.0], dtype=torch.bfloat16)
    # pick a seed under which element 0 is kept
    seed = next(s for s in range(100)
                if not orc.drop_mask(np.array([0]), 0.6, s)[0])
    y = orc.dropout_ref(x, 0.6, seed)
    assert int(y.view(torch.int16)[0]) == 16418


def test_dropout_ref_mask_definition_and_negative_seed():
    p, seed = 0.3, -(1 << 62) - 12345          # top bit set as uint64
    x = torch.ones(37, dtype=torch.bfloat16)
    y = orc.dropout_ref(x, p, seed)
    thr, scale = orc.drop_params(p)
    for i in range(37):
        r = orc.mix64((seed & orc.MASK64) ^ (i >> 3))
        dropped = ((r >> (8 * (i & 7))) & 0xFF) < thr
        want = 0.0 if dropped else float(
            torch.tensor(float(scale)).bfloat16())
        assert float(y[i]) == want, i


def test_dropout_ref_keep_rate():
    x = torch.ones(1 << 16, dtype=torch.bfloat16)
    for p in (0.3, 0.6, 0.8):
        kept = (orc.dropout_ref(x, p, 99) != 0).float().mean().item()
        thr, _ = orc.drop_params(p)
        assert abs(kept - (1 - thr / 256.0)) < 0.01


def test_spatial_dropout_ref_shares_mask_over_time():
    x = torch.ones(3, 7, 5, dtype=torch.bfloat16)
    y = orc.spatial_dropout_ref(x, 0.6, 7)
    assert (y == y[:, :1, :]).all()
    # channel (b, f) draws byte (b*F+f)&7 of octet (b*F+f)>>3
    m = orc.drop_mask(np.arange(15), 0.6, 7).reshape(3, 5)
    assert ((y[:, 0, :] == 0).numpy() == m).all()


def test_all_positive_normal_bf16_range():
    v = orc.all_positive_normal_bf16()
    assert v.numel() == 2560
    assert float(v[0]) == 2.0 ** -10 and float(v[-1]) < 2.0 ** 10
    assert float(v[-1]) == 2.0 ** 10 * (1 - 2.0 ** -8)


def test_pool_ref_first_index_tie_and_values():
    out = torch.tensor([[[1.0, 0.5, -1.0, 0.0],
                         [0.5, 1.0, -0.5, 0.5],
                         [1.0, 1.0, -1.0, 0.0]]])      # B=1, T=3, 2*H=4
    r = orc.pool_ref(out, 2)
    # direction sums: t0 [0.0, 0.5], t1 [0.0, 1.5], t2 [0.0, 1.0]
    assert r["maxv"].tolist() == [[0.0, 1.5]]
    assert r["amax"].tolist() == [[0, 1]]              # tie -> smallest t
    assert r["avg"].tolist() == [[0.0, 1.0]]
    r1 = orc.pool_ref(out, 1)
    assert r1["amax"].tolist() == [[0, 1, 1, 1]]
    g = orc.pool_bwd_ref(torch.tensor([[2.0, 3.0]]),
                         torch.tensor([[3.0, 6.0]]), r["amax"], 3, 2)
    assert g.shape == (1, 3, 4)
    assert g[0, :, 0].tolist() == [3.0, 1.0, 1.0]
    assert g[0, :, 3].tolist() == [2.0, 5.0, 2.0]


def test_gru_ref_matches_torch_gru_cell():
    torch.manual_seed(0)
    B, T, H = 3, 4, 5
    cell = torch.nn.GRUCell(H, H).double()
    gi = torch.randn(B, T, 3 * H, dtype=torch.float64)
    w = cell.weight_hh.detach()[None]
    bhh = cell.bias_hh.detach()[None]
    out, hl = orc.gru_ref_from_gi(gi, w, bhh)
    h = torch.zeros(B, H, dtype=torch.float64)
    eye = torch.eye(3 * H, dtype=torch.float64)
    for t in range(T):
        # feed gi through an identity input projection
        h = torch._VF.gru_cell(gi[:, t], h, eye, cell.weight_hh, None,
                               cell.bias_hh)
        assert torch.allclose(out[:, t], h, atol=1e-12)
    assert torch.allclose(hl[0], h, atol=1e-12)
