"""CPU check of the cases of tests/test_gpu_bwd_step_int.py: for every shape,
p and seed used there the oracle mask holds dropped and kept elements, so no
GPU comparison passes because a mask happened to be constant. Also the
counter algebra the kernel relies on: one octet per 8 consecutive columns,
advancing by n_dir * H / 8 per time step."""
import numpy as np

import oracles as orc
import test_gpu_bwd_step_int as cases


def test_every_case_drops_and_keeps():
    seen = set()
    for D in cases.DIRS:
        for T in cases.STEPS:
            for B in cases.BATCHES:
                for p in cases.P_POW2 + cases.P_ANY:
                    seed = cases.seed_for(D, T, B, p)
                    seen.add(seed)
                    idx = np.arange(B * T * D * cases.H, dtype=np.uint64)
                    m = orc.drop_mask(idx, p, seed)
                    assert m.any() and not m.all(), (D, T, B, p, seed)
    assert seen == set(cases.SEEDS)
    assert sum(s < 0 for s in cases.SEEDS) >= 2


def test_octet_counter_algebra():
    """o >> 3 of element (b, t, d, j) equals the octet at t = 0 plus
    t * D * H / 8, and o & 7 equals j & 7: what the kernel's per-launch row
    base and per-step stride assume."""
    H = cases.H
    for D in cases.DIRS:
        T = 7
        b = np.arange(70, dtype=np.int64)[:, None, None, None]
        t = np.arange(T, dtype=np.int64)[None, :, None, None]
        d = np.arange(D, dtype=np.int64)[None, None, :, None]
        j = np.arange(H, dtype=np.int64)[None, None, None, :]
        o = ((b * T + t) * D * H) + d * H + j
        base = ((b * T * D * H) + d * H + j) >> 3
        assert np.array_equal(o >> 3, base + t * (D * H // 8))
        assert np.array_equal(o & 7, np.broadcast_to(j & 7, o.shape))
        flat = np.arange(70 * T * D * H, dtype=np.int64).reshape(o.shape)
        assert np.array_equal(o, flat)
