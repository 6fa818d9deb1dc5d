"""Host-side oracles shared by the GPU kernel tests.

Everything here runs on the CPU in exact integer or fp64 arithmetic and is
independent of the HIP kernels it judges: the counter hash is re-implemented
from its definition (splitmix64), the pooling argmax is an explicit
first-index scan, the recurrence is the textbook GRU cell.
"""
import numpy as np
import torch

MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------------------
# counter-based dropout
# ---------------------------------------------------------------------------

def mix64(x: int) -> int:
    """splitmix64 finalizer on Python ints (exact, mod 2^64)."""
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def mix64_np(x: np.ndarray) -> np.ndarray:
    """Vectorized mix64 on uint64 arrays (wrapping arithmetic)."""
    x = x.astype(np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def drop_params(p: float):
    """(thr, scale): 8-bit draw threshold from float(p), keep scale
    1/(1-p) evaluated in double and rounded once to fp32."""
    thr = int(np.float32(p) * np.float32(256.0))
    scale = np.float32(1.0 / (1.0 - float(p)))
    return thr, scale


def drop_mask(counter: np.ndarray, p: float, seed: int) -> np.ndarray:
    """True where the element whose counter is `counter` is DROPPED.
    `seed` is the int64 the binding receives (negative = top bit set)."""
    thr, _ = drop_params(p)
    c = counter.astype(np.uint64)
    r = mix64_np(np.uint64(seed & MASK64) ^ (c >> np.uint64(3)))
    byte = (r >> (np.uint64(8) * (c & np.uint64(7)))) & np.uint64(0xFF)
    return byte < np.uint64(thr)


def _apply_drop(x: torch.Tensor, dropped: np.ndarray, p: float):
    _, scale = drop_params(p)
    x = x.detach().cpu()
    assert x.dtype == torch.bfloat16
    kept = (x.float() * torch.tensor(float(scale), dtype=torch.float32))
    kept = kept.bfloat16()     # one fp32 product, RNE to bf16
    m = torch.from_numpy(dropped).reshape(x.shape)
    return torch.where(m, torch.zeros_like(kept), kept)


def dropout_ref(x: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    """Element dropout of a contiguous bf16 tensor: counter = flat index."""
    idx = np.arange(x.numel(), dtype=np.uint64)
    return _apply_drop(x, drop_mask(idx, p, seed), p)


def spatial_dropout_ref(x: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    """Channel dropout of (B, T, F) bf16: counter = b*F + f for every t."""
    B, T, F = x.shape
    c = (np.arange(B, dtype=np.uint64)[:, None, None] * np.uint64(F)
         + np.arange(F, dtype=np.uint64)[None, None, :])
    c = np.broadcast_to(c, (B, T, F))
    return _apply_drop(x, drop_mask(c, p, seed), p)


def all_positive_normal_bf16(lo_exp: int = -10, hi_exp: int = 10):
    """Every positive bf16 pattern in [2^lo_exp, 2^hi_exp): 128 mantissas
    per binade."""
    lo = (127 + lo_exp) << 7
    hi = (127 + hi_exp) << 7
    bits = torch.arange(lo, hi, dtype=torch.int32).to(torch.int16)
    return bits.view(torch.bfloat16)


# ---------------------------------------------------------------------------
# direction-sum + temporal pooling
# ---------------------------------------------------------------------------

def pool_ref(out: torch.Tensor, n_dir: int):
    """out: (B, T, n_dir*H) CPU tensor (bf16 or fp32).

    Returns dict with
      s32   (B,T,H) fp32  direction sum formed once in fp32 (what the kernels
                          compare and store for the max)
      maxv  (B,H)   fp32  max over T of s32
      amax  (B,H)   int32 FIRST t attaining the max (explicit scan)
      avg   (B,H)   fp64  sum_t(fp64 direction sum) / T
      abssum(B,H)   fp64  sum_t |fp64 direction sum|
      max64 (B,H)   fp64  max over T of the fp64 direction sum
      absdir(B,T,H) fp64  sum over directions of |input|
    """
    out = out.detach().cpu()
    B, T, HD = out.shape
    H = HD // n_dir
    parts = [out[:, :, d * H:(d + 1) * H] for d in range(n_dir)]
    s32 = parts[0].float()
    s64 = parts[0].double()
    absdir = parts[0].double().abs()
    for q in parts[1:]:
        s32 = s32 + q.float()
        s64 = s64 + q.double()
        absdir = absdir + q.double().abs()
    maxv = s32.max(dim=1).values
    t_idx = torch.arange(T, dtype=torch.int64)[None, :, None].expand(B, T, H)
    cand = torch.where(s32 == maxv[:, None, :], t_idx,
                       torch.full_like(t_idx, T))
    amax = cand.min(dim=1).values.to(torch.int32)
    assert int(amax.max()) < T
    return {"s32": s32, "maxv": maxv, "amax": amax,
            "max64": s64.max(dim=1).values, "absdir": absdir,
            "avg": s64.sum(dim=1) / T, "abssum": s64.abs().sum(dim=1)}


def pool_bwd_ref(dmax, davg, amax, T, n_dir):
    """fp64 d_out (B, T, n_dir*H): davg/T everywhere, + dmax at t == amax,
    the same gradient for every direction."""
    dmax = dmax.detach().cpu().double()
    davg = davg.detach().cpu().double()
    amax = amax.detach().cpu().long()
    B, H = dmax.shape
    t_idx = torch.arange(T)[None, :, None]
    g = (davg / T)[:, None, :] + torch.where(
        t_idx == amax[:, None, :], dmax[:, None, :],
        torch.zeros((), dtype=torch.float64))
    return torch.cat([g] * n_dir, dim=-1)


def fp32_ulp(ref: torch.Tensor) -> torch.Tensor:
    """Spacing of fp32 numbers at |ref| (ref rounded to fp32), as fp64."""
    a = ref.detach().cpu().abs().to(torch.float32).numpy()
    return torch.from_numpy(np.spacing(a).astype(np.float64))


# ---------------------------------------------------------------------------
# golden GRU recurrence on precomputed input projections (autograd-capable;
# runs in the dtype/device of its arguments)
# ---------------------------------------------------------------------------

def gru_ref_from_gi(gi, w, bhh, h0=None):
    B, T, _ = gi.shape
    n_dir, threeH, H = w.shape
    outs, hlast = [], []
    for d in range(n_dir):
        h = (h0[d] if h0 is not None
             else torch.zeros(B, H, device=gi.device, dtype=gi.dtype))
        hs = [None] * T
        steps = range(T - 1, -1, -1) if d == 1 else range(T)
        for t in steps:
            g = gi[:, t, d * threeH:(d + 1) * threeH]
            gh = h @ w[d].t() + bhh[d]
            i_r, i_z, i_n = g.chunk(3, -1)
            h_r, h_z, h_n = gh.chunk(3, -1)
            r = torch.sigmoid(i_r + h_r)
            z = torch.sigmoid(i_z + h_z)
            n = torch.tanh(i_n + r * h_n)
            h = (1 - z) * n + z * h
            hs[t] = h
        outs.append(torch.stack(hs, 1))
        hlast.append(h)
    return torch.cat(outs, -1), torch.stack(hlast, 0)
