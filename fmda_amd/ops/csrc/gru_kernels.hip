// Persistent biGRU recurrence kernels for MI355X (gfx950, CDNA4).
//
// Design (MI355X-first, not a port of the reference's cuDNN RNN call at
// biGRU_model.py:102):
// - The time-batched input projections gi = x @ W_ih^T + b_ih for BOTH
//   directions are computed outside (one rocBLAS MFMA GEMM); these kernels
//   own the sequential part: per timestep the recurrent GEMM
//   gh = h_{t-1} @ W_hh^T on MFMA (v_mfma_f32_16x16x32_bf16), the gate
//   sigmoid/tanh fusion, and the hidden-state update.
// - One workgroup owns a tile of batch rows for one direction for the whole
//   sequence: batch rows are independent, so there is no inter-workgroup
//   communication and no grid sync. Both directions launch in one grid
//   (blockIdx.y = direction).
// - Recurrent-weight residency by size: the generic kernels keep W_hh in LDS
//   at small sizes (WLDS) and stream it from the per-XCD L2 at H >= 256. The
//   hot config (bf16 H = 128) runs the v3 kernels below, which hoist the
//   MFMA B-fragments of W_hh INTO REGISTERS once for all T timesteps
//   (~0.4-0.8 KB/lane) - zero W traffic in the loop.
// - Each kernel's dynamic LDS layout is one constexpr struct (byte offset of
//   every region and the total `bytes`): the kernel forms its pointers from
//   it and the launcher sizes the launch from it.
// - The next timestep's tiles are PREFETCHED into registers during the MFMA
//   phase and committed to LDS after the barrier (async-STAGE split,
//   cdna_hip_programming.md T14), so HBM latency hides under compute.
// - LDS rows are padded to an odd 16-byte-slot pitch: fragment reads touch
//   16 distinct rows at one 16-B column slot, which at a power-of-two pitch
//   is a 16-way bank conflict and at the padded pitch is conflict-free.
// - The backward (BPTT) kernel recomputes the gates from gi + a fresh
//   recurrent GEMM on the stored h (cheaper than materializing activations:
//   the op is HBM-bound), producing dGi (consumed by torch autograd for
//   dW_ih/db_ih/dx) and dGh. dGh is stored TIME-SHIFTED so that slot t holds
//   the gate grads whose h_prev is out[t]: dW_hh then reduces with a single
//   contiguous rocBLAS GEMM (dgh^T @ out), no sliced copies. db_hh is
//   accumulated in-kernel (registers across T, one store per column into the
//   block's own row of a partials table, summed in a fixed order afterwards).
// - fp32 instantiations use a plain VALU dot-product path with the same
//   phase structure and C-tile ownership; they are the on-GPU numerics
//   oracle, validated against the PyTorch fp32 reference.
//
// Gate math follows the PyTorch packed (r, z, n) convention
// (reference biGRU_model.py:54-56 uses nn.GRU):
//   r = sigmoid(i_r + W_hr h + b_hr)
//   z = sigmoid(i_z + W_hz h + b_hz)
//   n = tanh(i_n + r * (W_hn h + b_hn))
//   h' = (1 - z) * n + z * h
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdint>
#include <type_traits>

#include "dropout_common.h"   // mix64, drop_hit, drop_apply
#include "fmda_launch.h"

#define FMDA_DEV __device__ __forceinline__

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

namespace fmda {

// The dynamic LDS of one CU; every layout struct asserts its total against it.
constexpr int LDS_CU_BYTES = 160 * 1024;

// Tile constants that fmda_gru_bwd_db_rows shares with the launchers that own
// them: the v3 backward's batch tile, and the column-split kernels' batch
// rows and block size.
constexpr int BWD_V3_BT = 32;
constexpr int CS_BR = 256;
constexpr int CS_NT = 512;

// Gate activations on the raw hardware transcendentals (v_exp_f32 computes
// exp2; v_rcp_f32 is the fast reciprocal) — the libm expf/tanhf expansions
// cost ~30 VALU instructions each (range reduction + precise division +
// special-case cmp/cndmask chains) and dominated the per-timestep latency
// of the recurrence loop. |rel err| ~1e-7, far inside the test tolerances.
#define FMDA_LOG2E 1.4426950408889634f

FMDA_DEV float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
FMDA_DEV float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

FMDA_DEV float sigmoidf(float x) {
    // exp2 underflows to 0 for x << 0 and overflows to +inf for x >> 0;
    // rcp(1+inf)=0 and rcp(1+0)=1 give the right saturations, no clamps.
    return fast_rcp(1.0f + fast_exp2(-x * FMDA_LOG2E));
}

FMDA_DEV float fast_tanh(float x) {
    // tanh(x) = 1 - 2/(1+exp2(2x*log2e)); saturates correctly at +/-inf.
    return 1.0f - 2.0f * fast_rcp(1.0f + fast_exp2(2.0f * FMDA_LOG2E * x));
}

template <typename T> FMDA_DEV float to_f32(T v);
template <> FMDA_DEV float to_f32<float>(float v) { return v; }
template <> FMDA_DEV float to_f32<__hip_bfloat16>(__hip_bfloat16 v) {
    return __bfloat162float(v);
}
template <typename T> FMDA_DEV T from_f32(float v);
template <> FMDA_DEV float from_f32<float>(float v) { return v; }
template <> FMDA_DEV __hip_bfloat16 from_f32<__hip_bfloat16>(float v) {
    return __float2bfloat16(v);
}

struct alignas(16) chunk16 { unsigned int u[4]; };

// ---------------------------------------------------------------------------
// Cooperative tile copy helpers (NT threads), vectorized by 16-byte chunks.
// Global rows may be masked by `rows_valid`: out-of-range rows are skipped -
// their LDS content is garbage but never observed (batch rows independent).
// ---------------------------------------------------------------------------

template <typename T, int ROWS, int NT>
FMDA_DEV void stage_tile(T* __restrict__ lds, const T* __restrict__ gp,
                         int cols, int lds_pitch, long row_stride,
                         int rows_valid, int tid) {
    const int cpr = (cols * (int)sizeof(T)) / 16;
    for (int c = tid; c < ROWS * cpr; c += NT) {
        const int r = c / cpr;
        const int jc = c % cpr;
        if (r < rows_valid)
            ((chunk16*)((char*)lds + (long)r * lds_pitch * sizeof(T)))[jc] =
                ((const chunk16*)((const char*)gp +
                                  (long)r * row_stride * sizeof(T)))[jc];
    }
}

template <typename T, int ROWS, int NT>
FMDA_DEV void store_tile(const T* __restrict__ lds, T* __restrict__ gp,
                         int cols, int lds_pitch, long row_stride,
                         int rows_valid, int tid) {
    const int cpr = (cols * (int)sizeof(T)) / 16;
    for (int c = tid; c < ROWS * cpr; c += NT) {
        const int r = c / cpr;
        const int jc = c % cpr;
        if (r < rows_valid)
            ((chunk16*)((char*)gp + (long)r * row_stride * sizeof(T)))[jc] =
                ((const chunk16*)((const char*)lds +
                                  (long)r * lds_pitch * sizeof(T)))[jc];
    }
}

template <typename T, int ROWS, int NT>
FMDA_DEV void store_zero_tile(T* __restrict__ gp, int cols, long row_stride,
                              int rows_valid, int tid) {
    const int cpr = (cols * (int)sizeof(T)) / 16;
    const chunk16 z = {};
    for (int c = tid; c < ROWS * cpr; c += NT) {
        const int r = c / cpr;
        const int jc = c % cpr;
        if (r < rows_valid)
            ((chunk16*)((char*)gp + (long)r * row_stride * sizeof(T)))[jc] = z;
    }
}

template <typename T, int ROWS, int NT>
FMDA_DEV void zero_tile(T* __restrict__ lds, int lds_pitch, int tid) {
    for (int c = tid; c < ROWS * lds_pitch; c += NT)
        lds[c] = from_f32<T>(0.0f);
}

// Initial hidden state h0 (fp32, contiguous (rows, cols)) -> LDS tile of
// dtype T at `lds_pitch`; dead rows and pad columns are zeroed (nn.GRU h0
// support, reference biGRU_model.py:102 `self.gru(input_seq, hidden)`).
template <typename T, int ROWS, int NT>
FMDA_DEV void stage_h0_tile(T* __restrict__ lds, const float* __restrict__ h0,
                            int cols, int lds_pitch, int rows_valid, int tid) {
    for (int c = tid; c < ROWS * lds_pitch; c += NT) {
        const int r = c / lds_pitch;
        const int j = c % lds_pitch;
        const float v = (r < rows_valid && j < cols)
                            ? h0[(long)r * cols + j] : 0.0f;
        lds[c] = from_f32<T>(v);
    }
}

// fp32 LDS tile += T-typed global tile (dh += dOut[t]); synchronous form.
template <typename T, int ROWS, int NT>
FMDA_DEV void accum_tile_f32(float* __restrict__ lds, const T* __restrict__ gp,
                             int cols, int lds_pitch, long row_stride,
                             int rows_valid, int tid) {
    for (int c = tid; c < ROWS * cols; c += NT) {
        const int r = c / cols;
        const int j = c % cols;
        if (r < rows_valid)
            lds[r * lds_pitch + j] += to_f32<T>(gp[(long)r * row_stride + j]);
    }
}

// Register prefetch of a tile (async-STAGE split): issue loads in one phase,
// commit to LDS (or accumulate into an fp32 LDS tile) in a later phase.
// PC = max 16-byte chunks per thread.
template <typename T, int ROWS, int NT, int PC>
struct TilePrefetch {
    chunk16 v[PC];
    FMDA_DEV void issue(const T* __restrict__ gp, int cols, long row_stride,
                        int rows_valid, int tid) {
        const int cpr = (cols * (int)sizeof(T)) / 16;
#pragma unroll
        for (int i = 0; i < PC; ++i) {
            const int c = tid + i * NT;
            if (c < ROWS * cpr) {
                const int r = c / cpr;
                const int jc = c % cpr;
                if (r < rows_valid)
                    v[i] = ((const chunk16*)((const char*)gp +
                              (long)r * row_stride * sizeof(T)))[jc];
            }
        }
    }
    FMDA_DEV void commit(T* __restrict__ lds, int cols, int lds_pitch,
                         int tid) {
        const int cpr = (cols * (int)sizeof(T)) / 16;
#pragma unroll
        for (int i = 0; i < PC; ++i) {
            const int c = tid + i * NT;
            if (c < ROWS * cpr) {
                const int r = c / cpr;
                const int jc = c % cpr;
                ((chunk16*)((char*)lds + (long)r * lds_pitch * sizeof(T)))[jc]
                    = v[i];
            }
        }
    }
    // lds_f32[r][j] += (float)value for every element of the tile
    FMDA_DEV void commit_accum_f32(float* __restrict__ lds, int cols,
                                   int lds_pitch, int rows_valid, int tid) {
        constexpr int EPC = 16 / (int)sizeof(T);  // elements per chunk
        const int cpr = cols / EPC;
#pragma unroll
        for (int i = 0; i < PC; ++i) {
            const int c = tid + i * NT;
            if (c < ROWS * cpr) {
                const int r = c / cpr;
                const int jc = c % cpr;
                if (r < rows_valid) {
                    const T* e = (const T*)&v[i];
#pragma unroll
                    for (int k = 0; k < EPC; ++k)
                        lds[r * lds_pitch + jc * EPC + k] += to_f32<T>(e[k]);
                }
            }
        }
    }
};

// ---------------------------------------------------------------------------
// MFMA fragment layout (v_mfma_f32_16x16x32_bf16; ck_tile
// warp_gemm_attribute_mfma_impl.hpp M16N16K32 constants; verified on GPU by
// mfma_selftest):
//   A (M=16, K=32): lane l holds A[l%16][8*(l/16) + e], e = 0..7 contiguous
//   B (K=32, N=16): lane l holds B[8*(l/16) + e][l%16]
//   C (16x16):      lane l, reg v holds C[4*(l/16) + v][l%16]
// The fp32 path computes the same owned C elements with plain dots so the
// fused gate phase is identical for both dtypes.
// ---------------------------------------------------------------------------

// B-fragment of W for the gh GEMM (N = gate output column, K = h index).
template <int Hp>
FMDA_DEV bf16x8_t load_wfragA(const __hip_bfloat16* __restrict__ w, long pitch,
                              int ct, int g, int kk, int lane) {
    const long n = (long)g * Hp + ct * 16 + (lane & 15);
    const int kbase = 32 * kk + 8 * (lane >> 4);
    return *(const bf16x8_t*)((const __bf16*)w + n * pitch + kbase);
}

// B-fragment of W for the dh GEMM (K = gate row n, N = h column):
// element B[n][j] = W[n][j]; per lane 8 rows n at fixed column j.
template <int Hp>
FMDA_DEV bf16x8_t load_wfragB(const __hip_bfloat16* __restrict__ w, long pitch,
                              int ct, int kk, int lane) {
    const int jcol = ct * 16 + (lane & 15);
    const int nbase = 32 * kk + 8 * (lane >> 4);
    bf16x8_t b;
    const __bf16* wb = (const __bf16*)w;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        b[e] = wb[(long)(nbase + e) * pitch + jcol];
    return b;
}

// Dynamic LDS of gru_fwd_kernel (byte offsets) and the padded pitches
// (elements) of its tiles: W slice (WLDS only), fp32 h, bf16 h copy for the
// MFMA A-fragments (bf16 only), gi tile, b_hh.
template <typename T, int BT, int Hp, bool WLDS>
struct FwdLds {
    static constexpr int ES = (int)sizeof(T);
    static constexpr int PADE = 16 / ES;
    static constexpr int WP = Hp + PADE;
    static constexpr int GP3 = 3 * Hp + PADE;
    static constexpr int HFP = Hp + 4;
    static constexpr int w = 0;
    static constexpr int hf = w + (WLDS ? ES * 3 * Hp * WP : 0);
    static constexpr int hb = hf + 4 * BT * HFP;
    static constexpr int gi = hb + (ES == 2 ? 2 * BT * WP : 0);
    static constexpr int bhh = gi + ES * BT * GP3;
    static constexpr int bytes = bhh + 4 * 3 * Hp;
    static_assert(bytes <= LDS_CU_BYTES, "forward tiles do not fit the LDS");
};

// Dynamic LDS of gru_bwd_kernel: W slice (WLDS only), fp32 dh carry, h_prev
// tile, gi tile (turned into dGi in place), dGh tile, b_hh.
template <typename T, int BT, int Hp, bool WLDS>
struct BwdLds {
    static constexpr int ES = (int)sizeof(T);
    static constexpr int PADE = 16 / ES;
    static constexpr int WP = Hp + PADE;
    static constexpr int GP3 = 3 * Hp + PADE;
    static constexpr int HFP = Hp + 4;
    static constexpr int w = 0;
    static constexpr int dh = w + (WLDS ? ES * 3 * Hp * WP : 0);
    static constexpr int hb = dh + 4 * BT * HFP;
    static constexpr int gi = hb + ES * BT * WP;
    static constexpr int dgh = gi + ES * BT * GP3;
    static constexpr int bhh = dgh + ES * BT * GP3;
    static constexpr int bytes = bhh + 4 * 3 * Hp;
    static_assert(bytes <= LDS_CU_BYTES, "backward tiles do not fit the LDS");
};

// ===========================================================================
// Forward kernel.
//
// gi:    (B, T, n_dir*3Hp)  input projections incl. b_ih (dtype T)
// gi_pitch: elements between consecutive batch rows of gi. Dense gi has
//        T*n_dir*3Hp; sliding windows over a table of per-row projections
//        (window b starts at table row b*stride) have stride*n_dir*3Hp, so
//        overlapping windows share their rows. Every forward family takes
//        it; the time pitch n_dir*3Hp is the same in both layouts.
// w:     (n_dir, 3Hp, Hp)   recurrent weights, row-major [n][k] (dtype T)
// bhh:   (n_dir, 3Hp)       recurrent bias (fp32)
// out:   (B, T, n_dir*Hp)   hidden states (dtype T; direction-concat layout)
// hlast: (n_dir, B, Hp)     final hidden state (fp32)
// grid:  (ceil(B/BT), n_dir); block NT threads; direction 1 runs reversed.
// ===========================================================================
template <typename T, int BT, int Hp, bool WLDS, int NT>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT),
                          amdgpu_waves_per_eu(NT / 256, NT / 256))) void gru_fwd_kernel(
    const T* __restrict__ gi, const T* __restrict__ w,
    const float* __restrict__ bhh, T* __restrict__ out,
    float* __restrict__ hlast, int B, int Tseq, int n_dir,
    const float* __restrict__ h0, long gi_pitch) {
    constexpr int NW = NT / 64;
    constexpr int MT = BT / 16;
    constexpr int NCT = Hp / 16;
    constexpr int CPW = (NCT + NW - 1) / NW;
    constexpr bool IS_BF16 = !__is_same(T, float);
    constexpr int KK = Hp / 32;
    using L = FwdLds<T, BT, Hp, WLDS>;
    constexpr int WP = L::WP;
    constexpr int GP3 = L::GP3;
    constexpr int HFP = L::HFP;
    constexpr int GI_CHUNKS = (BT * 3 * Hp * (int)sizeof(T)) / 16;
    constexpr int PC = (GI_CHUNKS + NT - 1) / NT;

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int b0 = blockIdx.x * BT;
    const int dir = blockIdx.y;
    const bool rev = (dir == 1);
    const int rows_valid = min(BT, B - b0);

    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* w_s = WLDS ? (T*)(smem + L::w) : nullptr;
    float* hf_s = (float*)(smem + L::hf);
    __hip_bfloat16* hb_s =
        IS_BF16 ? (__hip_bfloat16*)(smem + L::hb) : nullptr;
    T* gi_s = (T*)(smem + L::gi);
    float* bhh_s = (float*)(smem + L::bhh);

    const T* wdir = w + (long)dir * 3 * Hp * Hp;
    if (WLDS)
        stage_tile<T, 3 * Hp, NT>(w_s, wdir, Hp, WP, Hp, 3 * Hp, tid);
    for (int c = tid; c < 3 * Hp; c += NT)
        bhh_s[c] = bhh[(long)dir * 3 * Hp + c];
    if (h0 != nullptr) {
        const float* h0d = h0 + ((long)dir * B + b0) * Hp;
        stage_h0_tile<float, BT, NT>(hf_s, h0d, Hp, HFP, rows_valid, tid);
        if (IS_BF16)
            stage_h0_tile<__hip_bfloat16, BT, NT>(hb_s, h0d, Hp, WP,
                                                  rows_valid, tid);
    } else {
        zero_tile<float, BT, NT>(hf_s, HFP, tid);
        if (IS_BF16) zero_tile<__hip_bfloat16, BT, NT>(hb_s, WP, tid);
    }

    const long gi_row = gi_pitch;   // elements between batch rows of gi
    const long out_row = (long)Tseq * n_dir * Hp;
    const T* gi_b = gi + (long)b0 * gi_row + (long)dir * 3 * Hp;
    T* out_b = out + (long)b0 * out_row + (long)dir * Hp;

    {   // stage gi for step 0 synchronously
        const int tt = rev ? (Tseq - 1) : 0;
        stage_tile<T, BT, NT>(gi_s, gi_b + (long)tt * n_dir * 3 * Hp, 3 * Hp,
                              GP3, gi_row, rows_valid, tid);
    }

    const T* wfrag = WLDS ? w_s : wdir;
    const long wstride = WLDS ? WP : Hp;

    __syncthreads();

    TilePrefetch<T, BT, NT, PC> pf;

    for (int u = 0; u < Tseq; ++u) {
        const int tt = rev ? (Tseq - 1 - u) : u;
        // keep the L2-streamed W pointer opaque so the compiler does not
        // hoist every fragment load out of the loop and spill
        const T* wdyn = wfrag;
        if constexpr (!WLDS && IS_BF16)
            asm volatile("" : "+s"(wdyn));

        // ---- phase A: issue next-step gi prefetch, then recurrent GEMM
        if (u + 1 < Tseq) {
            const int ttn = rev ? (Tseq - 2 - u) : (u + 1);
            pf.issue(gi_b + (long)ttn * n_dir * 3 * Hp, 3 * Hp, gi_row,
                     rows_valid, tid);
        }
        f32x4_t acc[CPW][3][MT];
#pragma unroll
        for (int i = 0; i < CPW; ++i)
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[i][g][m] = f32x4_t{0.f};

#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            const int ct = wave + NW * i;
            if (ct >= NCT) continue;
            if constexpr (IS_BF16) {
                const int arow = lane & 15;
                const int koff = 8 * (lane >> 4);
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const int kbase = 32 * kk + koff;
                    bf16x8_t a[MT];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        a[m] = *(const bf16x8_t*)&(
                            (const __bf16*)hb_s)[(16 * m + arow) * WP + kbase];
#pragma unroll
                    for (int g = 0; g < 3; ++g) {
                        const bf16x8_t b = load_wfragA<Hp>(
                            (const __hip_bfloat16*)wdyn, wstride, ct, g, kk,
                            lane);
#pragma unroll
                        for (int m = 0; m < MT; ++m)
                            acc[i][g][m] =
                                __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                    a[m], b, acc[i][g][m], 0, 0, 0);
                    }
                }
            } else {
                const int jcol = ct * 16 + (lane & 15);
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    const float* wrow = (const float*)wdyn +
                                        (long)(g * Hp + jcol) * wstride;
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int row = 16 * m + 4 * (lane >> 4) + e;
                            // explicit fma: left to the compiler, some
                            // of the unrolled (m, e) chains got fused
                            // multiply-adds and others a separate multiply
                            // and add, so a row's rounding depended on its
                            // slot in the batch tile
                            float s = acc[i][g][m][e];
                            for (int k = 0; k < Hp; ++k)
                                s = __builtin_fmaf(hf_s[row * HFP + k],
                                                   wrow[k], s);
                            acc[i][g][m][e] = s;
                        }
                }
            }
        }
        __syncthreads();  // all GEMM reads of h done

        // ---- phase B: fused gates + h update (owned (b, j) elements)
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            const int ct = wave + NW * i;
            if (ct >= NCT) continue;
            const int j = ct * 16 + (lane & 15);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * m + 4 * (lane >> 4) + e;
                    const float gr = acc[i][0][m][e] + bhh_s[j];
                    const float gz = acc[i][1][m][e] + bhh_s[Hp + j];
                    const float hn = acc[i][2][m][e] + bhh_s[2 * Hp + j];
                    const float ir = to_f32<T>(gi_s[b * GP3 + j]);
                    const float iz = to_f32<T>(gi_s[b * GP3 + Hp + j]);
                    const float in_ = to_f32<T>(gi_s[b * GP3 + 2 * Hp + j]);
                    const float r = sigmoidf(ir + gr);
                    const float z = sigmoidf(iz + gz);
                    const float n = fast_tanh(in_ + r * hn);
                    const float hprev = hf_s[b * HFP + j];
                    const float hnew = (1.0f - z) * n + z * hprev;
                    hf_s[b * HFP + j] = hnew;
                    if constexpr (IS_BF16)
                        hb_s[b * WP + j] = __float2bfloat16(hnew);
                }
            }
        }
        __syncthreads();  // h_t complete; gi_s free

        // ---- phase C: commit prefetched gi, then write out[t]. Commit
        // goes FIRST: its s_waitcnt vmcnt(0) then waits only for the gi
        // loads issued back in phase A (long returned), not for the out[t]
        // stores (which would add a store-completion stall every step).
        if (u + 1 < Tseq) pf.commit(gi_s, 3 * Hp, GP3, tid);
        if constexpr (IS_BF16) {
            store_tile<__hip_bfloat16, BT, NT>(
                hb_s, (__hip_bfloat16*)(out_b + (long)tt * n_dir * Hp), Hp, WP,
                out_row, rows_valid, tid);
        } else {
            store_tile<float, BT, NT>(
                hf_s, (float*)(out_b + (long)tt * n_dir * Hp), Hp, HFP,
                out_row, rows_valid, tid);
        }
        __syncthreads();
    }

    // final hidden state (fp32)
    float* hl = hlast + ((long)dir * B + b0) * Hp;
    for (int c = tid; c < BT * Hp; c += NT) {
        const int r = c / Hp;
        if (r < rows_valid)
            hl[(long)r * Hp + (c % Hp)] = hf_s[r * HFP + (c % Hp)];
    }
}

// ===========================================================================
// Backward (BPTT) kernel. See the header comment for the dGh time-shift and
// the in-kernel db_hh reduction.
// ===========================================================================
template <typename T, int BT, int Hp, bool WLDS, int NT>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT),
                          amdgpu_waves_per_eu(NT / 256, NT / 256))) void gru_bwd_kernel(
    const T* __restrict__ gi, const T* __restrict__ w,
    const float* __restrict__ bhh, const T* __restrict__ out,
    const T* __restrict__ dout, const float* __restrict__ dhT,
    T* __restrict__ dgi, T* __restrict__ dgh, float* __restrict__ dh0,
    float* __restrict__ dbhh, int B, int Tseq, int n_dir,
    const float* __restrict__ h0, T* __restrict__ dgh0) {
    constexpr int NW = NT / 64;
    constexpr int MT = BT / 16;
    constexpr int NCT = Hp / 16;
    constexpr int CPW = (NCT + NW - 1) / NW;
    constexpr bool IS_BF16 = !__is_same(T, float);
    constexpr int KK = Hp / 32;
    constexpr int KK2 = (3 * Hp) / 32;
    using L = BwdLds<T, BT, Hp, WLDS>;
    constexpr int WP = L::WP;
    constexpr int GP3 = L::GP3;
    constexpr int HFP = L::HFP;
    constexpr int GI_CHUNKS = (BT * 3 * Hp * (int)sizeof(T)) / 16;
    constexpr int H_CHUNKS = (BT * Hp * (int)sizeof(T)) / 16;
    constexpr int PCG = (GI_CHUNKS + NT - 1) / NT;
    constexpr int PCH = (H_CHUNKS + NT - 1) / NT;

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int b0 = blockIdx.x * BT;
    const int dir = blockIdx.y;
    const bool rev = (dir == 1);
    const int rows_valid = min(BT, B - b0);

    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* w_s = WLDS ? (T*)(smem + L::w) : nullptr;
    float* dh_s = (float*)(smem + L::dh);
    T* hb_s = (T*)(smem + L::hb);
    T* gi_s = (T*)(smem + L::gi);   // gi[t] -> dGi in place
    T* dgh_s = (T*)(smem + L::dgh);
    float* bhh_s = (float*)(smem + L::bhh);

    const T* wdir = w + (long)dir * 3 * Hp * Hp;
    if (WLDS)
        stage_tile<T, 3 * Hp, NT>(w_s, wdir, Hp, WP, Hp, 3 * Hp, tid);
    for (int c = tid; c < 3 * Hp; c += NT)
        bhh_s[c] = bhh[(long)dir * 3 * Hp + c];

    const long gi_row = (long)Tseq * n_dir * 3 * Hp;
    const long out_row = (long)Tseq * n_dir * Hp;
    const T* gi_b = gi + (long)b0 * gi_row + (long)dir * 3 * Hp;
    T* dgi_b = dgi + (long)b0 * gi_row + (long)dir * 3 * Hp;
    T* dgh_b = dgh + (long)b0 * gi_row + (long)dir * 3 * Hp;
    const T* out_b = out + (long)b0 * out_row + (long)dir * Hp;
    const T* dout_b = dout + (long)b0 * out_row + (long)dir * Hp;

    {   // dh carry init: dh = dhT
        const float* hT = dhT + ((long)dir * B + b0) * Hp;
        for (int c = tid; c < BT * Hp; c += NT) {
            const int r = c / Hp;
            dh_s[r * HFP + (c % Hp)] =
                (r < rows_valid) ? hT[(long)r * Hp + (c % Hp)] : 0.0f;
        }
    }

    {   // stage step u = Tseq-1 synchronously
        const int u = Tseq - 1;
        const int tt = rev ? (Tseq - 1 - u) : u;
        stage_tile<T, BT, NT>(gi_s, gi_b + (long)tt * n_dir * 3 * Hp, 3 * Hp,
                              GP3, gi_row, rows_valid, tid);
        if (u > 0) {
            const int ttp = rev ? (Tseq - u) : (u - 1);
            stage_tile<T, BT, NT>(hb_s, out_b + (long)ttp * n_dir * Hp, Hp, WP,
                                  out_row, rows_valid, tid);
        } else if (h0 != nullptr) {
            stage_h0_tile<T, BT, NT>(hb_s, h0 + ((long)dir * B + b0) * Hp, Hp,
                                     WP, rows_valid, tid);
        } else {
            zero_tile<T, BT, NT>(hb_s, WP, tid);
        }
        accum_tile_f32<T, BT, NT>(dh_s, dout_b + (long)tt * n_dir * Hp, Hp,
                                  HFP, out_row, rows_valid, tid);
    }

    const T* wfrag = WLDS ? w_s : wdir;
    const long wstride = WLDS ? WP : Hp;

    __syncthreads();

    float dbacc[CPW][4];   // dr, dz, dhn (db_hh) + dn (db_ih n-slot)
#pragma unroll
    for (int i = 0; i < CPW; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) dbacc[i][g] = 0.0f;

    TilePrefetch<T, BT, NT, PCG> pf_gi;
    TilePrefetch<T, BT, NT, PCH> pf_hb;
    TilePrefetch<T, BT, NT, PCH> pf_do;

    for (int u = Tseq - 1; u >= 0; --u) {
        const int tt = rev ? (Tseq - 1 - u) : u;
        const bool have_next = (u > 0);
        const int un = u - 1;
        const int ttn = rev ? (Tseq - 1 - un) : un;
        const T* wdyn = wfrag;
        if constexpr (!WLDS && IS_BF16)
            asm volatile("" : "+s"(wdyn));

        if (have_next) {
            pf_gi.issue(gi_b + (long)ttn * n_dir * 3 * Hp, 3 * Hp, gi_row,
                        rows_valid, tid);
            if (un > 0) {
                const int ttp = rev ? (Tseq - un) : (un - 1);
                pf_hb.issue(out_b + (long)ttp * n_dir * Hp, Hp, out_row,
                            rows_valid, tid);
            }
            pf_do.issue(dout_b + (long)ttn * n_dir * Hp, Hp, out_row,
                        rows_valid, tid);
        }

        // ---- phase A: recompute gh, fuse gate grads (per owned column tile)
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            const int ct = wave + NW * i;
            if (ct >= NCT) continue;
            f32x4_t acc[3][MT];
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[g][m] = f32x4_t{0.f};
            if constexpr (IS_BF16) {
                const int arow = lane & 15;
                const int koff = 8 * (lane >> 4);
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const int kbase = 32 * kk + koff;
                    bf16x8_t a[MT];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        a[m] = *(const bf16x8_t*)&(
                            (const __bf16*)hb_s)[(16 * m + arow) * WP + kbase];
#pragma unroll
                    for (int g = 0; g < 3; ++g) {
                        const bf16x8_t b = load_wfragA<Hp>(
                            (const __hip_bfloat16*)wdyn, wstride, ct, g, kk,
                            lane);
#pragma unroll
                        for (int m = 0; m < MT; ++m)
                            acc[g][m] =
                                __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                    a[m], b, acc[g][m], 0, 0, 0);
                    }
                }
            } else {
                const int jcol = ct * 16 + (lane & 15);
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    const float* wrow = (const float*)wdyn +
                                        (long)(g * Hp + jcol) * wstride;
#pragma unroll
                    for (int m = 0; m < MT; ++m)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int row = 16 * m + 4 * (lane >> 4) + e;
                            // explicit fma, as in the forward kernel: the
                            // same rounding for every (m, e) row slot
                            float s = acc[g][m][e];
                            for (int k = 0; k < Hp; ++k)
                                s = __builtin_fmaf(
                                    to_f32<T>(hb_s[row * WP + k]), wrow[k], s);
                            acc[g][m][e] = s;
                        }
                }
            }

            const int j = ct * 16 + (lane & 15);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * m + 4 * (lane >> 4) + e;
                    const float gr = acc[0][m][e] + bhh_s[j];
                    const float gz = acc[1][m][e] + bhh_s[Hp + j];
                    const float hn = acc[2][m][e] + bhh_s[2 * Hp + j];
                    const float ir = to_f32<T>(gi_s[b * GP3 + j]);
                    const float iz = to_f32<T>(gi_s[b * GP3 + Hp + j]);
                    const float in_ = to_f32<T>(gi_s[b * GP3 + 2 * Hp + j]);
                    const float r = sigmoidf(ir + gr);
                    const float z = sigmoidf(iz + gz);
                    const float n = fast_tanh(in_ + r * hn);
                    const float hprev = to_f32<T>(hb_s[b * WP + j]);
                    const float dht = dh_s[b * HFP + j];
                    const bool live = (b < rows_valid);
                    // Every dead-row product must be gated on `live`, not
                    // just zeroed upstream: uninitialized LDS can hold inf/
                    // NaN and 0 * inf = NaN would leak into dbacc below.
                    const float dz_pre =
                        live ? dht * (hprev - n) * z * (1.0f - z) : 0.0f;
                    const float dn_pre =
                        live ? dht * (1.0f - z) * (1.0f - n * n) : 0.0f;
                    const float dr_pre =
                        live ? dn_pre * hn * r * (1.0f - r) : 0.0f;
                    const float dhn = live ? dn_pre * r : 0.0f;
                    gi_s[b * GP3 + j] = from_f32<T>(dr_pre);
                    gi_s[b * GP3 + Hp + j] = from_f32<T>(dz_pre);
                    gi_s[b * GP3 + 2 * Hp + j] = from_f32<T>(dn_pre);
                    dgh_s[b * GP3 + j] = from_f32<T>(dr_pre);
                    dgh_s[b * GP3 + Hp + j] = from_f32<T>(dz_pre);
                    dgh_s[b * GP3 + 2 * Hp + j] = from_f32<T>(dhn);
                    dh_s[b * HFP + j] = live ? dht * z : 0.0f;
                    dbacc[i][0] += dr_pre;
                    dbacc[i][1] += dz_pre;
                    dbacc[i][2] += dhn;
                    dbacc[i][3] += dn_pre;
                }
            }
        }
        __syncthreads();  // dgh_s complete

        // ---- phase B: dh_{t-1} += dGh @ W
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            const int ct = wave + NW * i;
            if (ct >= NCT) continue;
            f32x4_t acc2[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) acc2[m] = f32x4_t{0.f};
            if constexpr (IS_BF16) {
                const int arow = lane & 15;
                const int koff = 8 * (lane >> 4);
#pragma unroll
                for (int kk = 0; kk < KK2; ++kk) {
                    const int kbase = 32 * kk + koff;
                    bf16x8_t a[MT];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        a[m] = *(const bf16x8_t*)&(
                            (const __bf16*)dgh_s)[(16 * m + arow) * GP3 +
                                                  kbase];
                    const bf16x8_t b = load_wfragB<Hp>(
                        (const __hip_bfloat16*)wdyn, wstride, ct, kk, lane);
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        acc2[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            a[m], b, acc2[m], 0, 0, 0);
                }
            } else {
                const int jcol = ct * 16 + (lane & 15);
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int row = 16 * m + 4 * (lane >> 4) + e;
                        float s = acc2[m][e];
                        for (int n = 0; n < 3 * Hp; ++n)
                            s = __builtin_fmaf(
                                to_f32<T>(dgh_s[row * GP3 + n]),
                                ((const float*)wdyn)[(long)n * wstride + jcol],
                                s);
                        acc2[m][e] = s;
                    }
            }
            const int j = ct * 16 + (lane & 15);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * m + 4 * (lane >> 4) + e;
                    dh_s[b * HFP + j] += acc2[m][e];
                }
        }
        __syncthreads();

        // ---- phase C: commit prefetches, then write dGi / dGh. The first
        // commit's s_waitcnt vmcnt(0) waits only for phase-A loads, not the
        // stores below (which would stall every step on store completion).
        // gi_s is read (dGi values) and rewritten (next gi) by the SAME
        // thread's chunk assignment, so store-then-commit within one thread
        // needs no barrier; commits of hb_s/dh_s touch buffers no store
        // reads.
        if (have_next) {
            if (un > 0)
                pf_hb.commit(hb_s, Hp, WP, tid);
            else if (h0 != nullptr)
                stage_h0_tile<T, BT, NT>(hb_s,
                                         h0 + ((long)dir * B + b0) * Hp, Hp,
                                         WP, rows_valid, tid);
            else
                zero_tile<T, BT, NT>(hb_s, WP, tid);
            pf_do.commit_accum_f32(dh_s, Hp, HFP, rows_valid, tid);
        }
        store_tile<T, BT, NT>(gi_s, dgi_b + (long)tt * n_dir * 3 * Hp, 3 * Hp,
                              GP3, gi_row, rows_valid, tid);
        {
            const int slot = rev ? (tt + 1) : (tt - 1);
            if (slot >= 0 && slot < Tseq) {
                store_tile<T, BT, NT>(dgh_s,
                                      dgh_b + (long)slot * n_dir * 3 * Hp,
                                      3 * Hp, GP3, gi_row, rows_valid, tid);
            } else {
                // u = 0: this dGh pairs with h_{-1}. Its global slot gets
                // zeros (the dW_hh reduction pairs slots with out[t]); with
                // an initial hidden state the values go to dgh0 instead so
                // the host can add the dGh_0 (x) h0 term to dW_hh.
                store_zero_tile<T, BT, NT>(
                    dgh_b + (long)(rev ? 0 : (Tseq - 1)) * n_dir * 3 * Hp,
                    3 * Hp, gi_row, rows_valid, tid);
                if (dgh0 != nullptr)
                    store_tile<T, BT, NT>(
                        dgh_s, dgh0 + ((long)dir * B + b0) * 3 * Hp, 3 * Hp,
                        GP3, 3 * Hp, rows_valid, tid);
            }
        }
        if (have_next)
            pf_gi.commit(gi_s, 3 * Hp, GP3, tid);
        __syncthreads();
    }

    // dh0 (fp32)
    float* d0 = dh0 + ((long)dir * B + b0) * Hp;
    for (int c = tid; c < BT * Hp; c += NT) {
        const int r = c / Hp;
        if (r < rows_valid)
            d0[(long)r * Hp + (c % Hp)] = dh_s[r * HFP + (c % Hp)];
    }

    // bias grads: reduce the 4 row-quarter lanes (same j = lane&15), then
    // one store per (slot, column) into THIS batch tile's row of the
    // partials table — (batch tile, n_dir, 4Hp), summed over tiles by the
    // host in a fixed order, so the result is bitwise reproducible (a
    // float atomicAdd across blocks is not). Row layout (n_dir, 4Hp):
    // [dr, dz, dhn | dn] — db_hh = slots 0..2, db_ih = slots 0,1,3.
    float* dbrow = dbhh + ((long)blockIdx.x * n_dir + dir) * 4 * Hp;
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int ct = wave + NW * i;
        if (ct >= NCT) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float v = dbacc[i][g];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if ((lane >> 4) == 0)
                dbrow[g * Hp + ct * 16 + (lane & 15)] = v;
        }
    }
}

// ===========================================================================
// v3 kernels (bf16, Hp = 128 hot path).
//
// What changed vs the v2 phase structure above, and why (measured on
// MI355X, profiles/r01*):
// - v2 spent 72% of wave time parked: 3 __syncthreads per step, a register
//   prefetch the allocator spilled to scratch (global!) with an immediate
//   vmcnt(0) stall, and gi staged through chunk registers.
// - v3 stages gi by LDS-DMA (`global_load_lds`, 16 B/lane, lane-linear
//   image) into a ring, so staging costs zero registers and no commit
//   pass; raw `s_barrier` + counted `s_waitcnt vmcnt(N)` keep the DMA in
//   flight across barriers (cdna_hip_programming.md glds rules).
// - fp32 h lives in REGISTERS (each lane owns its MFMA C elements (b, j)
//   across all timesteps); LDS holds only the bf16 copy the MFMA
//   A-fragments need, double-buffered so the step loop has exactly TWO raw
//   barriers (GEMM reads hb[p] while gates write hb[1-p]).
// - forward runs BT=16/NT=256 with amdgpu_waves_per_eu(2,2): two BLOCKS
//   per CU, whose independent serial chains hide each other's latencies.
// - out[t-1] is stored one step late (from the buffer the GEMM is reading
//   anyway), decoupling store completion from the chain.
// ===========================================================================

FMDA_DEV void glds16(const void* gsrc, void* ldst) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)gsrc,
        (__attribute__((address_space(3))) unsigned int*)ldst, 16, 0, 0);
}

// Dynamic LDS of gru_fwd_v3_kernel: the two-slot gi ring (unpadded rows, the
// lane-linear image of the DMA), the double-buffered bf16 h tile at the
// padded pitch WP (elements), b_hh.
template <int BT, int Hp>
struct FwdV3Lds {
    static constexpr int GP = 3 * Hp;
    static constexpr int WP = Hp + 8;
    static constexpr int gi0 = 0;
    static constexpr int gi1 = gi0 + 2 * BT * GP;
    static constexpr int hb0 = gi1 + 2 * BT * GP;
    static constexpr int hb1 = hb0 + 2 * BT * WP;
    static constexpr int bhh = hb1 + 2 * BT * WP;
    static constexpr int bytes = bhh + 4 * 3 * Hp;
    static_assert(bytes <= LDS_CU_BYTES, "forward tiles do not fit the LDS");
};

template <int BT, int Hp, int NT, int WPE>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT),
                          amdgpu_waves_per_eu(WPE, WPE)))
void gru_fwd_v3_kernel(const __hip_bfloat16* __restrict__ gi,
                       const __hip_bfloat16* __restrict__ w,
                       const float* __restrict__ bhh,
                       __hip_bfloat16* __restrict__ out,
                       float* __restrict__ hlast, int B, int Tseq,
                       int n_dir, const float* __restrict__ h0,
                       __hip_bfloat16* __restrict__ out_drop,
                       unsigned int drop_thr, float drop_scale,
                       unsigned long long drop_seed, long gi_pitch) {
    constexpr int NW = NT / 64;
    constexpr int MT = BT / 16;
    constexpr int NCT = Hp / 16;
    constexpr int CPW = NCT / NW;
    constexpr int KK = Hp / 32;
    using L = FwdV3Lds<BT, Hp>;
    constexpr int GP = L::GP;            // unpadded gi pitch (lane-linear DMA)
    constexpr int WP = L::WP;            // padded bf16 h pitch
    constexpr int PIECES = (BT * GP * 2) / 1024;
    constexpr int PW = PIECES / NW;      // glds instructions per wave per step
    static_assert(PIECES % NW == 0 && NCT % NW == 0, "tiling mismatch");

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int b0 = blockIdx.x * BT;
    const int dir = blockIdx.y;
    const bool rev = (dir == 1);
    const int rows_valid = min(BT, B - b0);

    extern __shared__ __attribute__((aligned(16))) char smem[];
    // Select HELPERS, not pointer arrays: a runtime-indexed local pointer
    // array defeats LDS address-space inference, so every gi/h access in
    // the loop compiled to FLAT ops — which wait on vmcnt and made the
    // compiler drain the in-flight LDS-DMA with a vmcnt(0) before every
    // gate group (the 2.4x slowdown this comment is a tombstone for).
    __hip_bfloat16* gi_s0 = (__hip_bfloat16*)(smem + L::gi0);
    __hip_bfloat16* gi_s1 = (__hip_bfloat16*)(smem + L::gi1);
    __hip_bfloat16* hb_s0 = (__hip_bfloat16*)(smem + L::hb0);
    __hip_bfloat16* hb_s1 = (__hip_bfloat16*)(smem + L::hb1);
    float* bhh_s = (float*)(smem + L::bhh);
    auto gi_buf = [&](int b) { return b ? gi_s1 : gi_s0; };
    auto hb_buf = [&](int b) { return b ? hb_s1 : hb_s0; };

    const long gi_row = gi_pitch;   // elements between batch rows of gi
    const long out_row = (long)Tseq * n_dir * Hp;
    const __hip_bfloat16* gi_b = gi + (long)b0 * gi_row + (long)dir * 3 * Hp;
    __hip_bfloat16* out_b = out + (long)b0 * out_row + (long)dir * Hp;
    __hip_bfloat16* outd_b =
        (out_drop != nullptr)
            ? out_drop + (long)b0 * out_row + (long)dir * Hp : nullptr;

    // Fused forward half of the inter-layer dropout (the backward half
    // lives in gru_bwd_v3_kernel's d_out read): the same counter-based
    // octet mask as dropout_kernel over the (B, T, n_dir*Hp) `out` layout,
    // applied while the data is still in LDS — the separate full-tensor
    // dropout pass (1 read + 1 write of ~0.5 GB at the flagship config)
    // becomes one extra store stream here.
    auto store_dropped = [&](const __hip_bfloat16* hb, int ttp) {
        constexpr int CPR = (Hp * 2) / 16;    // 16-byte chunks per row
        __hip_bfloat16* dst = outd_b + (long)ttp * n_dir * Hp;
        for (int c = tid; c < BT * CPR; c += NT) {
            const int r = c / CPR, jc = c % CPR;
            if (r >= rows_valid) continue;
            bf16x8_t v = *(const bf16x8_t*)((const char*)hb +
                                            (long)r * WP * 2 + jc * 16);
            const long o = ((long)(b0 + r) * Tseq + ttp) * n_dir * Hp +
                           (long)dir * Hp + jc * 8;   // octet-aligned
            const unsigned long long rnd =
                mix64(drop_seed ^ (unsigned long long)(o >> 3));
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned int u = (unsigned int)(rnd >> (8 * k)) & 0xFF;
                const float f =
                    (u < drop_thr)
                        ? 0.0f : (float)((__bf16*)&v)[k] * drop_scale;
                ((__bf16*)&v)[k] = (__bf16)__float2bfloat16(f);
            }
            *(bf16x8_t*)((char*)dst + (long)r * out_row * 2 + jc * 16) = v;
        }
    };

    for (int c = tid; c < 3 * Hp; c += NT)
        bhh_s[c] = bhh[(long)dir * 3 * Hp + c];
    const float* h0d = (h0 != nullptr) ? h0 + ((long)dir * B + b0) * Hp
                                       : nullptr;
    if (h0d != nullptr)
        stage_h0_tile<__hip_bfloat16, BT, NT>(hb_s0, h0d, Hp, WP, rows_valid,
                                              tid);
    else
        zero_tile<__hip_bfloat16, BT, NT>(hb_s0, WP, tid);

    // W_hh B-fragments, register-resident for the whole sequence.
    const __hip_bfloat16* wdir = w + (long)dir * 3 * Hp * Hp;
    bf16x8_t wA[CPW][3][KK];
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int ct = wave + NW * i;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                wA[i][g][kk] = load_wfragA<Hp>(wdir, Hp, ct, g, kk, lane);
    }

    float hreg[CPW][MT][4];
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int ct = wave + NW * i;
        const int j = ct * 16 + (lane & 15);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = 16 * m + 4 * (lane >> 4) + e;
                hreg[i][m][e] = (h0d != nullptr && b < rows_valid)
                                    ? h0d[(long)b * Hp + j] : 0.0f;
            }
    }

    // Lane-linear LDS-DMA of one timestep's gi tile (per-lane global
    // addresses handle the strided batch rows; dead rows clamp to row 0).
    const int wavu = __builtin_amdgcn_readfirstlane(wave);
    auto glds_tile = [&](int tt, int buf) {
        const __hip_bfloat16* src_t = gi_b + (long)tt * n_dir * 3 * Hp;
#pragma unroll
        for (int k = 0; k < PW; ++k) {
            const int off = (wavu * PW + k) * 1024 + lane * 16;  // bytes
            const int e = off >> 1;
            int r = e / GP;
            const int c = e % GP;
            if (r >= rows_valid) r = 0;
            glds16(src_t + (long)r * gi_row + c,
                   (char*)gi_buf(buf) + (long)(wavu * PW + k) * 1024);
        }
    };

    {   // prologue: stage step 0 synchronously
        glds_tile(rev ? (Tseq - 1) : 0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    for (int u = 0; u < Tseq; ++u) {
        const int pb = u & 1;
        const int tt = rev ? (Tseq - 1 - u) : u;

        // ---- phase A: DMA gi[u+1] first, then store out[u-1] (issue
        // order matters: the B-end counted wait leaves only the store in
        // flight), then the recurrent GEMM ----
        if (u + 1 < Tseq)
            glds_tile(rev ? (Tseq - 2 - u) : (u + 1), 1 - pb);
        if (u > 0) {
            const int ttp = rev ? (Tseq - u) : (u - 1);
            store_tile<__hip_bfloat16, BT, NT>(
                hb_buf(pb), out_b + (long)ttp * n_dir * Hp, Hp, WP, out_row,
                rows_valid, tid);
            if (outd_b != nullptr) store_dropped(hb_buf(pb), ttp);
        }

        f32x4_t acc[CPW][3][MT];
#pragma unroll
        for (int i = 0; i < CPW; ++i)
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[i][g][m] = f32x4_t{0.f};
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            const int arow = lane & 15;
            const int koff = 8 * (lane >> 4);
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const int kbase = 32 * kk + koff;
                bf16x8_t a[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    a[m] = *(const bf16x8_t*)&(
                        (const __bf16*)hb_buf(pb))[(16 * m + arow) * WP +
                                                   kbase];
#pragma unroll
                for (int g = 0; g < 3; ++g)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        acc[i][g][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            a[m], wA[i][g][kk], acc[i][g][m], 0, 0, 0);
            }
        }
        // No barrier between A and B: the GEMM reads hb[pb] and glds
        // writes gi_s[1-pb] while the gates (B) read gi_s[pb] and write
        // hb[1-pb] — all buffer-disjoint. The single per-step barrier
        // lives at B-end and doubles as the DMA rendezvous for the tile
        // issued THIS step (read next step).

        // ---- phase B: fused gates; h stays in registers ----
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            const int ct = wave + NW * i;
            const int j = ct * 16 + (lane & 15);
            const __bf16* gprow = (const __bf16*)gi_buf(pb);
            __bf16* hrow = (__bf16*)hb_buf(1 - pb);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * m + 4 * (lane >> 4) + e;
                    const float gr = acc[i][0][m][e] + bhh_s[j];
                    const float gz = acc[i][1][m][e] + bhh_s[Hp + j];
                    const float hn = acc[i][2][m][e] + bhh_s[2 * Hp + j];
                    const float ir = (float)gprow[b * GP + j];
                    const float iz = (float)gprow[b * GP + Hp + j];
                    const float in_ = (float)gprow[b * GP + 2 * Hp + j];
                    const float r = sigmoidf(ir + gr);
                    const float z = sigmoidf(iz + gz);
                    const float n = fast_tanh(in_ + r * hn);
                    const float hprev = hreg[i][m][e];
                    const float hnew = (1.0f - z) * n + z * hprev;
                    hreg[i][m][e] = hnew;
                    hrow[b * WP + j] = (__bf16)__float2bfloat16(hnew);
                }
            }
        }
        // rendezvous: drain this step's glds (tile u+1) across all waves,
        // leaving the out[u-1] store (and, when fused dropout is on, the
        // out_drop[u-1] store — one more instruction per thread) in
        // flight: both were issued after the glds, so the counted wait
        // never stalls on store completion. The leave-count is PER-THREAD
        // exact: a batch-tail thread whose row is dead issued no store, so
        // leaving 1 outstanding there would leave a gi glds un-drained.
        {
            // vmcnt is per-WAVE: each store pass issues one instruction per
            // wave iff any of the wave's rows is live (first row suffices:
            // rows are wave-contiguous).
            constexpr int RPW = 64 / ((Hp * 2) / 16);   // rows per wave
            const bool wave_stored = (u > 0) && (wave * RPW < rows_valid);
            const int leave =
                wave_stored ? (outd_b != nullptr ? 2 : 1) : 0;
            if (leave == 2)
                asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else if (leave == 1)
                asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    {   // epilogue: out[T-1] + hlast
        const int pl = Tseq & 1;
        const int ttl = rev ? 0 : (Tseq - 1);
        store_tile<__hip_bfloat16, BT, NT>(
            hb_buf(pl), out_b + (long)ttl * n_dir * Hp, Hp, WP, out_row,
            rows_valid, tid);
        if (outd_b != nullptr) store_dropped(hb_buf(pl), ttl);
        float* hl = hlast + ((long)dir * B + b0) * Hp;
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            const int ct = wave + NW * i;
            const int j = ct * 16 + (lane & 15);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * m + 4 * (lane >> 4) + e;
                    if (b < rows_valid) hl[(long)b * Hp + j] = hreg[i][m][e];
                }
        }
    }
}

// v3 backward (third structure — the one that measures fastest; the
// previous two are documented here so they are not rediscovered):
//   (1) glds tiles + per-step W^T fragments as ordinary L2 loads: ROCm 7.2
//       rewrites every use of an ordinary-load result into s_waitcnt
//       vmcnt(0) while ANY glds is in flight, so each step drained the
//       whole DMA pipeline and parked 67% of wave time.
//   (2) register staging everywhere (no glds): the chunk registers pushed
//       allocation past 256 VGPRs and the spill RELOADS are themselves
//       ordinary loads — 2x slower again.
//   => ALL in-loop VMEM must be glds or stores; both W fragment sets are
//      hoisted ONCE in the prologue (their one-time loads complete before
//      the loop); the kernel must allocate with ZERO spills.
// h tiles (read as MFMA A-fragments) are DMA'd with an XOR-swizzled
// SOURCE address (lane-linear LDS image, cdna_hip_programming.md rule 21):
// LDS[r][k16] holds out[r][k16 ^ (r & 15)], so fragment reads at
// row*256 + ((k16 ^ (r & 15)) * 16) touch 16 distinct 16-byte slots per
// 16-row group instead of one (16-way conflict at the unswizzled pitch).
// Phases: A[glds issues + one-step-late dGi/dGh stores] -> rendezvous ->
// B[recompute GEMM + fused gate grads] -> barrier -> C[carry GEMM from
// dgh_s, register-only] -> (no barrier).
// ===========================================================================
// Batch-1 forward for streaming inference (the predict path).
//
// At batch 1 the batch-tiled forward launches 2 blocks on 256 CUs and pays
// a per-step LDS-DMA rendezvous for a tile that contains one live row.
// This kernel instead makes the whole problem LDS/register-resident:
// the ENTIRE gi sequence (T x 3Hp bf16, ~94 KB at T=120) is staged into
// LDS once, W_hh fragments are register-hoisted as in v3, and h crosses
// timesteps through a 2-slot LDS ring — one __syncthreads per step and
// zero global traffic in the loop except the 256 B/step `out` write.
// MFMA layout: batch is the M dimension (A-fragment rows; only row 0 is
// live, supplied by the l%16==0 lanes), so each output lane l<16 holds
// r, z and n for the SAME h column across its three accumulators and the
// gate math needs no cross-lane traffic. Latency-bound by design: 24
// MFMAs + one barrier per step per wave.
// ===========================================================================

// Dynamic LDS of gru_fwd_b1_body (byte offsets) for a sequence of Tseq
// steps: the whole gi sequence at the padded row pitch GIP (elements), the
// two-slot h ring (pitch HRP), b_hh. The same layout serves the batch-1,
// streams and bank kernels.
template <int Hp>
struct B1Lds {
    static constexpr int GIP = 3 * Hp + 8;
    static constexpr int HRP = Hp + 8;
    long gi, hr0, hr1, bhh, bytes;
    __host__ __device__ constexpr explicit B1Lds(int Tseq)
        : gi(0), hr0(gi + 2 * (long)Tseq * GIP), hr1(hr0 + 2 * HRP),
          bhh(hr1 + 2 * HRP), bytes(bhh + 4 * 3 * Hp) {}
};

// One block's work, shared by the single-sequence kernel and the
// multi-stream kernel below: direction blockIdx.x of ONE sequence. gi and
// out point at that sequence's slab, h0 (or null) at its (n_dir, Hp)
// initial state; this direction's (Hp) fp32 h_last goes to hlast + hl_off.
template <int Hp, int NT>
__device__ __forceinline__
void gru_fwd_b1_body(const __hip_bfloat16* __restrict__ gi,
                     const __hip_bfloat16* __restrict__ w,
                     const float* __restrict__ bhh,
                     __hip_bfloat16* __restrict__ out,
                     float* __restrict__ hlast, int Tseq, int n_dir,
                     const float* __restrict__ h0, long hl_off) {
    constexpr int NW = NT / 64;      // 4 waves
    constexpr int CT = Hp / 16;      // 8 h-column tiles
    constexpr int CPW = CT / NW;     // 2 per wave
    constexpr int KK = Hp / 32;
    constexpr int GIP = B1Lds<Hp>::GIP;  // padded gi row pitch (elements)
    constexpr int HRP = B1Lds<Hp>::HRP;  // h ring pitch
    static_assert(CT % NW == 0, "tiling mismatch");

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int dir = blockIdx.x;
    const bool rev = (dir == 1);

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const B1Lds<Hp> L(Tseq);
    __hip_bfloat16* gi_s = (__hip_bfloat16*)(smem + L.gi);
    __hip_bfloat16* hr0 = (__hip_bfloat16*)(smem + L.hr0);
    __hip_bfloat16* hr1 = (__hip_bfloat16*)(smem + L.hr1);
    float* bhh_s = (float*)(smem + L.bhh);
    auto hring = [&](int s) { return s ? hr1 : hr0; };

    // stage the whole gi sequence (batch row 0, this direction); with a
    // single batch row the kernel needs no gi batch pitch
    const __hip_bfloat16* gi_b = gi + (long)dir * 3 * Hp;
    const long gi_trow = (long)n_dir * 3 * Hp;
    for (int idx = tid; idx < Tseq * (3 * Hp / 8); idx += NT) {
        const int t = idx / (3 * Hp / 8);
        const int c8 = idx % (3 * Hp / 8);
        *(bf16x8_t*)(gi_s + (long)t * GIP + c8 * 8) =
            *(const bf16x8_t*)(gi_b + t * gi_trow + c8 * 8);
    }
    for (int c = tid; c < 3 * Hp; c += NT)
        bhh_s[c] = bhh[(long)dir * 3 * Hp + c];
    const float* h0d = (h0 != nullptr) ? h0 + (long)dir * Hp : nullptr;
    for (int c = tid; c < HRP; c += NT)
        ((__bf16*)hr0)[c] = (h0d != nullptr && c < Hp)
                                ? (__bf16)__float2bfloat16(h0d[c])
                                : (__bf16)0.0f;

    const __hip_bfloat16* wdir = w + (long)dir * 3 * Hp * Hp;
    bf16x8_t wA[CPW][3][KK];
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int ct = wave + NW * i;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                wA[i][g][kk] = load_wfragA<Hp>(wdir, Hp, ct, g, kk, lane);
    }
    float hreg[CPW];                 // this lane's h column (lanes 0..15)
#pragma unroll
    for (int i = 0; i < CPW; ++i)
        hreg[i] = (h0d != nullptr)
                      ? h0d[(wave + NW * i) * 16 + (lane & 15)] : 0.0f;

    __hip_bfloat16* out_b = out + (long)dir * Hp;   // batch row 0
    const long out_trow = (long)n_dir * Hp;
    __syncthreads();

    for (int u = 0; u < Tseq; ++u) {
        const int tt = rev ? (Tseq - 1 - u) : u;
        const __bf16* hs = (const __bf16*)hring(u & 1);

        f32x4_t acc[CPW][3];
#pragma unroll
        for (int i = 0; i < CPW; ++i)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[i][g] = f32x4_t{0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            bf16x8_t a;
            if ((lane & 15) == 0)
                a = *(const bf16x8_t*)&hs[32 * kk + 8 * (lane >> 4)];
            else
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] = (__bf16)0.0f;
#pragma unroll
            for (int i = 0; i < CPW; ++i)
#pragma unroll
                for (int g = 0; g < 3; ++g)
                    acc[i][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a, wA[i][g][kk], acc[i][g], 0, 0, 0);
        }

        // gates: batch row 0 lives in C row 0 -> lanes 0..15, element 0
        __bf16* hw = (__bf16*)hring(1 - (u & 1));
        if ((lane >> 4) == 0) {
#pragma unroll
            for (int i = 0; i < CPW; ++i) {
                const int ct = wave + NW * i;
                const int j = ct * 16 + lane;
                const float gr = acc[i][0][0] + bhh_s[j];
                const float gz = acc[i][1][0] + bhh_s[Hp + j];
                const float hn = acc[i][2][0] + bhh_s[2 * Hp + j];
                const __bf16* gt = (const __bf16*)gi_s + (long)tt * GIP;
                const float r = sigmoidf((float)gt[j] + gr);
                const float z = sigmoidf((float)gt[Hp + j] + gz);
                const float n = fast_tanh((float)gt[2 * Hp + j] + r * hn);
                // (1 - z) * n + z * h with the product z * h fused into the
                // add. Spelled out because the contraction was the
                // compiler's choice and did not survive this body being
                // inlined into two kernels; this is the rounding the
                // batch-1 kernel has always had.
                const float hnew = __builtin_fmaf(z, hreg[i], (1.0f - z) * n);
                hreg[i] = hnew;
                const __bf16 hb = (__bf16)__float2bfloat16(hnew);
                hw[j] = hb;
                ((__bf16*)out_b)[(long)tt * out_trow + j] = hb;
            }
        }
        // raw barrier + lgkm-only wait: __syncthreads would also drain
        // vmcnt and stall every step on the out stores' retirement
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    if ((lane >> 4) == 0) {
        float* hl = hlast + hl_off;
#pragma unroll
        for (int i = 0; i < CPW; ++i)
            hl[(wave + NW * i) * 16 + lane] = hreg[i];
    }
}

template <int Hp, int NT>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT),
                          amdgpu_waves_per_eu(1, 1)))
void gru_fwd_b1_kernel(const __hip_bfloat16* __restrict__ gi,
                       const __hip_bfloat16* __restrict__ w,
                       const float* __restrict__ bhh,
                       __hip_bfloat16* __restrict__ out,
                       float* __restrict__ hlast, int Tseq, int n_dir,
                       const float* __restrict__ h0) {
    gru_fwd_b1_body<Hp, NT>(gi, w, bhh, out, hlast, Tseq, n_dir, h0,
                            (long)blockIdx.x * Hp);   // (n_dir, B=1, Hp)
}

// S independent sequences side by side (the fleet predict path): block
// (d, s) is the batch-1 block for direction d on stream s's slab of
// gi (S, T, n_dir*3Hp) and out (S, T, n_dir*Hp); hlast is (n_dir, S, Hp),
// the layout pool_concat_infer reads for B = S. Zero h0. Blocks share
// nothing, so up to one block per CU the S streams run in the latency of
// one.
template <int Hp, int NT>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT),
                          amdgpu_waves_per_eu(1, 1)))
void gru_fwd_streams_kernel(const __hip_bfloat16* __restrict__ gi,
                            const __hip_bfloat16* __restrict__ w,
                            const float* __restrict__ bhh,
                            __hip_bfloat16* __restrict__ out,
                            float* __restrict__ hlast, int Tseq, int n_dir) {
    const long dir = blockIdx.x;
    const long s = blockIdx.y;
    const long S = gridDim.y;
    gru_fwd_b1_body<Hp, NT>(
        gi + s * Tseq * n_dir * 3 * Hp, w, bhh, out + s * Tseq * n_dir * Hp,
        hlast, Tseq, n_dir, nullptr, (dir * S + s) * Hp);
}

// A per-stream slot index into a bank of M models, read on the device so a
// captured graph follows it between replays. Clamped into [0, M): a bad
// index reads another model's weights, never memory outside the bank (the
// host rejects bad indices before it writes them).
FMDA_DEV long bank_slot(const int* __restrict__ slot, long s, int M) {
    const int m = slot[s];
    return m < 0 ? 0 : (m >= M ? M - 1 : m);
}

// gru_fwd_streams over a bank of models: w is (M, n_dir, 3Hp, Hp), bhh
// (M, n_dir, 3Hp), and block (d, s) runs the unchanged batch-1 body on the
// W_hh / b_hh of slot[s]. Same grid, LDS and output layouts as
// gru_fwd_streams_kernel; the body loads its own fragments per block, so
// the bank costs one index load.
template <int Hp, int NT>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT),
                          amdgpu_waves_per_eu(1, 1)))
void gru_fwd_streams_bank_kernel(const __hip_bfloat16* __restrict__ gi,
                                 const int* __restrict__ slot, int M,
                                 const __hip_bfloat16* __restrict__ w,
                                 const float* __restrict__ bhh,
                                 __hip_bfloat16* __restrict__ out,
                                 float* __restrict__ hlast, int Tseq,
                                 int n_dir) {
    const long dir = blockIdx.x;
    const long s = blockIdx.y;
    const long S = gridDim.y;
    const long m = bank_slot(slot, s, M);
    gru_fwd_b1_body<Hp, NT>(
        gi + s * Tseq * n_dir * 3 * Hp, w + m * n_dir * 3 * Hp * Hp,
        bhh + m * n_dir * 3 * Hp, out + s * Tseq * n_dir * Hp,
        hlast, Tseq, n_dir, nullptr, (dir * S + s) * Hp);
}

// ---------------------------------------------------------------------------
// Grouped input projection over a bank of models:
//   gi[s] = x[s] @ W[slot[s]]^T + b[slot[s]]
// x (S, T, K), W (M, N, K), b (M, N), gi (S, T, N), all bf16. One launch
// covers every stream; the library GEMM it replaces takes one W.
//
// Both operands are K-contiguous, which is the per-lane order of the MFMA
// A and B fragments (8 consecutive k per lane), so fragments load straight
// from global memory and the kernel uses no LDS. W is the A operand and x
// the B operand: the accumulator then holds gi^T, lane l owning 4
// consecutive n of ONE time row, which it rounds once and writes with one
// 8-byte store. A wave owns a 64-column x 32-row tile of one stream's gi:
// per k-step four W fragments and two x fragments feed eight MFMAs, and
// two k-steps of loads are in flight before their MFMAs (a 16 x 32 tile
// with one step in flight measured 24.9 us per launch at S = 64, T = 120,
// bound by fragment traffic: profiles/fleet_bank.md). Grid (ceil(N/256),
// S, row tiles), 4 waves per block. Every output element is the same
// K/32-step MFMA chain whatever its stream, slot or tile, so streams are
// independent bit for bit.
//
// VEC is the widest load the row pitch 2*K bytes keeps aligned: 8 elements
// (16 bytes) when K % 8 == 0, 4 when K % 4 == 0 (K = 108: rows are only
// 8-byte aligned), else single elements. Elements at k >= K and rows at
// t >= T are zero in the fragment and are not read.
// ---------------------------------------------------------------------------
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));

template <int VEC>
FMDA_DEV bf16x8_t load_krow_frag(const __bf16* __restrict__ row, int k0,
                                 int K) {
    bf16x8_t f;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (__bf16)0.0f;
    if constexpr (VEC == 8) {
        if (k0 < K) f = *(const bf16x8_t*)(row + k0);
    } else if constexpr (VEC == 4) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (k0 + 4 * h < K) {
                const bf16x4_t v = *(const bf16x4_t*)(row + k0 + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) f[4 * h + e] = v[e];
            }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (k0 + e < K) f[e] = row[k0 + e];
    }
    return f;
}

template <int VEC>
__global__ __launch_bounds__(256)
void gi_proj_bank_kernel(const __hip_bfloat16* __restrict__ x,
                         const int* __restrict__ slot,
                         const __hip_bfloat16* __restrict__ W,
                         const __hip_bfloat16* __restrict__ b,
                         __hip_bfloat16* __restrict__ gi, int Tseq, int K,
                         int N, int M) {
    constexpr int KU = 2;        // k-steps of loads in flight
    constexpr int NTW = 4;       // 16-column tiles of N per wave
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int nw = (blockIdx.x * 4 + wave) * NTW * 16;   // first column
    if (nw >= N) return;                         // no barriers below
    const long s = blockIdx.y;
    const long m = bank_slot(slot, s, M);
    const int r16 = lane & 15;
    const int kl = 8 * (lane >> 4);
    const int q4 = 4 * (lane >> 4);              // this lane's 4 columns

    const __bf16* xs = (const __bf16*)x + s * Tseq * K;
    // N is a multiple of 16, not of 64: a tile past N loads and stores
    // nothing (Kw = 0 zero-fills its fragments); wave-uniform
    const __bf16* wrow[NTW];
    int Kw[NTW];
    float bias[NTW][4];
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        const int nt = nw + 16 * i;
        const bool ok = nt < N;
        Kw[i] = ok ? K : 0;
        wrow[i] = (const __bf16*)W + (m * N + (ok ? nt + r16 : 0)) * K;
#pragma unroll
        for (int v = 0; v < 4; ++v)
            bias[i][v] = ok ? (float)((const __bf16*)b)[m * N + (ok ? nt : 0)
                                                        + q4 + v]
                            : 0.0f;
    }

    {
        const int t0 = blockIdx.z * 32;          // < Tseq by the grid
        const bool two = t0 + 16 < Tseq;         // wave-uniform
        const int ta = t0 + r16, tb = ta + 16;
        const int Ka = ta < Tseq ? K : 0, Kb = tb < Tseq ? K : 0;
        const __bf16* xa = xs + (long)(ta < Tseq ? ta : Tseq - 1) * K;
        const __bf16* xb = xs + (long)(tb < Tseq ? tb : Tseq - 1) * K;
        f32x4_t acc[NTW][2];
#pragma unroll
        for (int i = 0; i < NTW; ++i)
            acc[i][0] = acc[i][1] = f32x4_t{0.f};
        // KU k-steps of loads in flight before their MFMAs
        for (int kb = 0; kb < K; kb += 32 * KU) {
            bf16x8_t wf[KU][NTW], fa[KU], fb[KU];
#pragma unroll
            for (int j = 0; j < KU; ++j) {
                const int k0 = kb + 32 * j + kl;
#pragma unroll
                for (int i = 0; i < NTW; ++i)
                    wf[j][i] = load_krow_frag<VEC>(wrow[i], k0, Kw[i]);
                fa[j] = load_krow_frag<VEC>(xa, k0, Ka);
                fb[j] = load_krow_frag<VEC>(xb, k0, Kb);
            }
#pragma unroll
            for (int j = 0; j < KU; ++j) {
                if (kb + 32 * j >= K) break;     // wave-uniform
#pragma unroll
                for (int i = 0; i < NTW; ++i) {
                    acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        wf[j][i], fa[j], acc[i][0], 0, 0, 0);
                    if (two)
                        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            wf[j][i], fb[j], acc[i][1], 0, 0, 0);
                }
            }
        }
        // C[row = n][col = t]: lane l holds 4 consecutive n of time row
        // t0 + l%16 (and of t0 + 16 + l%16)
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            if (nw + 16 * i >= N) break;         // wave-uniform
            __bf16* gs = (__bf16*)gi + s * Tseq * N + nw + 16 * i + q4;
            if (ta < Tseq) {
                bf16x4_t o;
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    o[v] = (__bf16)__float2bfloat16(acc[i][0][v] +
                                                    bias[i][v]);
                *(bf16x4_t*)(gs + (long)ta * N) = o;
            }
            if (tb < Tseq) {
                bf16x4_t o;
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    o[v] = (__bf16)__float2bfloat16(acc[i][1][v] +
                                                    bias[i][v]);
                *(bf16x4_t*)(gs + (long)tb * N) = o;
            }
        }
    }
}

// Exact exchanges inside aligned groups of 8 lanes: lane l receives the
// operand of lane l ^ 4 (ds_swizzle, bit-mask mode: and 0x1F, or 0, xor 4),
// l ^ 2 (DPP quad_perm [2,3,0,1]) or l ^ 1 (DPP quad_perm [1,0,3,2]). All
// lanes of the wave must be active.
FMDA_DEV unsigned int lane_xor4(unsigned int v) {
    return (unsigned int)__builtin_amdgcn_ds_swizzle((int)v, 0x101F);
}
FMDA_DEV unsigned int lane_xor2(unsigned int v) {
    return (unsigned int)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);
}
FMDA_DEV unsigned int lane_xor1(unsigned int v) {
    return (unsigned int)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}

// 8 x 8 byte transpose across an aligned group of 8 lanes: lane k (= lane
// & 7) passes the 8 bytes of x_k; on return byte c of lane l's value is byte
// l of x_c. Three butterfly stages, each swapping one lane bit with one
// byte-index bit (dword, 16-bit half, byte): one cross-lane move per stage.
FMDA_DEV unsigned long long transpose_bytes8(unsigned long long x, int lane) {
    unsigned int lo = (unsigned int)x, hi = (unsigned int)(x >> 32);
    const bool l2 = (lane & 4) != 0, l1 = (lane & 2) != 0,
               l0 = (lane & 1) != 0;
    unsigned int r = lane_xor4(l2 ? lo : hi);
    if (l2) lo = r; else hi = r;
    r = lane_xor2(l1 ? ((lo & 0xFFFFu) | (hi << 16))
                     : ((lo >> 16) | (hi & 0xFFFF0000u)));
    if (l1) {
        lo = (lo & 0xFFFF0000u) | (r & 0xFFFFu);
        hi = (hi & 0xFFFF0000u) | (r >> 16);
    } else {
        lo = (lo & 0xFFFFu) | (r << 16);
        hi = (hi & 0xFFFFu) | (r & 0xFFFF0000u);
    }
    // v_perm_b32 selectors: bytes 0..3 index the second operand, 4..7 the
    // first. Odd lanes hand over their even bytes, even lanes their odd ones.
    r = lane_xor1(__builtin_amdgcn_perm(hi, lo,
                                        l0 ? 0x06040200u : 0x07050301u));
    const unsigned int nlo =
        __builtin_amdgcn_perm(r, lo, l0 ? 0x03050104u : 0x05020400u);
    const unsigned int nhi =
        __builtin_amdgcn_perm(r, hi, l0 ? 0x03070106u : 0x07020600u);
    return ((unsigned long long)nhi << 32) | nlo;
}

// store_tile with the per-thread addressing formed by the caller, once: chunk
// n of the thread sits at LDS byte `n * NT * 16 + (PAD ? r16[n] : 0)` past
// `lds` (which already includes tid * 16) and goes to `gp + goff[n]`; its row
// is live when r16[n] < rv16 (= rows_valid * 16). A full block issues the
// tile's LDS reads together and then its stores, with no predicate; the
// tail block predicates each chunk as store_tile does. `__restrict__` as in
// store_tile: the tile read here is never a target of an LDS DMA in flight.
template <int SPT, int NT, bool PAD>
FMDA_DEV void store_tile_pre(const char* __restrict__ lds,
                             char* __restrict__ gp,
                             const unsigned int (&goff)[SPT],
                             const unsigned int (&r16)[SPT],
                             unsigned int rv16, bool full) {
    if (full) {
        typedef unsigned int st_u32x4 __attribute__((ext_vector_type(4)));
        static_assert(SPT == 3, "the pin below names three chunks");
        st_u32x4 v[SPT];
#pragma unroll
        for (int n = 0; n < SPT; ++n)
            v[n] = *(const st_u32x4*)(lds + n * NT * 16 +
                                      (PAD ? r16[n] : 0u));
        // pin all three reads ahead of the first store (the empty asm needs
        // every value): one LDS round trip per tile instead of one per chunk
        asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]));
#pragma unroll
        for (int n = 0; n < SPT; ++n) *(st_u32x4*)(gp + goff[n]) = v[n];
    } else {
#pragma unroll
        for (int n = 0; n < SPT; ++n)
            if (r16[n] < rv16)
                *(chunk16*)(gp + goff[n]) = *(const chunk16*)(
                    lds + n * NT * 16 + (PAD ? r16[n] : 0u));
    }
}

// Dynamic LDS of gru_bwd_v3_kernel: the three-slot gi ring and the two h
// tiles (unpadded rows: lane-linear DMA images), the d_out region, the
// double-buffered dGh tile at the padded pitch GP3 (elements), b_hh. The
// d_out region is two d_out tiles (do0, do1) in the dense kernel; the pooled
// kernel keeps its (v0, v1) words in exactly that space (pv) and adds BT * Hp
// amax bytes (im) behind it.
template <int BT, int Hp, bool POOLED>
struct BwdV3Lds {
    static constexpr int GP = 3 * Hp;
    static constexpr int HROW = Hp * 2;      // h/dout tile row bytes
    static constexpr int GP3 = 3 * Hp + 8;
    static constexpr int gi0 = 0;
    static constexpr int gi1 = gi0 + 2 * BT * GP;
    static constexpr int gi2 = gi1 + 2 * BT * GP;
    static constexpr int hb0 = gi2 + 2 * BT * GP;
    static constexpr int hb1 = hb0 + BT * HROW;
    static constexpr int do0 = hb1 + BT * HROW;
    static constexpr int pv = do0;
    static constexpr int do1 = do0 + BT * HROW;
    static constexpr int im = do1 + BT * HROW;
    static constexpr int dgh0 = im + (POOLED ? BT * Hp : 0);
    static constexpr int dgh1 = dgh0 + 2 * BT * GP3;
    static constexpr int bhh = dgh1 + 2 * BT * GP3;
    static constexpr int bytes = bhh + 4 * 3 * Hp;
    static_assert(bytes <= LDS_CU_BYTES,
                  "backward tiles / pooled table do not fit the LDS");
};

// POOLED: the layer feeds pool_features_fwd and nothing else, so its d_out
// is never materialised. pool_features_bwd_kernel would write
//   d_out[b, t, d*H + j] = bf16(ga + (t == amax[b, j] ? gm : 0.0f))
// with ga = float(dfeat[b, 2H + j]) / (float)T, gm = float(dfeat[b, H + j])
// for both directions, and d_hlast[d, b, j] = float(dfeat[b, j]). Here the
// block builds, once, a table of (v0 = bf16(ga + 0.0f), v1 = bf16(ga + gm),
// amax as a byte: T <= 256) for its BT rows in the LDS that the two d_out
// tiles occupied, and every step picks v1 at t == amax and v0 elsewhere:
// the same bits, without the (B, T, D*H) write, its read back, and the
// glds_do DMA stream. dout / dhT are not read (the launcher passes null);
// dfeat / amax / dfeat_ld are not read when !POOLED. No dropout in this
// variant (the top layer never defers one): that branch is compiled out.
//
// Table layout: entry k of thread `tid` (k = (i * MT + m) * 4 + e, the
// thread's own C elements in the order phase B visits them) sits at word
// k * NT + tid of pv_s (v0 low half, v1 high half) and at byte e of word
// (i * MT + m) * NT + tid of im_s: consecutive lanes read consecutive
// words, and the offsets of k are immediates off one base register.
template <int BT, int Hp, int NT, int WPE, bool POOLED = false>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT),
                          amdgpu_waves_per_eu(WPE, WPE)))
void gru_bwd_v3_kernel(const __hip_bfloat16* __restrict__ gi,
                       const __hip_bfloat16* __restrict__ w,
                       const __hip_bfloat16* __restrict__ wt,
                       const float* __restrict__ bhh,
                       const __hip_bfloat16* __restrict__ out,
                       const __hip_bfloat16* __restrict__ dout,
                       const float* __restrict__ dhT,
                       __hip_bfloat16* __restrict__ dgi,
                       __hip_bfloat16* __restrict__ dgh, float* __restrict__ dh0,
                       float* __restrict__ dbhh, int B, int Tseq, int n_dir,
                       unsigned int drop_thr, float drop_scale,
                       unsigned long long drop_seed,
                       const float* __restrict__ h0,
                       __hip_bfloat16* __restrict__ dgh0,
                       const __hip_bfloat16* __restrict__ dfeat,
                       const int* __restrict__ amax, long dfeat_ld) {
    constexpr int NW = NT / 64;
    constexpr int MT = BT / 16;
    constexpr int NCT = Hp / 16;
    constexpr int CPW = NCT / NW;
    constexpr int KK = Hp / 32;
    constexpr int KK2 = (3 * Hp) / 32;
    using L = BwdV3Lds<BT, Hp, POOLED>;
    constexpr int GP = L::GP;
    constexpr int HROW = L::HROW;        // h/dout tile row bytes (unpadded)
    constexpr int GP3 = L::GP3;          // padded dgh_s pitch (MFMA A reads)
    constexpr int PW = (BT * GP * 2) / 1024 / NW;   // gi glds per wave
    constexpr int DOP = (BT * HROW) / 1024 / NW;    // dout glds per wave
    constexpr int HBP = DOP;                        // h glds per wave
    constexpr int NST = 2 * ((BT * GP * 2) / 16) / NT;  // dGi+dGh store instrs
    static_assert(NCT % NW == 0 && (BT * GP * 2) % (1024 * NW) == 0 &&
                  (BT * HROW) % (1024 * NW) == 0, "tiling mismatch");

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int b0 = blockIdx.x * BT;
    const int dir = blockIdx.y;
    const bool rev = (dir == 1);
    const int rows_valid = min(BT, B - b0);

    extern __shared__ __attribute__((aligned(16))) char smem[];
    // Plain pointers + select helpers, NOT runtime-indexed local arrays:
    // a dynamically indexed private pointer array lands in scratch, and
    // every scratch reload is an ordinary VMEM load that triggers the
    // glds vmcnt(0) drain (this alone cost 3x on this kernel).
    __hip_bfloat16* gi_s0 = (__hip_bfloat16*)(smem + L::gi0);
    __hip_bfloat16* gi_s1 = (__hip_bfloat16*)(smem + L::gi1);
    __hip_bfloat16* gi_s2 = (__hip_bfloat16*)(smem + L::gi2);
    __hip_bfloat16* hb_s0 = (__hip_bfloat16*)(smem + L::hb0);
    __hip_bfloat16* hb_s1 = (__hip_bfloat16*)(smem + L::hb1);
    __hip_bfloat16* do_s0 = (__hip_bfloat16*)(smem + L::do0);
    __hip_bfloat16* do_s1 = (__hip_bfloat16*)(smem + L::do1);
    unsigned int* pv_s = (unsigned int*)(smem + L::pv);
    unsigned int* im_s = (unsigned int*)(smem + L::im);
    __hip_bfloat16* dgh_s0 = (__hip_bfloat16*)(smem + L::dgh0);
    __hip_bfloat16* dgh_s1 = (__hip_bfloat16*)(smem + L::dgh1);
    float* bhh_s = (float*)(smem + L::bhh);
    auto dgh_buf = [&](int b) { return b ? dgh_s1 : dgh_s0; };
    auto gi_slot = [&](int sl) {
        return sl == 0 ? gi_s0 : (sl == 1 ? gi_s1 : gi_s2);
    };
    auto hb_buf = [&](int b) { return b ? hb_s1 : hb_s0; };
    auto do_buf = [&](int b) { return b ? do_s1 : do_s0; };

    const long gi_row = (long)Tseq * n_dir * 3 * Hp;
    const long out_row = (long)Tseq * n_dir * Hp;
    const __hip_bfloat16* gi_b = gi + (long)b0 * gi_row + (long)dir * 3 * Hp;
    __hip_bfloat16* dgi_b = dgi + (long)b0 * gi_row + (long)dir * 3 * Hp;
    __hip_bfloat16* dgh_b = dgh + (long)b0 * gi_row + (long)dir * 3 * Hp;
    const __hip_bfloat16* out_b = out + (long)b0 * out_row + (long)dir * Hp;
    const __hip_bfloat16* dout_b = dout + (long)b0 * out_row + (long)dir * Hp;

    for (int c = tid; c < 3 * Hp; c += NT)
        bhh_s[c] = bhh[(long)dir * 3 * Hp + c];

    if (POOLED) {
        // Table fill, before any glds like the loads below: one (row,
        // 8-column group) per thread and pass, three 16-byte dfeat loads
        // and two 16-byte amax loads per lane, scattered to the owners'
        // slots. ga, gm and the roundings are pool_features_bwd_kernel's
        // expressions (`+ 0.0f` turns a -0.0 average gradient into +0.0).
        // The bf16 d_hlast column goes to dgh_s0 in the same [k][tid]
        // order; nothing else touches dgh_s0 before the first phase B,
        // which runs after the prologue barrier below.
        constexpr int H8 = Hp / 8;
        unsigned short* gl_s = (unsigned short*)dgh_s0;
        for (int c = tid; c < BT * H8; c += NT) {
            const int b = c / H8;
            const int h8 = (c % H8) * 8;
            bf16x8_t dl, dm, da;
            int4 a0 = make_int4(0, 0, 0, 0), a1 = a0;
            const bool rowlive = (b < rows_valid);
            if (rowlive) {
                const __hip_bfloat16* dr =
                    dfeat + (long)(b0 + b) * dfeat_ld + h8;
                dl = *(const bf16x8_t*)dr;
                dm = *(const bf16x8_t*)(dr + Hp);
                da = *(const bf16x8_t*)(dr + 2 * Hp);
                const int* ai = amax + (long)(b0 + b) * Hp + h8;
                a0 = *(const int4*)ai;
                a1 = *(const int4*)(ai + 4);
            }
            const int imv[8] = {a0.x, a0.y, a0.z, a0.w,
                                a1.x, a1.y, a1.z, a1.w};
            // owner of (b, j): column tile ct = j / 16 -> wave ct % NW,
            // i = ct / NW; lane (j & 15) + 16 * ((b >> 2) & 3); m = b / 16;
            // e = b & 3 (the C layout of the MFMA, see phase B)
            const int ct = h8 >> 4;             // 8 columns: one column tile
            const int im0 = (ct / NW) * MT + (b >> 4);
            const int e = b & 3;
            const int t0 = (ct % NW) * 64 + 16 * ((b >> 2) & 3) + (h8 & 15);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                unsigned int pv = 0u, iv = 0u;
                unsigned short gl = 0;
                if (rowlive) {
                    const float ga = (float)da[k] / (float)Tseq;
                    const float gm = (float)dm[k];
                    const __bf16 v0 = (__bf16)__float2bfloat16(ga + 0.0f);
                    const __bf16 v1 = (__bf16)__float2bfloat16(ga + gm);
                    pv = (unsigned int)__builtin_bit_cast(unsigned short, v0) |
                         ((unsigned int)__builtin_bit_cast(unsigned short, v1)
                          << 16);
                    iv = (unsigned int)imv[k];
                    gl = __builtin_bit_cast(unsigned short, (__bf16)dl[k]);
                }
                pv_s[(im0 * 4 + e) * NT + t0 + k] = pv;
                ((unsigned char*)im_s)[(im0 * NT + t0 + k) * 4 + e] =
                    (unsigned char)iv;
                gl_s[(im0 * 4 + e) * NT + t0 + k] = gl;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    // Both W fragment sets, register-resident; loaded ONCE here (ordinary
    // loads are legal before any glds is issued).
    const __hip_bfloat16* wdir = w + (long)dir * 3 * Hp * Hp;
    const __hip_bfloat16* wt_dir = wt + (long)dir * Hp * 3 * Hp;
    bf16x8_t wA[CPW][3][KK];
    bf16x8_t wB[CPW][KK2];
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int ct = wave + NW * i;
        const int jcol = ct * 16 + (lane & 15);
        const __bf16* wtrow = (const __bf16*)wt_dir + (long)jcol * 3 * Hp;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                wA[i][g][kk] = load_wfragA<Hp>(wdir, Hp, ct, g, kk, lane);
#pragma unroll
        for (int kk = 0; kk < KK2; ++kk)
            wB[i][kk] = *(const bf16x8_t*)&wtrow[32 * kk + 8 * (lane >> 4)];
    }

    float dhreg[CPW][MT][4];   // dh carry (fp32, lane-owned)
    // 4 running sums: dr, dz, dhn (-> db_hh) and dn (-> db_ih; dr/dz are
    // shared between the two bias gradients).
    float dbacc[CPW][4];
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
#pragma unroll
        for (int g = 0; g < 4; ++g) dbacc[i][g] = 0.0f;
        const int ct = wave + NW * i;
        const int j = ct * 16 + (lane & 15);
        const float* hT = dhT + ((long)dir * B + b0) * Hp;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = 16 * m + 4 * (lane >> 4) + e;
                if (POOLED) {
                    // float(dfeat[b, j]) for both directions, as the pool
                    // backward wrote d_hlast; dead rows were filled with 0
                    const unsigned short gl = ((const unsigned short*)
                        dgh_s0)[((i * MT + m) * 4 + e) * NT + tid];
                    dhreg[i][m][e] = __uint_as_float((unsigned int)gl << 16);
                } else {
                    dhreg[i][m][e] =
                        (b < rows_valid) ? hT[(long)b * Hp + j] : 0.0f;
                }
            }
    }

    const int wavu = __builtin_amdgcn_readfirstlane(wave);
    auto glds_gi = [&](int tt, int sl) {
        const __hip_bfloat16* src_t = gi_b + (long)tt * n_dir * 3 * Hp;
        __hip_bfloat16* dst = gi_slot(sl);
#pragma unroll
        for (int k = 0; k < PW; ++k) {
            const int off = (wavu * PW + k) * 1024 + lane * 16;
            const int e = off >> 1;
            int r = e / GP;
            const int c = e % GP;
            if (r >= rows_valid) r = 0;
            glds16(src_t + (long)r * gi_row + c,
                   (char*)dst + (long)(wavu * PW + k) * 1024);
        }
    };
    auto glds_do = [&](int tt, int buf) {
        const __hip_bfloat16* src_t = dout_b + (long)tt * n_dir * Hp;
#pragma unroll
        for (int k = 0; k < DOP; ++k) {
            const int off = (wavu * DOP + k) * 1024 + lane * 16;
            const int e = off >> 1;
            int r = e / Hp;
            const int c = e % Hp;
            if (r >= rows_valid) r = 0;
            glds16(src_t + (long)r * out_row + c,
                   (char*)do_buf(buf) + (long)(wavu * DOP + k) * 1024);
        }
    };
    // XOR-swizzled source: LDS[r][k16] = out[r][k16 ^ (r & 15)] so the
    // MFMA A-fragment reads are bank-conflict-free at the unpadded pitch.
    auto glds_hb = [&](int tt, int buf) {
        const __hip_bfloat16* src_t = out_b + (long)tt * n_dir * Hp;
#pragma unroll
        for (int k = 0; k < HBP; ++k) {
            const int off = (wavu * HBP + k) * 1024 + lane * 16;
            int r = off / HROW;
            const int k16 = (off % HROW) >> 4;
            const int csrc = (k16 ^ (r & 15)) << 4;  // byte col in row
            if (r >= rows_valid) r = 0;
            glds16((const char*)(src_t + (long)r * out_row) + csrc,
                   (char*)hb_buf(buf) + (long)(wavu * HBP + k) * 1024);
        }
    };
    // Boundary h image: zeros, or h0 when an initial hidden state is given.
    // h0 goes in SWIZZLED (LDS[r][k16] = h[r][k16 ^ (r & 15)]) like the
    // glds_hb image so hb_read / the A-fragment reads see the same layout.
    // The h0 loads are ordinary VMEM loads; at the in-loop call site (u==1)
    // they cost one vmcnt(0) drain of that step's DMA — once per launch.
    auto zero_hb = [&](int buf) {
        if (h0 != nullptr) {
            const float* h0d = h0 + ((long)dir * B + b0) * Hp;
            char* dst = (char*)hb_buf(buf);
            for (int c = tid; c < BT * Hp; c += NT) {
                const int r = c / Hp, j = c % Hp;
                const float v =
                    (r < rows_valid) ? h0d[(long)r * Hp + j] : 0.0f;
                const int k16 = ((j * 2) >> 4) ^ (r & 15);
                *(__bf16*)(dst + r * HROW + k16 * 16 + ((j * 2) & 15)) =
                    (__bf16)__float2bfloat16(v);
            }
            return;
        }
        for (int c = tid; c < BT * Hp; c += NT)
            ((__bf16*)hb_buf(buf))[c] = (__bf16)0.0f;
    };
    // swizzled scalar read of h_prev[b][j]
    auto hb_read = [&](const __hip_bfloat16* hb, int b, int j) -> float {
        const int k16 = (j * 2) >> 4;           // 16B slot of column j
        const int ksw = k16 ^ (b & 15);
        const int within = (j * 2) & 15;
        return (float)*(const __bf16*)((const char*)hb + b * HROW +
                                       ksw * 16 + within);
    };

    // Fused-dropout mask, one draw per octet: the element at (b, tt, dir, j)
    // takes byte o & 7 of mix64(seed ^ (o >> 3)), o = ((b0 + b) * Tseq + tt)
    // * n_dir * Hp + dir * Hp + j. In the MFMA C layout j = ct * 16 +
    // (lane & 15) and n_dir * Hp, dir * Hp are multiples of 8, so o & 7 =
    // lane & 7 and, for each of the thread's 8 elements of a step, the 8
    // lanes of an aligned group share one octet. Lane k of the group hashes
    // the octet of element k = (i * MT + m) * 4 + e (the order phase B
    // visits them) and transpose_bytes8 hands every lane its byte of all 8
    // draws. oct0 is that octet at tt = 0; a step adds tt * n_dir * (Hp / 8).
    static_assert(Hp % 16 == 0, "octets must not straddle column tiles");
    static_assert(POOLED || CPW * MT * 4 == 8,
                  "the dropout exchange covers 8 elements per thread");
    const bool dropping = !POOLED && drop_thr != 0u;
    long oct0 = 0;
    if (dropping) {
        const int k = lane & 7;
        const int ik = k / (4 * MT), mk = (k >> 2) % MT, ek = k & 3;
        const int bk = 16 * mk + 4 * (lane >> 4) + ek;
        const int jk = (wave + NW * ik) * 16 + (lane & 15);
        oct0 = ((long)(b0 + bk) * Tseq * n_dir * Hp + (long)dir * Hp + jk) >> 3;
    }
    const long oct_step = (long)n_dir * (Hp / 8);

    // Step-invariant addressing of the one-step-late dGi / dGh tile stores:
    // chunk c = tid + n * NT of a tile sits in row r = c / CPR at chunk
    // c % CPR, for both tiles (same global layout). Its byte offset from
    // the tile's (uniform) time-step base and r * 16 (the dgh_s pad; also
    // the rows_valid predicate) are formed once here; the gi tile's LDS
    // offset is c * 16, the padded dgh tile's c * 16 + r * 16. 32-bit
    // offsets when a block's BT rows span less than 2 GiB, else store_tile.
    constexpr int SPT = NST / 2;                 // chunks per thread and tile
    constexpr int CPR = (GP * 2) / 16;           // 16-byte chunks per row
    static_assert(SPT * NT == BT * CPR && GP3 * 2 == CPR * 16 + 16,
                  "store addressing mismatch");
    const bool st_fast = (long)BT * gi_row * 2 < (1L << 31);
    unsigned int st_goff[SPT], st_r16[SPT];
#pragma unroll
    for (int n = 0; n < SPT; ++n) {
        const int c = tid + n * NT;
        const int r = c / CPR;
        st_goff[n] = (unsigned int)r * (unsigned int)(gi_row * 2) +
                     (unsigned int)(c % CPR) * 16u;
        st_r16[n] = (unsigned int)r * 16u;
    }
    const unsigned int rv16 = (unsigned int)rows_valid * 16u;

    {   // prologue: stage step Tseq-1 inputs
        const int u = Tseq - 1;
        const int tt = rev ? 0 : u;
        glds_gi(tt, u % 3);
        if (!POOLED) glds_do(tt, u & 1);
        if (u > 0) {
            const int ttp = rev ? 1 : (u - 1);
            glds_hb(ttp, u & 1);
        } else {
            zero_hb(u & 1);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    for (int u = Tseq - 1; u >= 0; --u) {
        const int q = u & 1;
        const int slot = u % 3;
        const int tt = rev ? (Tseq - 1 - u) : u;
        const bool have_next = (u > 0);
        const bool have_prev = (u + 1 < Tseq);  // a step was processed before

        // ---- phase A: DMA issues, then one-step-late stores ----
        if (have_next) {
            const int ttn = rev ? (Tseq - u) : (u - 1);
            glds_gi(ttn, (u - 1) % 3);
            if (!POOLED) glds_do(ttn, 1 - q);
            if (u >= 2)
                glds_hb(rev ? (Tseq + 1 - u) : (u - 2), 1 - q);
            else
                zero_hb(1 - q);
        }
        if (have_prev) {
            // one-step-late stores; dgh_s is double-buffered so these
            // reads never race phase B's writes and no A-end barrier is
            // needed (the single per-step barrier is at B-end, where it
            // also rendezvouses this step's DMA).
            const int ttp = rev ? (Tseq - 2 - u) : (u + 1);
            const int sh = rev ? (ttp + 1) : (ttp - 1);  // always in range
            if (st_fast) {
                // only the two uniform bases depend on the step
                store_tile_pre<SPT, NT, false>(
                    (const char*)gi_slot((u + 1) % 3) + tid * 16,
                    (char*)(dgi_b + (long)ttp * n_dir * 3 * Hp), st_goff,
                    st_r16, rv16, rows_valid == BT);
                store_tile_pre<SPT, NT, true>(
                    (const char*)dgh_buf(1 - q) + tid * 16,
                    (char*)(dgh_b + (long)sh * n_dir * 3 * Hp), st_goff,
                    st_r16, rv16, rows_valid == BT);
            } else {
                store_tile<__hip_bfloat16, BT, NT>(
                    gi_slot((u + 1) % 3), dgi_b + (long)ttp * n_dir * 3 * Hp,
                    GP, GP, gi_row, rows_valid, tid);
                store_tile<__hip_bfloat16, BT, NT>(
                    dgh_buf(1 - q), dgh_b + (long)sh * n_dir * 3 * Hp, GP,
                    GP3, gi_row, rows_valid, tid);
            }
        }

        // this step's 8 mask bytes (byte k: element k), off the gate chain
        unsigned long long dmask = 0ull;
        if (dropping)
            dmask = transpose_bytes8(
                mix64(drop_seed ^
                      (unsigned long long)(oct0 + (long)tt * oct_step)),
                lane);

        // ---- phase B: recompute GEMM, then fused gate gradients ----
        const __hip_bfloat16* hbq = hb_buf(q);
        f32x4_t acc[CPW][3][MT];
#pragma unroll
        for (int i = 0; i < CPW; ++i)
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[i][g][m] = f32x4_t{0.f};
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            const int arow = lane & 15;
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                bf16x8_t a[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const int row = 16 * m + arow;
                    const int k16 = (4 * kk + (lane >> 4)) ^ (row & 15);
                    a[m] = *(const bf16x8_t*)((const char*)hbq +
                                              row * HROW + k16 * 16);
                }
#pragma unroll
                for (int g = 0; g < 3; ++g)
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        acc[i][g][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            a[m], wA[i][g][kk], acc[i][g][m], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            const int ct = wave + NW * i;
            const int j = ct * 16 + (lane & 15);
            __bf16* grow = (__bf16*)gi_slot(slot);
            __bf16* dgrow = (__bf16*)dgh_buf(q);
            const __bf16* dorow = (const __bf16*)do_buf(q);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                // this thread's four amax bytes of (i, m); read every step
                // like the (v0, v1) words below (the table stays in LDS:
                // the kernel has no registers to spare for it)
                unsigned int imw = 0u;
                if (POOLED) imw = im_s[(i * MT + m) * NT + tid];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * m + 4 * (lane >> 4) + e;
                    const bool live = (b < rows_valid);
                    const float gr = acc[i][0][m][e] + bhh_s[j];
                    const float gz = acc[i][1][m][e] + bhh_s[Hp + j];
                    const float hn = acc[i][2][m][e] + bhh_s[2 * Hp + j];
                    const float ir = (float)grow[b * GP + j];
                    const float iz = (float)grow[b * GP + Hp + j];
                    const float in_ = (float)grow[b * GP + 2 * Hp + j];
                    const float r = sigmoidf(ir + gr);
                    const float z = sigmoidf(iz + gz);
                    const float n = fast_tanh(in_ + r * hn);
                    const float hprev = hb_read(hbq, b, j);
                    float doval;
                    if (POOLED) {
                        const unsigned int pv =
                            pv_s[((i * MT + m) * 4 + e) * NT + tid];
                        const int im = (int)((imw >> (8 * e)) & 0xFFu);
                        // bf16 -> fp32: v1 is the high half already
                        const unsigned int bits =
                            (tt == im) ? (pv & 0xFFFF0000u) : (pv << 16);
                        doval = live ? __uint_as_float(bits) : 0.0f;
                    } else {
                        doval = live ? (float)dorow[b * Hp + j] : 0.0f;
                    }
                    if (!POOLED && drop_thr != 0u) {
                        // fused inter-layer dropout backward: dout is the
                        // grad w.r.t. the DROPPED activations; recompute
                        // the counter-based mask (same splitmix64 draw as
                        // dropout_kernel) instead of a separate 1 GB
                        // read+write pass over d_out. dmask holds this
                        // element's byte of its octet's draw (see oct0).
                        const unsigned int u =
                            (unsigned int)(dmask >>
                                           (8 * ((i * MT + m) * 4 + e))) &
                            0xFF;
                        doval = (u < drop_thr) ? 0.0f : doval * drop_scale;
                    }
                    const float dht = dhreg[i][m][e] + doval;
                    // live-gating every product: 0 * inf = NaN would leak
                    // into dbacc from uninitialized dead-row LDS.
                    const float dz_pre =
                        live ? dht * (hprev - n) * z * (1.0f - z) : 0.0f;
                    const float dn_pre =
                        live ? dht * (1.0f - z) * (1.0f - n * n) : 0.0f;
                    const float dr_pre =
                        live ? dn_pre * hn * r * (1.0f - r) : 0.0f;
                    const float dhn = live ? dn_pre * r : 0.0f;
                    grow[b * GP + j] = (__bf16)__float2bfloat16(dr_pre);
                    grow[b * GP + Hp + j] = (__bf16)__float2bfloat16(dz_pre);
                    grow[b * GP + 2 * Hp + j] =
                        (__bf16)__float2bfloat16(dn_pre);
                    dgrow[b * GP3 + j] = (__bf16)__float2bfloat16(dr_pre);
                    dgrow[b * GP3 + Hp + j] = (__bf16)__float2bfloat16(dz_pre);
                    dgrow[b * GP3 + 2 * Hp + j] =
                        (__bf16)__float2bfloat16(dhn);
                    dhreg[i][m][e] = live ? dht * z : 0.0f;
                    dbacc[i][0] += dr_pre;
                    dbacc[i][1] += dz_pre;
                    dbacc[i][2] += dhn;
                    dbacc[i][3] += dn_pre;
                }
            }
        }
        // single per-step barrier: publishes dgh_s[q] for phase C AND
        // rendezvouses this step's DMA (tiles for step u-1, read at
        // B(u-1)), leaving the trailing dGi/dGh stores in flight. The
        // counted form assumes every thread issued its full store quota;
        // in the (single) batch-tail block dead rows skip stores, so that
        // block full-drains instead — exactness over speed there.
        // POOLED: a thread's vector-memory operations of a step are, in
        // program order, the gi DMAs, the h DMA (or zero_hb's h0 loads)
        // and then the NST tile stores; the variant only takes the d_out
        // DMA out from between them, and its table reads are LDS traffic
        // (lgkmcnt). The NST stores are therefore still the youngest NST
        // operations of every thread of a full block, vmcnt(NST) still
        // means "every DMA of this step has landed", and the tail block
        // still drains to zero.
        // store_tile_pre issues the same NST stores as the two store_tile
        // calls it stands in for (unpredicated in a full block, SPT per
        // tile), after the DMAs and with LDS reads only in between; the
        // dropout mask's hash and lane exchange (DPP, ds_swizzle: lgkmcnt)
        // add no vector-memory operation. The quota and the order hold.
        if (have_next) {
            if (have_prev && rows_valid == BT)
                asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NST) : "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();

        // ---- phase C: carry GEMM dh += dGh W — registers + LDS only ----
        {
            f32x4_t acc2[CPW][MT];
#pragma unroll
            for (int i = 0; i < CPW; ++i)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc2[i][m] = f32x4_t{0.f};
#pragma unroll
            for (int i = 0; i < CPW; ++i) {
                const int arow = lane & 15;
                const int koff = 8 * (lane >> 4);
#pragma unroll
                for (int kk = 0; kk < KK2; ++kk) {
                    const int kbase = 32 * kk + koff;
                    bf16x8_t a[MT];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        a[m] = *(const bf16x8_t*)&((const __bf16*)
                                   dgh_buf(q))[(16 * m + arow) * GP3 + kbase];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        acc2[i][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            a[m], wB[i][kk], acc2[i][m], 0, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < CPW; ++i)
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        dhreg[i][m][e] += acc2[i][m][e];
        }
        // no barrier: the next step's A-end rendezvous orders everything.
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    {   // epilogue: last dGi store, boundary zero dGh slot, dh0, db_hh
        const int ttl = rev ? (Tseq - 1) : 0;
        store_tile<__hip_bfloat16, BT, NT>(
            gi_s0, dgi_b + (long)ttl * n_dir * 3 * Hp, GP, GP, gi_row,
            rows_valid, tid);
        // step u=0's dGh pairs with h_{-1}: its global slot (rev ? 0 :
        // Tseq-1) gets zeros (the dW_hh reduction pairs slots with out[t]);
        // with an initial hidden state the values go to dgh0 so the host
        // adds the dGh_0 (x) h0 term to dW_hh.
        store_zero_tile<__hip_bfloat16, BT, NT>(
            dgh_b + (long)(rev ? 0 : (Tseq - 1)) * n_dir * 3 * Hp, GP, gi_row,
            rows_valid, tid);
        if (dgh0 != nullptr)
            store_tile<__hip_bfloat16, BT, NT>(
                dgh_s0, dgh0 + ((long)dir * B + b0) * GP, GP, GP3, GP,
                rows_valid, tid);
        float* d0 = dh0 + ((long)dir * B + b0) * Hp;
#pragma unroll
        for (int i = 0; i < CPW; ++i) {
            const int ct = wave + NW * i;
            const int j = ct * 16 + (lane & 15);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * m + 4 * (lane >> 4) + e;
                    if (b < rows_valid) d0[(long)b * Hp + j] = dhreg[i][m][e];
                }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                // one store into this batch tile's row of the partials
                // table (batch tile, n_dir, 4Hp); the host sums the tiles
                // in a fixed order (bitwise reproducible, unlike a float
                // atomicAdd across blocks). Row layout (n_dir, 4Hp):
                // [dr, dz, dhn | dn] — db_hh = slots 0..2, db_ih = slots
                // 0,1,3 (assembled host-side).
                float v = dbacc[i][g];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if ((lane >> 4) == 0)
                    dbhh[((long)blockIdx.x * n_dir + dir) * 4 * Hp + g * Hp +
                         ct * 16 + (lane & 15)] = v;
            }
        }
    }
}


// ===========================================================================
// Column-split persistent forward for LARGE hidden sizes (Hp = 512).
//
// At H = 512 the batch-parallel kernels above starve the chip (W_hh is
// 1.5 MB/direction — far past LDS and the register file — so every block
// re-streams it from L2 each step, and B/BT blocks can't fill 256 CUs).
// This kernel splits the HIDDEN dimension instead (SURVEY.md section 7
// "hard part (a)"): a GROUP of CT=16 column-blocks owns one (batch-rows,
// direction) pair; each block keeps its 96-gate-row slice of W_hh
// row-major in LDS (~98 KB, read as contiguous MFMA B-fragments) and owns
// 32 h columns. Per timestep every block:
//   1. polls the group's monotonic arrival counter (relaxed agent load)
//      until all CT slices of h_{t-1} are published,
//   2. MFMA-multiplies the FULL h_{t-1} (asm sc1 b128 loads from the
//      publication ring — sc1 both sides is the placement-independent
//      visibility recipe; block->XCD placement is speed-only),
//   3. fuses the gates for its 32 columns (own h carried in fp32 regs),
//   4. publishes h_t: LDS stage -> cooperative 16-B sc1 stores ->
//      s_waitcnt vmcnt(0) -> one relaxed agent atomicAdd per block.
// The 2-deep publication ring is safe because the counter bounds block
// skew to one step: a block enters step t only after every peer published
// t-1, so nobody can overwrite a slot a peer still reads.
// gi tiles stage through LDS one step ahead (ordinary loads; this kernel
// has NO LDS-DMA, so the ROCm 7.2 glds/ordinary-load drain hazard does
// not apply).
// ===========================================================================

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// Dynamic LDS of gru_fwd_cs_kernel and gru_bwd_cs_kernel (byte offsets): the
// block's W_hh slice (3CS rows at the padded pitch WPITCH, elements), the
// (BR, GP) gi tile that also stages the published strips, the block's b_hh.
template <int BR, int Hp, int CS>
struct CsLds {
    static constexpr int WPITCH = Hp + 8;
    static constexpr int GP = 3 * CS;
    static constexpr int w = 0;
    static constexpr int gi = w + 2 * 3 * CS * WPITCH;
    static constexpr int bhh = gi + 2 * BR * GP;
    static constexpr int bytes = bhh + 4 * 3 * CS;
    static_assert(bytes <= LDS_CU_BYTES,
                  "column-split tiles do not fit the LDS");
};

FMDA_DEV void store16_sc1(void* p, u32x4_t v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\ns_nop 1"
                 :: "v"(p), "v"(v) : "memory");
}

template <int BR, int Hp, int CS, int NT>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT),
                          amdgpu_waves_per_eu(2, 2)))
void gru_fwd_cs_kernel(const __hip_bfloat16* __restrict__ gi,
                       const __hip_bfloat16* __restrict__ w,
                       const float* __restrict__ bhh,
                       __hip_bfloat16* __restrict__ out,
                       float* __restrict__ hlast,
                       __hip_bfloat16* __restrict__ hpub,  // (2,G,BR,Hp)
                       unsigned int* __restrict__ cnt,     // (G)
                       int B, int Tseq, int n_dir, int GB,
                       __hip_bfloat16* __restrict__ out_drop,
                       unsigned int drop_thr, float drop_scale,
                       unsigned long long drop_seed, long gi_pitch) {
    constexpr int CT = Hp / CS;          // column-blocks per group
    constexpr int NW = NT / 64;          // waves
    constexpr int MT = BR / 16 / NW;     // m-tiles per wave
    constexpr int NCT = 3 * CS / 16;     // gate-column tiles (all per wave)
    constexpr int KK = Hp / 32;
    constexpr int WPITCH = CsLds<BR, Hp, CS>::WPITCH;  // W slice LDS pitch
    constexpr int GP = CsLds<BR, Hp, CS>::GP;          // gi tile pitch
    static_assert(BR % (16 * NW) == 0, "rows must tile");

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    // id -> (group, member): member-major within an XCD (id % 8 observed
    // = XCD) so one group's 16 members share an L2. Speed-only.
    const int id = blockIdx.x;
    const int nG = GB * n_dir;
    const int xcd = id % 8;
    const int slot_in_xcd = id / 8;
    int g, ct;
    if (nG >= 8 && (nG % 8) == 0) {
        ct = slot_in_xcd % CT;
        g = xcd + 8 * (slot_in_xcd / CT);
    } else {                              // small grids: plain mapping
        g = id / CT;
        ct = id % CT;
    }
    const int dir = g / GB;
    const int gb = g % GB;
    const bool rev = (dir == 1);
    const int b0 = gb * BR;
    const int rows_valid = min(BR, B - b0);

    extern __shared__ __attribute__((aligned(16))) char smem[];
    using L = CsLds<BR, Hp, CS>;
    __hip_bfloat16* w_s = (__hip_bfloat16*)(smem + L::w);    // (3CS, WPITCH)
    __hip_bfloat16* gi_s = (__hip_bfloat16*)(smem + L::gi);  // also h stage
    float* bhh_s = (float*)(smem + L::bhh);

    const long gi_row = gi_pitch;   // elements between batch rows of gi
    const long out_row = (long)Tseq * n_dir * Hp;
    // this block's gate rows: dir block, gate gslices at ct*CS
    const __hip_bfloat16* wdir = w + (long)dir * 3 * Hp * Hp;
    for (int g3 = 0; g3 < 3; ++g3) {
        stage_tile<__hip_bfloat16, CS, NT>(
            w_s + g3 * CS * WPITCH, wdir + (long)(g3 * Hp + ct * CS) * Hp,
            Hp, WPITCH, Hp, CS, tid);
        for (int c = tid; c < CS; c += NT)
            bhh_s[g3 * CS + c] = bhh[(long)dir * 3 * Hp + g3 * Hp + ct * CS + c];
    }

    const __hip_bfloat16* gi_b =
        gi + (long)b0 * gi_row + (long)dir * 3 * Hp;
    __hip_bfloat16* out_b = out + (long)b0 * out_row + (long)dir * Hp;
    __hip_bfloat16* pub_base = hpub + (long)g * BR * Hp;   // + ring*G*BR*Hp
    const long ring_stride = (long)nG * BR * Hp;

    // stage gi tile for step tt into gi_s (this block's 3*CS gate columns,
    // in r|z|n blocks of CS)
    auto stage_gi = [&](int tt) {
        const __hip_bfloat16* src =
            gi_b + (long)tt * n_dir * 3 * Hp;
        for (int g3 = 0; g3 < 3; ++g3)
            stage_tile<__hip_bfloat16, BR, NT>(
                gi_s + g3 * CS, src + g3 * Hp + ct * CS, CS, GP,
                gi_row, rows_valid, tid);
    };

    // own h (fp32) carried in registers: lane owns (b, jj) for its C tiles
    float hreg[NCT / 3][MT][4];   // jj tiles per gate = CS/16 = NCT/3
    constexpr int JT = CS / 16;
#pragma unroll
    for (int i = 0; i < JT; ++i)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int e = 0; e < 4; ++e) hreg[i][m][e] = 0.0f;

    {   // prologue: publish h_{-1} = 0 into ring slot 0; stage gi(step 0)
        stage_gi(rev ? (Tseq - 1) : 0);
        __hip_bfloat16* dst = pub_base;            // ring slot 0
        const u32x4_t z = {0, 0, 0, 0};
        for (int c = tid; c < BR * CS * 2 / 16; c += NT) {
            const int r = c / (CS * 2 / 16);
            const int jc = c % (CS * 2 / 16);
            store16_sc1((char*)(dst + (long)r * Hp + ct * CS) + jc * 16, z);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0)
            __hip_atomic_fetch_add(&cnt[g], 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
    }

    for (int u = 0; u < Tseq; ++u) {
        const int tt = rev ? (Tseq - 1 - u) : u;
        const unsigned want = (unsigned)CT * (u + 1);

        // ---- wait for all of h_{u-1} ----
        // The poll is BOUNDED: if a peer block were never scheduled the
        // kernel must terminate (garbage output) rather than wedge the
        // GPU. The grid is sized to exactly fit co-resident (1 block/CU),
        // so the cap should never trip in practice.
        if (tid == 0) {
            long spins = 0;
            while (__hip_atomic_load(&cnt[g], __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT) < want) {
                __builtin_amdgcn_s_sleep(8);
                if (++spins > (1L << 24)) break;
            }
        }
        __syncthreads();

        // ---- load h_{u-1} fragments (sc1) and run the recurrent GEMM ----
        const __hip_bfloat16* hsrc =
            pub_base + (long)(u & 1) * ring_stride;   // slot of h_{u-1}
        f32x4_t acc[NCT][MT];
#pragma unroll
        for (int i = 0; i < NCT; ++i)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[i][m] = f32x4_t{0.f};
        {
            const int arow = lane & 15;
            const int koff = 8 * (lane >> 4);
            // h fragments via NONTEMPORAL loads: `nt` bypasses the L1
            // exactly like sc1 (ring slots repeat every 2 steps, so an
            // L1 hit would be stale) while staying compiler-tracked —
            // precise waitcnt scheduling for free.
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const int kbase = 32 * kk + koff;
                bf16x8_t a[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const int row = 16 * (wave + NW * m) + arow;
                    a[m] = __builtin_nontemporal_load(
                        (const bf16x8_t*)(hsrc + (long)row * Hp + kbase));
                }
#pragma unroll
                for (int i = 0; i < NCT; ++i) {
                    const bf16x8_t b = *(const bf16x8_t*)&(
                        (const __bf16*)w_s)[(i * 16 + (lane & 15)) * WPITCH +
                                            kbase];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        acc[i][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            a[m], b, acc[i][m], 0, 0, 0);
                }
            }
        }

        // ---- fused gates for the block's CS columns ----
        float hnew_keep[JT][MT][4];
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const int jj = j * 16 + (lane & 15);       // 0..CS
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * (wave + NW * m) + 4 * (lane >> 4) + e;
                    const float gr = acc[j][m][e] + bhh_s[jj];
                    const float gz = acc[JT + j][m][e] + bhh_s[CS + jj];
                    const float hn = acc[2 * JT + j][m][e] + bhh_s[2 * CS + jj];
                    const float ir = (float)((const __bf16*)gi_s)[b * GP + jj];
                    const float iz =
                        (float)((const __bf16*)gi_s)[b * GP + CS + jj];
                    const float in_ =
                        (float)((const __bf16*)gi_s)[b * GP + 2 * CS + jj];
                    const float r = sigmoidf(ir + gr);
                    const float z = sigmoidf(iz + gz);
                    const float n = fast_tanh(in_ + r * hn);
                    const float hnew = (1.0f - z) * n + z * hreg[j][m][e];
                    hreg[j][m][e] = hnew;
                    hnew_keep[j][m][e] = hnew;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();   // gi_s reads done; reuse its space as h stage

        // ---- stage h_t slice in LDS (BR x CS bf16), write out + publish --
        __hip_bfloat16* hst = gi_s;   // (BR, CS) in the gi buffer's space
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const int jj = j * 16 + (lane & 15);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * (wave + NW * m) + 4 * (lane >> 4) + e;
                    ((__bf16*)hst)[b * CS + jj] =
                        (__bf16)__float2bfloat16(hnew_keep[j][m][e]);
                }
        }
        __syncthreads();
        // out[t] slice (plain stores) + publication (sc1 stores)
        store_tile<__hip_bfloat16, BR, NT>(
            hst, out_b + (long)tt * n_dir * Hp + ct * CS, CS, CS, out_row,
            rows_valid, tid);
        if (out_drop != nullptr) {
            // fused forward dropout (same octet mask as dropout_kernel
            // over the (B, T, n_dir*Hp) out layout)
            __hip_bfloat16* dst = out_drop + (long)b0 * out_row +
                                  (long)dir * Hp + (long)tt * n_dir * Hp +
                                  ct * CS;
            constexpr int CPR = CS * 2 / 16;
            for (int c = tid; c < BR * CPR; c += NT) {
                const int r = c / CPR, jc = c % CPR;
                if (r >= rows_valid) continue;
                bf16x8_t v = *(const bf16x8_t*)((const char*)hst +
                                                (long)r * CS * 2 + jc * 16);
                const long o = ((long)(b0 + r) * Tseq + tt) * n_dir * Hp +
                               (long)dir * Hp + ct * CS + jc * 8;
                const unsigned long long rnd =
                    mix64(drop_seed ^ (unsigned long long)(o >> 3));
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const unsigned int u =
                        (unsigned int)(rnd >> (8 * k)) & 0xFF;
                    const float f =
                        (u < drop_thr)
                            ? 0.0f : (float)((__bf16*)&v)[k] * drop_scale;
                    ((__bf16*)&v)[k] = (__bf16)__float2bfloat16(f);
                }
                *(bf16x8_t*)((char*)dst + (long)r * out_row * 2 + jc * 16) =
                    v;
            }
        }
        {
            __hip_bfloat16* dst = pub_base + (long)((u + 1) & 1) * ring_stride;
            constexpr int CPR = CS * 2 / 16;
            for (int c = tid; c < BR * CPR; c += NT) {
                const int r = c / CPR;
                const int jc = c % CPR;
                u32x4_t v = *(const u32x4_t*)((const char*)hst +
                                              (long)r * CS * 2 + jc * 16);
                store16_sc1((char*)(dst + (long)r * Hp + ct * CS) + jc * 16,
                            v);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0)
            __hip_atomic_fetch_add(&cnt[g], 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        // stage gi for the next step (overwrites the h stage; safe: the
        // publish reads above finished before this barrier)
        if (u + 1 < Tseq)
            stage_gi(rev ? (Tseq - 2 - u) : (u + 1));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
    }

    {   // epilogue: hlast (fp32) for the block's columns
        float* hl = hlast + ((long)dir * B + b0) * Hp + ct * CS;
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const int jj = j * 16 + (lane & 15);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * (wave + NW * m) + 4 * (lane >> 4) + e;
                    if (b < rows_valid) hl[(long)b * Hp + jj] = hreg[j][m][e];
                }
        }
    }
}

extern "C" int fmda_gru_fwd_cs_launch(const void* gi, const void* w,
                                      const float* bhh, void* out,
                                      float* hlast, void* hpub,
                                      unsigned int* cnt, int B, int Tseq,
                                      int n_dir, void* out_drop,
                                      unsigned int drop_thr,
                                      float drop_scale,
                                      unsigned long long drop_seed,
                                      long gi_pitch, hipStream_t stream) {
    constexpr int BR = CS_BR, Hp = 512, CS = 32, NT = CS_NT;
    const int GB = (B + BR - 1) / BR;
    constexpr size_t lds = CsLds<BR, Hp, CS>::bytes;
    auto k = gru_fwd_cs_kernel<BR, Hp, CS, NT>;
    (void)hipFuncSetAttribute((const void*)k,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 grid(GB * (Hp / CS) * n_dir);
    k<<<grid, NT, lds, stream>>>((const __hip_bfloat16*)gi,
                                 (const __hip_bfloat16*)w, bhh,
                                 (__hip_bfloat16*)out, hlast,
                                 (__hip_bfloat16*)hpub, cnt, B, Tseq, n_dir,
                                 GB, (__hip_bfloat16*)out_drop, drop_thr,
                                 drop_scale, drop_seed, gi_pitch);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ===========================================================================
// Column-split persistent BPTT for Hp = 512 (design notes on the forward
// kernel above apply). The exchanged quantity here is dGh: the carry GEMM
// dh_j += sum_n dGh[n] W[n][j] needs ALL 3Hp gate rows, so each block
// publishes its three 32-column dGh strips into a (BR, 3Hp) ring image
// that readers consume as contiguous MFMA A-fragments. Per step:
//   1. poll for the full dGh(u+1) set; carry GEMM (A = sc1 asm loads from
//      the ring, software-pipelined in 8-k-slice chunks; B = W^T fragments
//      streamed from the XCD L2 as ordinary loads — legal, no glds here),
//   2. recompute GEMM gh = out(u-1) @ W_A^T (W_A slice LDS-resident,
//      out read with plain loads - it is a static kernel input),
//   3. fused gate grads for the block's 32 columns (dout/h_prev scalars
//      register-prefetched one step ahead),
//   4. dGi strip stores, then the n-slot swap (dn -> dhn), dGh strip
//      stores + sc1 publication + arrival atomic.
// dir = group & 1 so each XCD hosts one direction (W + W^T fit its L2).
// ===========================================================================
template <int BR, int Hp, int CS, int NT>
__global__ __attribute__((amdgpu_flat_work_group_size(NT, NT),
                          amdgpu_waves_per_eu(2, 2)))
void gru_bwd_cs_kernel(const __hip_bfloat16* __restrict__ gi,
                       const __hip_bfloat16* __restrict__ w,
                       const __hip_bfloat16* __restrict__ wt,
                       const float* __restrict__ bhh,
                       const __hip_bfloat16* __restrict__ out,
                       const __hip_bfloat16* __restrict__ dout,
                       const float* __restrict__ dhT,
                       __hip_bfloat16* __restrict__ dgi,
                       __hip_bfloat16* __restrict__ dgh,
                       float* __restrict__ dh0, float* __restrict__ dbhh,
                       __hip_bfloat16* __restrict__ gpub,  // (2,G,BR,3Hp)
                       unsigned int* __restrict__ cnt, int B, int Tseq,
                       int n_dir, int GB, unsigned int drop_thr,
                       float drop_scale, unsigned long long drop_seed) {
    constexpr int CT = Hp / CS;
    constexpr int NW = NT / 64;
    constexpr int MT = BR / 16 / NW;
    constexpr int NCT = 3 * CS / 16;     // 6 gate-column tiles
    constexpr int JT = CS / 16;          // 2 h-column tiles
    constexpr int KK = Hp / 32;          // 16 (recompute GEMM K)
    constexpr int KK2 = 3 * Hp / 32;     // 48 (carry GEMM K)
    constexpr int WPITCH = CsLds<BR, Hp, CS>::WPITCH;
    constexpr int GP = CsLds<BR, Hp, CS>::GP;          // LDS gi/stage pitch

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int id = blockIdx.x;
    const int nG = GB * n_dir;
    int g, ct;
    if (nG >= 8 && (nG % 8) == 0) {
        ct = (id / 8) % CT;
        g = (id % 8) + 8 * ((id / 8) / CT);
    } else {
        g = id / CT;
        ct = id % CT;
    }
    const int dir = (n_dir == 2) ? (g & 1) : 0;   // one direction per XCD
    const int gb = (n_dir == 2) ? (g >> 1) : g;
    const bool rev = (dir == 1);
    const int b0 = gb * BR;
    const int rows_valid = min(BR, B - b0);

    extern __shared__ __attribute__((aligned(16))) char smem[];
    using L = CsLds<BR, Hp, CS>;
    __hip_bfloat16* w_s = (__hip_bfloat16*)(smem + L::w);    // W_A slice
    __hip_bfloat16* gi_s = (__hip_bfloat16*)(smem + L::gi);  // also dGi/dGh stage
    float* bhh_s = (float*)(smem + L::bhh);

    const long gi_row = (long)Tseq * n_dir * 3 * Hp;
    const long out_row = (long)Tseq * n_dir * Hp;
    const __hip_bfloat16* wdir = w + (long)dir * 3 * Hp * Hp;
    const __hip_bfloat16* wt_dir = wt + (long)dir * Hp * 3 * Hp;
    for (int g3 = 0; g3 < 3; ++g3) {
        stage_tile<__hip_bfloat16, CS, NT>(
            w_s + g3 * CS * WPITCH, wdir + (long)(g3 * Hp + ct * CS) * Hp,
            Hp, WPITCH, Hp, CS, tid);
        for (int c = tid; c < CS; c += NT)
            bhh_s[g3 * CS + c] =
                bhh[(long)dir * 3 * Hp + g3 * Hp + ct * CS + c];
    }

    const __hip_bfloat16* gi_b = gi + (long)b0 * gi_row + (long)dir * 3 * Hp;
    __hip_bfloat16* dgi_b = dgi + (long)b0 * gi_row + (long)dir * 3 * Hp;
    __hip_bfloat16* dgh_b = dgh + (long)b0 * gi_row + (long)dir * 3 * Hp;
    const __hip_bfloat16* out_b = out + (long)b0 * out_row + (long)dir * Hp;
    const __hip_bfloat16* dout_b = dout + (long)b0 * out_row + (long)dir * Hp;
    __hip_bfloat16* pub_base = gpub + (long)g * BR * 3 * Hp;
    const long ring_stride = (long)nG * BR * 3 * Hp;

    auto stage_gi = [&](int tt) {
        const __hip_bfloat16* src = gi_b + (long)tt * n_dir * 3 * Hp;
        for (int g3 = 0; g3 < 3; ++g3)
            stage_tile<__hip_bfloat16, BR, NT>(
                gi_s + g3 * CS, src + g3 * Hp + ct * CS, CS, GP, gi_row,
                rows_valid, tid);
    };

    // carry + per-lane scalars for the block's own columns
    float dhcar[JT][MT][4];
    float dbacc[JT][4];
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) dbacc[j][q4] = 0.0f;
    {
        const float* hT = dhT + ((long)dir * B + b0) * Hp + ct * CS;
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const int jj = j * 16 + (lane & 15);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * (wave + NW * m) + 4 * (lane >> 4) + e;
                    dhcar[j][m][e] =
                        (b < rows_valid) ? hT[(long)b * Hp + jj] : 0.0f;
                }
        }
    }

    {   // prologue: stage gi(T-1)
        stage_gi(rev ? 0 : (Tseq - 1));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
    }

    for (int u = Tseq - 1; u >= 0; --u) {
        const int tt = rev ? (Tseq - 1 - u) : u;
        const bool have_prev = (u + 1 < Tseq);

        // ---- carry GEMM: dh += dGh(u+1) @ W^T (own columns) ----
        if (have_prev) {
            const unsigned want = (unsigned)CT * (Tseq - 1 - u);
            if (tid == 0) {
                long spins = 0;
                while (__hip_atomic_load(&cnt[g], __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT) < want) {
                    __builtin_amdgcn_s_sleep(8);
                    if (++spins > (1L << 24)) break;
                }
            }
            __syncthreads();
            const __hip_bfloat16* asrc =
                pub_base + (long)((u + 1) & 1) * ring_stride;
            f32x4_t acc2[JT][MT];
#pragma unroll
            for (int j = 0; j < JT; ++j)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc2[j][m] = f32x4_t{0.f};
            const int arow = lane & 15;
            const int koff = 8 * (lane >> 4);
            // Ring reads via NONTEMPORAL loads (L1 bypass, compiler-
            // tracked — see the forward kernel note); W^T fragments are
            // plain L2 loads. The compiler schedules and waits both.
            // Partial unroll: a full KK2=48 unroll batches enough live
            // loads to spill.
#pragma unroll 4
            for (int kk = 0; kk < KK2; ++kk) {
                const int kbase = 32 * kk + koff;
                bf16x8_t a[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const int row = 16 * (wave + NW * m) + arow;
                    a[m] = __builtin_nontemporal_load(
                        (const bf16x8_t*)(asrc + (long)row * 3 * Hp + kbase));
                }
#pragma unroll
                for (int j = 0; j < JT; ++j) {
                    const bf16x8_t bfr = *(const bf16x8_t*)&(
                        (const __bf16*)wt_dir)[
                        (long)(ct * CS + j * 16 + (lane & 15)) * 3 * Hp +
                        kbase];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        acc2[j][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            a[m], bfr, acc2[j][m], 0, 0, 0);
                }
            }
#pragma unroll
            for (int j = 0; j < JT; ++j)
#pragma unroll
                for (int m = 0; m < MT; ++m)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        dhcar[j][m][e] += acc2[j][m][e];
        }

        // ---- recompute GEMM: gh = out(u-1) @ W_A^T ----
        const bool haveh = (u > 0);
        const __hip_bfloat16* hsrc =
            out_b + (long)(rev ? (Tseq - u) : (u - 1)) * n_dir * Hp;
        f32x4_t acc[NCT][MT];
#pragma unroll
        for (int i = 0; i < NCT; ++i)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[i][m] = f32x4_t{0.f};
        if (haveh) {
            const int arow = lane & 15;
            const int koff = 8 * (lane >> 4);
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const int kbase = 32 * kk + koff;
                bf16x8_t a[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    // clamp: `out` is a real (B, ...) tensor, not the
                    // always-BR-row publication ring — dead rows must not
                    // read past the batch end (garbage rows are fine).
                    int row = 16 * (wave + NW * m) + arow;
                    if (row >= rows_valid) row = 0;
                    a[m] = *(const bf16x8_t*)(hsrc + (long)row * out_row +
                                              kbase);
                }
#pragma unroll
                for (int i = 0; i < NCT; ++i) {
                    const bf16x8_t b = *(const bf16x8_t*)&(
                        (const __bf16*)w_s)[(i * 16 + (lane & 15)) * WPITCH +
                                            kbase];
#pragma unroll
                    for (int m = 0; m < MT; ++m)
                        acc[i][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            a[m], b, acc[i][m], 0, 0, 0);
                }
            }
        }

        // ---- fused gate grads for the block's columns ----
        const __hip_bfloat16* do_t = dout_b + (long)tt * n_dir * Hp + ct * CS;
        float keep_dhn[JT][MT][4];
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const int jj = j * 16 + (lane & 15);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * (wave + NW * m) + 4 * (lane >> 4) + e;
                    const bool live = (b < rows_valid);
                    const float gr = acc[j][m][e] + bhh_s[jj];
                    const float gz = acc[JT + j][m][e] + bhh_s[CS + jj];
                    const float hn =
                        acc[2 * JT + j][m][e] + bhh_s[2 * CS + jj];
                    const float ir = (float)((const __bf16*)gi_s)[b * GP + jj];
                    const float iz =
                        (float)((const __bf16*)gi_s)[b * GP + CS + jj];
                    const float in_ =
                        (float)((const __bf16*)gi_s)[b * GP + 2 * CS + jj];
                    const float r = sigmoidf(ir + gr);
                    const float z = sigmoidf(iz + gz);
                    const float n = fast_tanh(in_ + r * hn);
                    const float hprev =
                        (live && haveh)
                            ? (float)hsrc[(long)b * out_row + ct * CS + jj]
                            : 0.0f;
                    float doval =
                        live ? (float)do_t[(long)b * out_row + jj] : 0.0f;
                    if (drop_thr != 0u) {
                        // fused inter-layer dropout backward: recompute
                        // the counter-based mask at the d_out read (the
                        // v3 kernel's scheme at the cs shapes)
                        const long o = ((long)(b0 + b) * Tseq + tt) *
                                           n_dir * Hp +
                                       (long)dir * Hp + ct * CS + jj;
                        const unsigned long long rnd =
                            mix64(drop_seed ^ (unsigned long long)(o >> 3));
                        const unsigned int u =
                            (unsigned int)(rnd >> (8 * ((int)o & 7))) & 0xFF;
                        doval = (u < drop_thr) ? 0.0f : doval * drop_scale;
                    }
                    const float dht = dhcar[j][m][e] + doval;
                    const float dz_pre =
                        live ? dht * (hprev - n) * z * (1.0f - z) : 0.0f;
                    const float dn_pre =
                        live ? dht * (1.0f - z) * (1.0f - n * n) : 0.0f;
                    const float dr_pre =
                        live ? dn_pre * hn * r * (1.0f - r) : 0.0f;
                    const float dhn = live ? dn_pre * r : 0.0f;
                    // stage dGi (dr, dz, dn) into the gi buffer in place
                    ((__bf16*)gi_s)[b * GP + jj] =
                        (__bf16)__float2bfloat16(dr_pre);
                    ((__bf16*)gi_s)[b * GP + CS + jj] =
                        (__bf16)__float2bfloat16(dz_pre);
                    ((__bf16*)gi_s)[b * GP + 2 * CS + jj] =
                        (__bf16)__float2bfloat16(dn_pre);
                    keep_dhn[j][m][e] = dhn;
                    dhcar[j][m][e] = live ? dht * z : 0.0f;
                    dbacc[j][0] += dr_pre;
                    dbacc[j][1] += dz_pre;
                    dbacc[j][2] += dhn;
                    dbacc[j][3] += dn_pre;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();

        // ---- store dGi strips; swap n-slot to dhn; store + publish dGh --
        {
            __hip_bfloat16* dst = dgi_b + (long)tt * n_dir * 3 * Hp;
            for (int g3 = 0; g3 < 3; ++g3)
                store_tile<__hip_bfloat16, BR, NT>(
                    gi_s + g3 * CS, dst + g3 * Hp + ct * CS, CS, GP, gi_row,
                    rows_valid, tid);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const int jj = j * 16 + (lane & 15);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * (wave + NW * m) + 4 * (lane >> 4) + e;
                    ((__bf16*)gi_s)[b * GP + 2 * CS + jj] =
                        (__bf16)__float2bfloat16(keep_dhn[j][m][e]);
                }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
        {
            // time-shifted global dGh (slot pairs with out[t]; v2/v3
            // semantics) + publication for the carry GEMM of step u-1
            const int sh = rev ? (tt + 1) : (tt - 1);
            if (sh >= 0 && sh < Tseq) {
                __hip_bfloat16* dst = dgh_b + (long)sh * n_dir * 3 * Hp;
                for (int g3 = 0; g3 < 3; ++g3)
                    store_tile<__hip_bfloat16, BR, NT>(
                        gi_s + g3 * CS, dst + g3 * Hp + ct * CS, CS, GP,
                        gi_row, rows_valid, tid);
            } else {
                __hip_bfloat16* dst =
                    dgh_b + (long)(rev ? 0 : (Tseq - 1)) * n_dir * 3 * Hp;
                for (int g3 = 0; g3 < 3; ++g3)
                    store_zero_tile<__hip_bfloat16, BR, NT>(
                        dst + g3 * Hp + ct * CS, CS, gi_row, rows_valid, tid);
            }
            if (u > 0) {
                __hip_bfloat16* dst =
                    pub_base + (long)(u & 1) * ring_stride;
                constexpr int CPR = CS * 2 / 16;
                for (int g3 = 0; g3 < 3; ++g3)
                    for (int c = tid; c < BR * CPR; c += NT) {
                        const int r = c / CPR;
                        const int jc = c % CPR;
                        u32x4_t v = *(const u32x4_t*)((const char*)(gi_s +
                                        g3 * CS) + (long)r * GP * 2 + jc * 16);
                        store16_sc1((char*)(dst + (long)r * 3 * Hp +
                                            g3 * Hp + ct * CS) + jc * 16, v);
                    }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0)
                    __hip_atomic_fetch_add(&cnt[g], 1u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (u > 0)
            stage_gi(rev ? (Tseq - u) : (u - 1));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
    }

    {   // epilogue: dh0 + packed bias sums (layout (n_dir, 4Hp))
        float* d0 = dh0 + ((long)dir * B + b0) * Hp + ct * CS;
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const int jj = j * 16 + (lane & 15);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 16 * (wave + NW * m) + 4 * (lane >> 4) + e;
                    if (b < rows_valid) d0[(long)b * Hp + jj] = dhcar[j][m][e];
                }
        }
        // packed bias sums: per j-tile column, reduce the row-quarter
        // lanes and emit one store per (slot, column). The waves of a
        // block split the batch rows, so each (batch group, wave) owns a
        // row of the partials table — (gb * NW + wave, n_dir, 4Hp) — and
        // the host sums the rows in a fixed order (bitwise reproducible,
        // unlike float atomics). Row layout (n_dir, 4Hp) = [dr | dz | dhn
        // | dn] (db_hh / db_ih assembled host-side exactly as for the
        // Hp=128 kernels).
        float* dbrow =
            dbhh + (((long)gb * NW + wave) * n_dir + dir) * 4 * Hp;
#pragma unroll
        for (int j = 0; j < JT; ++j)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                float v = dbacc[j][q4];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if ((lane >> 4) == 0)
                    dbrow[q4 * Hp + ct * CS + j * 16 + (lane & 15)] = v;
            }
    }
}

// ===========================================================================
// Counter-based dropout (the reference's nn.Dropout call
// sites, biGRU_model.py:50-52,87-94). The mask is a pure function of
// (seed, element index) via a splitmix64 mix, so backward RECOMPUTES it
// instead of loading a saved mask — half the memory traffic of the eager
// pair (no mask tensor exists at all). Keep/scale semantics match
// torch.nn.functional.dropout (scale 1/(1-p) on kept elements).
// ===========================================================================

template <typename T>
__global__ void dropout_kernel(const T* __restrict__ x, T* __restrict__ y,
                               long n, unsigned int thr, float scale,
                               unsigned long long seed) {
    // 8 elements per thread; the mask bits come from one mix64 per octet
    const long o = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (o >= n) return;
    // ONE mix64 per octet: its 8 bytes are 8 per-element draws against an
    // 8-bit threshold (p quantized to 1/256 — immaterial for dropout and
    // 9x less hashing, which made the kernel compute-bound).
    const unsigned long long r = mix64(seed ^ (unsigned long long)(o >> 3));
    if (o + 8 <= n) {
        T v[8];
        *(chunk16*)v = *(const chunk16*)(x + o);  // bf16 x8 = 16 B
#pragma unroll
        for (int k = 0; k < 8; ++k)
            v[k] = from_f32<T>(drop_apply(to_f32<T>(v[k]),
                                          drop_hit(r, k, thr), scale));
        *(chunk16*)(y + o) = *(const chunk16*)v;
    } else {
        for (long i = o; i < n; ++i)
            y[i] = from_f32<T>(drop_apply(
                to_f32<T>(x[i]), drop_hit(r, (int)(i - o), thr), scale));
    }
}

// (thr, scale) come from the binding's single drop_params(): the fused
// recurrence epilogues use the very same pair, so all four dropout paths
// agree bitwise.
extern "C" int fmda_dropout_launch(int is_bf16, const void* x, void* y,
                                   long n, unsigned int thr, float scale,
                                   unsigned long long seed,
                                   hipStream_t stream) {
    const long threads = (n + 7) / 8;
    const dim3 grid((threads + 255) / 256);
    if (is_bf16)
        dropout_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
            (const __hip_bfloat16*)x, (__hip_bfloat16*)y, n, thr, scale,
            seed);
    else
        return -2;  // bf16-only: the fp32 paths use torch's dropout
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Spatial (channel) dropout: the reference's Dropout2d call
// (biGRU_model.py:50-52,87-94) zeroes whole FEATURE channels — the mask is
// a function of (b, f) only and is shared by every timestep. Counter-based
// like dropout_kernel (one splitmix64 draw per channel octet, recomputed in
// backward), but WITHOUT the permute(0,2,1) round trips the reference needs:
// the mask is evaluated per element of the natural (B, T, F) layout.
template <typename T>
__global__ void spatial_dropout_kernel(const T* __restrict__ x,
                                       T* __restrict__ y, long n, long TF,
                                       int F, unsigned int thr, float scale,
                                       unsigned long long seed) {
    const long o = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (o >= n) return;
    const int cnt = (int)((o + 8 <= n) ? 8 : (n - o));
    T v[8];
    if (cnt == 8)
        *(chunk16*)v = *(const chunk16*)(x + o);
    else
        for (int k = 0; k < cnt; ++k) v[k] = x[o + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k >= cnt) break;
        const long i = o + k;
        const long c = (i / TF) * F + (i % F);   // channel id (b, f)
        const unsigned long long r =
            mix64(seed ^ (unsigned long long)(c >> 3));
        v[k] = from_f32<T>(drop_apply(to_f32<T>(v[k]),
                                      drop_hit(r, (int)c & 7, thr), scale));
    }
    if (cnt == 8)
        *(chunk16*)(y + o) = *(const chunk16*)v;
    else
        for (int k = 0; k < cnt; ++k) y[o + k] = v[k];
}

extern "C" int fmda_spatial_dropout_launch(int is_bf16, const void* x,
                                           void* y, long B, long Tlen, long F,
                                           unsigned int thr, float scale,
                                           unsigned long long seed,
                                           hipStream_t stream) {
    if (!is_bf16) return -2;
    const long n = B * Tlen * F;
    const long threads = (n + 7) / 8;
    const dim3 grid((threads + 255) / 256);
    spatial_dropout_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
        (const __hip_bfloat16*)x, (__hip_bfloat16*)y, n, Tlen * F, (int)F,
        thr, scale, seed);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ===========================================================================
// Fused direction-sum + temporal max/avg pooling (biGRU_model.py:108-133
// semantics: gru_out = fwd_dir + bwd_dir; max over T with argmax; sum/T).
// One thread per (b, h): replaces four eager kernels (direction add, max
// reduce, sum reduce, and the backward scatter) with one read / one write
// pass over the (B, T, n_dir*H) activations.
// OT is the type of the pooled outputs and GT that of their incoming
// gradients: float, or the activation type T, which spares the caller a
// cast kernel per tensor (the value is rounded once either way).
// ===========================================================================
template <typename T, typename OT>
__global__ void pool_fwd_kernel(const T* __restrict__ out,
                                OT* __restrict__ maxv,
                                OT* __restrict__ avgv,
                                int* __restrict__ amax, int B, int Tseq,
                                int H, int n_dir) {
    // one thread per (b, h-pair): 4-byte loads keep the row reads at full
    // cache-line efficiency (2-byte-per-lane halves it)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int HP2 = H / 2;
    if (idx >= B * HP2) return;
    const int b = idx / HP2;
    const int h2 = (idx % HP2) * 2;
    const int HD = n_dir * H;
    const T* p = out + (long)b * Tseq * HD + h2;
    float mx0 = -3.4e38f, mx1 = -3.4e38f, s0 = 0.0f, s1 = 0.0f;
    int im0 = 0, im1 = 0;
    for (int t = 0; t < Tseq; ++t) {
        const T* pt = p + (long)t * HD;
        struct alignas(2 * sizeof(T)) Pair { T x, y; };
        const Pair v2 = *(const Pair*)pt;
        float v0 = to_f32<T>(v2.x), v1 = to_f32<T>(v2.y);
        if (n_dir == 2) {
            const Pair w2 = *(const Pair*)(pt + H);
            v0 += to_f32<T>(w2.x);
            v1 += to_f32<T>(w2.y);
        }
        s0 += v0; s1 += v1;
        if (v0 > mx0) { mx0 = v0; im0 = t; }
        if (v1 > mx1) { mx1 = v1; im1 = t; }
    }
    const int o = b * H + h2;
    maxv[o] = from_f32<OT>(mx0); maxv[o + 1] = from_f32<OT>(mx1);
    avgv[o] = from_f32<OT>(s0 / (float)Tseq);
    avgv[o + 1] = from_f32<OT>(s1 / (float)Tseq);
    amax[o] = im0; amax[o + 1] = im1;
}

template <typename T, typename GT>
__global__ void pool_bwd_kernel(const GT* __restrict__ dmax,
                                const GT* __restrict__ davg,
                                const int* __restrict__ amax,
                                T* __restrict__ dout, int B, int Tseq, int H,
                                int n_dir, long ld_max, long ld_avg) {
    // ld_*: row pitch of dmax / davg in elements (column slices of the
    // pooled-feature gradient are read in place)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * H) return;
    const int b = idx / H;
    const int h = idx % H;
    const int HD = n_dir * H;
    const float ga = to_f32<GT>(davg[b * ld_avg + h]) / (float)Tseq;
    const float gm = to_f32<GT>(dmax[b * ld_max + h]);
    const int im = amax[idx];
    T* p = dout + (long)b * Tseq * HD + h;
    for (int t = 0; t < Tseq; ++t) {
        const float g = ga + (t == im ? gm : 0.0f);
        p[(long)t * HD] = from_f32<T>(g);
        if (n_dir == 2) p[(long)t * HD + H] = from_f32<T>(g);
    }
}

// Octet variants: one thread per (b, 8-column group), 16-byte bf16x8 row
// loads/stores — the pair kernels' 4-byte accesses ran at ~3.3 TB/s
// against the 6.3 TB/s stream peak. Requires H % 8 == 0 (the pair kernels
// stay as the fallback for odd hidden sizes).
template <typename OT>
__global__ void pool_fwd_oct_kernel(const __hip_bfloat16* __restrict__ out,
                                    OT* __restrict__ maxv,
                                    OT* __restrict__ avgv,
                                    int* __restrict__ amax, int B, int Tseq,
                                    int H, int n_dir) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int H8 = H / 8;
    if (idx >= B * H8) return;
    const int b = idx / H8;
    const int h8 = (idx % H8) * 8;
    const int HD = n_dir * H;
    const __hip_bfloat16* p = out + (long)b * Tseq * HD + h8;
    float mx[8], s[8];
    int im[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { mx[k] = -3.4e38f; s[k] = 0.0f; im[k] = 0; }
    for (int t = 0; t < Tseq; ++t) {
        const __hip_bfloat16* pt = p + (long)t * HD;
        bf16x8_t v = *(const bf16x8_t*)pt;
        bf16x8_t w;
        if (n_dir == 2) w = *(const bf16x8_t*)(pt + H);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float x = (float)((const __bf16*)&v)[k];
            if (n_dir == 2) x += (float)((const __bf16*)&w)[k];
            s[k] += x;
            if (x > mx[k]) { mx[k] = x; im[k] = t; }
        }
    }
    const int o = b * H + h8;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        maxv[o + k] = from_f32<OT>(mx[k]);
        avgv[o + k] = from_f32<OT>(s[k] / (float)Tseq);
        amax[o + k] = im[k];
    }
}

template <typename GT>
__global__ void pool_bwd_oct_kernel(const GT* __restrict__ dmax,
                                    const GT* __restrict__ davg,
                                    const int* __restrict__ amax,
                                    __hip_bfloat16* __restrict__ dout,
                                    int B, int Tseq, int H, int n_dir,
                                    long ld_max, long ld_avg) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int H8 = H / 8;
    if (idx >= B * H8) return;
    const int b = idx / H8;
    const int h8 = (idx % H8) * 8;
    const int o = b * H + h8;
    float ga[8], gm[8];
    int im[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        ga[k] = to_f32<GT>(davg[b * ld_avg + h8 + k]) / (float)Tseq;
        gm[k] = to_f32<GT>(dmax[b * ld_max + h8 + k]);
        im[k] = amax[o + k];
    }
    const int HD = n_dir * H;
    __hip_bfloat16* p = dout + (long)b * Tseq * HD + h8;
    for (int t = 0; t < Tseq; ++t) {
        bf16x8_t v;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            ((__bf16*)&v)[k] =
                (__bf16)__float2bfloat16(ga[k] + (t == im[k] ? gm[k] : 0.0f));
        *(bf16x8_t*)(p + (long)t * HD) = v;
        if (n_dir == 2) *(bf16x8_t*)(p + (long)t * HD + H) = v;
    }
}

// Small-batch variant (the streaming predict path: B=1 would give the
// thread-per-pair kernel a 2-wave grid looping serially over T): one WAVE
// per (b, h-pair), lanes strided over T, max/argmax/sum combined with
// shfl_xor reductions. Argmax tie-break keeps the smallest t — exactly the
// sequential kernel's first-strictly-greater scan.
template <typename T, typename OT>
__global__ void pool_fwd_small_kernel(const T* __restrict__ out,
                                      OT* __restrict__ maxv,
                                      OT* __restrict__ avgv,
                                      int* __restrict__ amax, int B, int Tseq,
                                      int H, int n_dir) {
    const int HP2 = H / 2;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * (blockDim.x >> 6) + wave;
    if (idx >= B * HP2) return;
    const int b = idx / HP2;
    const int h2 = (idx % HP2) * 2;
    const int HD = n_dir * H;
    const T* p = out + (long)b * Tseq * HD + h2;
    float mx0 = -3.4e38f, mx1 = -3.4e38f, s0 = 0.0f, s1 = 0.0f;
    int im0 = Tseq, im1 = Tseq;
    for (int t = lane; t < Tseq; t += 64) {
        const T* pt = p + (long)t * HD;
        struct alignas(2 * sizeof(T)) Pair { T x, y; };
        const Pair v2 = *(const Pair*)pt;
        float v0 = to_f32<T>(v2.x), v1 = to_f32<T>(v2.y);
        if (n_dir == 2) {
            const Pair w2 = *(const Pair*)(pt + H);
            v0 += to_f32<T>(w2.x);
            v1 += to_f32<T>(w2.y);
        }
        s0 += v0; s1 += v1;
        if (v0 > mx0) { mx0 = v0; im0 = t; }
        if (v1 > mx1) { mx1 = v1; im1 = t; }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float omx0 = __shfl_xor(mx0, d), omx1 = __shfl_xor(mx1, d);
        const int oim0 = __shfl_xor(im0, d), oim1 = __shfl_xor(im1, d);
        s0 += __shfl_xor(s0, d);
        s1 += __shfl_xor(s1, d);
        if (omx0 > mx0 || (omx0 == mx0 && oim0 < im0)) { mx0 = omx0; im0 = oim0; }
        if (omx1 > mx1 || (omx1 == mx1 && oim1 < im1)) { mx1 = omx1; im1 = oim1; }
    }
    if (lane == 0) {
        const int o = b * H + h2;
        maxv[o] = from_f32<OT>(mx0); maxv[o + 1] = from_f32<OT>(mx1);
        avgv[o] = from_f32<OT>(s0 / (float)Tseq);
        avgv[o + 1] = from_f32<OT>(s1 / (float)Tseq);
        amax[o] = im0; amax[o + 1] = im1;
    }
}

// act_io != 0 (bf16 only): maxv / avgv are bf16 like the activations.
// serial != 0: never the small-grid kernel, whose lanes split T and sum it
// in another order than the thread-per-column kernels' ascending t.
extern "C" int fmda_pool_fwd_launch(int is_bf16, const void* out, void* maxv,
                                    void* avgv, int* amax, int B, int Tseq,
                                    int H, int n_dir, int act_io, int serial,
                                    hipStream_t stream) {
    using bf16 = __hip_bfloat16;
    if (act_io && !is_bf16) return -2;
    const int n = B * (H / 2);   // thread per h-pair (H is always even)
    if (n < 4096 && !serial) {
        // small grid (streaming predict): wave per pair, lanes over T
        const dim3 grid((n + 3) / 4);
        if (act_io)
            pool_fwd_small_kernel<bf16, bf16><<<grid, 256, 0, stream>>>(
                (const bf16*)out, (bf16*)maxv, (bf16*)avgv, amax, B, Tseq, H,
                n_dir);
        else if (is_bf16)
            pool_fwd_small_kernel<bf16, float><<<grid, 256, 0, stream>>>(
                (const bf16*)out, (float*)maxv, (float*)avgv, amax, B, Tseq,
                H, n_dir);
        else
            pool_fwd_small_kernel<float, float><<<grid, 256, 0, stream>>>(
                (const float*)out, (float*)maxv, (float*)avgv, amax, B, Tseq,
                H, n_dir);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    if (is_bf16 && H % 8 == 0) {
        const int n8 = B * (H / 8);
        const dim3 grid8((n8 + 255) / 256);
        if (act_io)
            pool_fwd_oct_kernel<bf16><<<grid8, 256, 0, stream>>>(
                (const bf16*)out, (bf16*)maxv, (bf16*)avgv, amax, B, Tseq, H,
                n_dir);
        else
            pool_fwd_oct_kernel<float><<<grid8, 256, 0, stream>>>(
                (const bf16*)out, (float*)maxv, (float*)avgv, amax, B, Tseq,
                H, n_dir);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    const dim3 grid((n + 255) / 256);
    if (act_io)
        pool_fwd_kernel<bf16, bf16><<<grid, 256, 0, stream>>>(
            (const bf16*)out, (bf16*)maxv, (bf16*)avgv, amax, B, Tseq, H,
            n_dir);
    else if (is_bf16)
        pool_fwd_kernel<bf16, float><<<grid, 256, 0, stream>>>(
            (const bf16*)out, (float*)maxv, (float*)avgv, amax, B, Tseq, H,
            n_dir);
    else
        pool_fwd_kernel<float, float><<<grid, 256, 0, stream>>>(
            (const float*)out, (float*)maxv, (float*)avgv, amax, B, Tseq, H,
            n_dir);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// act_io != 0 (bf16 only): dmax / davg are bf16 like the activations.
// ld_max / ld_avg: their row pitches in elements (H when contiguous).
extern "C" int fmda_pool_bwd_launch(int is_bf16, const void* dmax,
                                    const void* davg, const int* amax,
                                    void* dout, int B, int Tseq, int H,
                                    int n_dir, int act_io, long ld_max,
                                    long ld_avg, hipStream_t stream) {
    using bf16 = __hip_bfloat16;
    if (act_io && !is_bf16) return -2;
    const int n = B * H;
    if (is_bf16 && H % 8 == 0 && B * (H / 8) >= 4096) {
        const int n8 = B * (H / 8);
        const dim3 grid8((n8 + 255) / 256);
        if (act_io)
            pool_bwd_oct_kernel<bf16><<<grid8, 256, 0, stream>>>(
                (const bf16*)dmax, (const bf16*)davg, amax, (bf16*)dout, B,
                Tseq, H, n_dir, ld_max, ld_avg);
        else
            pool_bwd_oct_kernel<float><<<grid8, 256, 0, stream>>>(
                (const float*)dmax, (const float*)davg, amax, (bf16*)dout, B,
                Tseq, H, n_dir, ld_max, ld_avg);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    const dim3 grid((n + 255) / 256);
    if (act_io)
        pool_bwd_kernel<bf16, bf16><<<grid, 256, 0, stream>>>(
            (const bf16*)dmax, (const bf16*)davg, amax, (bf16*)dout, B, Tseq,
            H, n_dir, ld_max, ld_avg);
    else if (is_bf16)
        pool_bwd_kernel<bf16, float><<<grid, 256, 0, stream>>>(
            (const float*)dmax, (const float*)davg, amax, (bf16*)dout, B,
            Tseq, H, n_dir, ld_max, ld_avg);
    else
        pool_bwd_kernel<float, float><<<grid, 256, 0, stream>>>(
            (const float*)dmax, (const float*)davg, amax, (float*)dout, B,
            Tseq, H, n_dir, ld_max, ld_avg);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ===========================================================================
// Pooled-head feature path in two kernels (bf16, H % 8 == 0, unpadded H):
// feat (B, 3H) = [dirsum(h_last) | max_T | avg_T] straight from the top
// layer's out and raw fp32 h_last, and its backward. Every value is what
// pool_fwd_oct_kernel / pool_bwd_oct_kernel plus the eager cast / sum / cat
// chain around them produce, bit for bit:
// - max / avg / amax: pool_fwd_oct_kernel's arithmetic in its order (fp32
//   direction sum, s += x in ascending t, first strictly greater value
//   wins, one rounding of s / T);
// - last hidden: each direction's fp32 h_last rounded to bf16 (the h_n
//   cast), the two added in fp32 and rounded again (torch's bf16 sum over
//   the direction axis accumulates in fp32); one direction: the first
//   rounding alone.
// ===========================================================================
FMDA_DEV void pool_oct_consume(const bf16x8_t& v, const bf16x8_t& w,
                               bool two_dir, int t, float (&mx)[8],
                               float (&s)[8], int (&im)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float x = (float)((const __bf16*)&v)[k];
        if (two_dir) x += (float)((const __bf16*)&w)[k];
        s[k] += x;
        if (x > mx[k]) { mx[k] = x; im[k] = t; }
    }
}

// One thread per (b, 8-column group) like pool_fwd_oct_kernel, which ran
// at 4.2 TB/s with one or two 16-byte loads in flight per thread and only
// 8 waves per CU: here the loads of UNR consecutive timesteps are issued
// before the first is consumed (UNR * ND * 16 bytes in flight per thread);
// the timesteps are still consumed in ascending order.
template <int ND, int UNR>
__global__ __launch_bounds__(256) void pool_features_fwd_kernel(
        const __hip_bfloat16* __restrict__ out,
        const float* __restrict__ hlast, __hip_bfloat16* __restrict__ feat,
        int* __restrict__ amax, int B, int Tseq, int H) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int H8 = H / 8;
    if (idx >= B * H8) return;
    const int b = idx / H8;
    const int h8 = (idx % H8) * 8;
    const int HD = ND * H;
    const __hip_bfloat16* p = out + (long)b * Tseq * HD + h8;
    float mx[8], s[8];
    int im[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { mx[k] = -3.4e38f; s[k] = 0.0f; im[k] = 0; }
    int t = 0;
    for (; t + UNR <= Tseq; t += UNR) {
        bf16x8_t v[UNR], w[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const __hip_bfloat16* pt = p + (long)(t + u) * HD;
            v[u] = *(const bf16x8_t*)pt;
            if (ND == 2) w[u] = *(const bf16x8_t*)(pt + H);
            else w[u] = v[u];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            pool_oct_consume(v[u], w[u], ND == 2, t + u, mx, s, im);
    }
    for (; t < Tseq; ++t) {
        const __hip_bfloat16* pt = p + (long)t * HD;
        const bf16x8_t v = *(const bf16x8_t*)pt;
        bf16x8_t w = v;
        if (ND == 2) w = *(const bf16x8_t*)(pt + H);
        pool_oct_consume(v, w, ND == 2, t, mx, s, im);
    }

    const float* h0p = hlast + (long)b * H + h8;
    bf16x8_t fl, fm, fa;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        __hip_bfloat16 l = __float2bfloat16(h0p[k]);
        if (ND == 2) {
            const __hip_bfloat16 r = __float2bfloat16(h0p[(long)B * H + k]);
            l = __float2bfloat16(__bfloat162float(l) + __bfloat162float(r));
        }
        ((__hip_bfloat16*)&fl)[k] = l;
        ((__hip_bfloat16*)&fm)[k] = from_f32<__hip_bfloat16>(mx[k]);
        ((__hip_bfloat16*)&fa)[k] =
            from_f32<__hip_bfloat16>(s[k] / (float)Tseq);
    }
    __hip_bfloat16* fr = feat + (long)b * 3 * H + h8;
    *(bf16x8_t*)fr = fl;
    *(bf16x8_t*)(fr + H) = fm;
    *(bf16x8_t*)(fr + 2 * H) = fa;
    int* ao = amax + (long)b * H + h8;   // 32-byte aligned: H % 8 == 0
    *(int4*)ao = make_int4(im[0], im[1], im[2], im[3]);
    *(int4*)(ao + 4) = make_int4(im[4], im[5], im[6], im[7]);
}

// Backward of the whole feature path from dfeat (B, 3H) with row pitch ld
// (elements): d_out (B, T, ND*H) exactly as pool_bwd_oct_kernel assembles
// it from the max / avg column blocks, and d_hlast (ND, B, H) fp32 =
// float(dfeat[:, :H]) for every direction (what the sum / cat / cast chain
// hands back to the top layer).
template <int ND>
__global__ __launch_bounds__(256) void pool_features_bwd_kernel(
        const __hip_bfloat16* __restrict__ dfeat,
        const int* __restrict__ amax, __hip_bfloat16* __restrict__ dout,
        float* __restrict__ dhlast, int B, int Tseq, int H, long ld) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int H8 = H / 8;
    if (idx >= B * H8) return;
    const int b = idx / H8;
    const int h8 = (idx % H8) * 8;
    const __hip_bfloat16* dr = dfeat + (long)b * ld + h8;
    const int* ai = amax + (long)b * H + h8;
    float* dh = dhlast + (long)b * H + h8;
    float ga[8], gm[8], gl[8];
    int im[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        gl[k] = __bfloat162float(dr[k]);
        gm[k] = __bfloat162float(dr[H + k]);
        ga[k] = __bfloat162float(dr[2 * H + k]) / (float)Tseq;
        im[k] = ai[k];
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) {   // 32-byte aligned: H % 8 == 0
        float* dhd = dh + (long)d * B * H;
        *(float4*)dhd = make_float4(gl[0], gl[1], gl[2], gl[3]);
        *(float4*)(dhd + 4) = make_float4(gl[4], gl[5], gl[6], gl[7]);
    }
    const int HD = ND * H;
    __hip_bfloat16* p = dout + (long)b * Tseq * HD + h8;
    for (int t = 0; t < Tseq; ++t) {
        bf16x8_t v;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            ((__bf16*)&v)[k] =
                (__bf16)__float2bfloat16(ga[k] + (t == im[k] ? gm[k] : 0.0f));
        *(bf16x8_t*)(p + (long)t * HD) = v;
        if (ND == 2) *(bf16x8_t*)(p + (long)t * HD + H) = v;
    }
}

extern "C" int fmda_pool_features_fwd_launch(const void* out,
                                             const float* hlast, void* feat,
                                             int* amax, int B, int Tseq,
                                             int H, int n_dir,
                                             hipStream_t stream) {
    using bf16 = __hip_bfloat16;
    if (H % 8 != 0 || (n_dir != 1 && n_dir != 2) || Tseq < 1) return -2;
    const int n8 = B * (H / 8);
    const dim3 grid((n8 + 255) / 256);
    // load depth 8: measured at the flagship shape (B8192 T120 H128), depths
    // 6, 8 and 15 all sit at 94-96 us (5.3 TB/s); 4 takes 113 us
    if (n_dir == 2)
        pool_features_fwd_kernel<2, 8><<<grid, 256, 0, stream>>>(
            (const bf16*)out, hlast, (bf16*)feat, amax, B, Tseq, H);
    else
        pool_features_fwd_kernel<1, 8><<<grid, 256, 0, stream>>>(
            (const bf16*)out, hlast, (bf16*)feat, amax, B, Tseq, H);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int fmda_pool_features_bwd_launch(const void* dfeat,
                                             const int* amax, void* dout,
                                             float* dhlast, int B, int Tseq,
                                             int H, int n_dir, long ld,
                                             hipStream_t stream) {
    using bf16 = __hip_bfloat16;
    if (H % 8 != 0 || (n_dir != 1 && n_dir != 2) || Tseq < 1) return -2;
    const int n8 = B * (H / 8);
    const dim3 grid((n8 + 255) / 256);
    if (n_dir == 2)
        pool_features_bwd_kernel<2><<<grid, 256, 0, stream>>>(
            (const bf16*)dfeat, amax, (bf16*)dout, dhlast, B, Tseq, H, ld);
    else
        pool_features_bwd_kernel<1><<<grid, 256, 0, stream>>>(
            (const bf16*)dfeat, amax, (bf16*)dout, dhlast, B, Tseq, H, ld);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ===========================================================================
// Streaming-inference fused kernels (the predict.py path, batch = 1;
// reference predict.py:124-197). The window ring lives ON the GPU: per
// tick the host uploads one raw fp32 feature row (384 B) and the captured
// graph runs [ingest -> gi GEMM -> b1 recurrence] x L -> pool_concat ->
// head_sigmoid — no CPU normalize, no full-window H2D, no eager glue.
// ===========================================================================

// Shift the GPU-resident window one row up and append the normalized new
// row: ring[t] = ring[t+1]; ring[T-1][f] = (row[f] - xmin[f]) / xrng[f]
// (predict.py:175 normalize + the SQL last-N-rows fetch semantics).
// One workgroup; read-everything -> barrier -> write-everything makes the
// in-place shift race-free. 48 chunks/thread x 1024 threads bounds T*F.
__global__ void ingest_row_kernel(__hip_bfloat16* __restrict__ ring,
                                  const float* __restrict__ row,
                                  const float* __restrict__ xmin,
                                  const float* __restrict__ xrng,
                                  int Tseq, int F) {
    const int n = (Tseq - 1) * F;
    const int tid = threadIdx.x;
    __hip_bfloat16 keep[48];
    int cnt = 0;
    for (int i = tid; i < n; i += blockDim.x) keep[cnt++] = ring[i + F];
    __syncthreads();
    cnt = 0;
    for (int i = tid; i < n; i += blockDim.x) ring[i] = keep[cnt++];
    for (int f = tid; f < F; f += blockDim.x)
        ring[n + f] = __float2bfloat16((row[f] - xmin[f]) / xrng[f]);
}

extern "C" int fmda_ingest_row_launch(void* ring, const float* row,
                                      const float* xmin, const float* xrng,
                                      int Tseq, int F, hipStream_t stream) {
    const int n = (Tseq - 1) * F;
    if (n > 48 * 1024) return -5;   // window too large for one workgroup
    ingest_row_kernel<<<1, 1024, 0, stream>>>(
        (__hip_bfloat16*)ring, row, xmin, xrng, Tseq, F);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Batched ingest_row for the fleet path: block s shifts ring s of
// rings (S, T, F) and appends rows[s] normalized with table s of
// xmin / xrng (S, F) — the same expression as ingest_row_kernel — unless
// active[s] == 0, in which case ring s is left untouched. The early return
// is block-uniform and precedes the barrier.
__global__ void ingest_rows_kernel(__hip_bfloat16* __restrict__ rings,
                                   const float* __restrict__ rows,
                                   const int* __restrict__ active,
                                   const float* __restrict__ xmin,
                                   const float* __restrict__ xrng,
                                   int Tseq, int F) {
    const long s = blockIdx.x;
    if (active[s] == 0) return;
    __hip_bfloat16* __restrict__ ring = rings + s * Tseq * F;
    const float* __restrict__ row = rows + s * F;
    const float* __restrict__ mn = xmin + s * F;
    const float* __restrict__ rg = xrng + s * F;
    const int n = (Tseq - 1) * F;
    const int tid = threadIdx.x;
    __hip_bfloat16 keep[48];
    int cnt = 0;
    for (int i = tid; i < n; i += blockDim.x) keep[cnt++] = ring[i + F];
    __syncthreads();
    cnt = 0;
    for (int i = tid; i < n; i += blockDim.x) ring[i] = keep[cnt++];
    for (int f = tid; f < F; f += blockDim.x)
        ring[n + f] = __float2bfloat16((row[f] - mn[f]) / rg[f]);
}

extern "C" int fmda_ingest_rows_launch(void* rings, const float* rows,
                                       const int* active, const float* xmin,
                                       const float* xrng, int S, int Tseq,
                                       int F, hipStream_t stream) {
    const long n = ((long)Tseq - 1) * F;
    if (n > 48 * 1024) return -5;   // window too large for one workgroup
    if (S < 1) return -1;
    ingest_rows_kernel<<<S, 1024, 0, stream>>>(
        (__hip_bfloat16*)rings, rows, active, xmin, xrng, Tseq, F);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Fused 3-way pooling head for inference: feat = concat[dirsum(h_last),
// maxpool_T, avgpool_T] (biGRU_model.py:108-133) in ONE kernel — replaces
// pool + hidden view/sum + cat (+ their launch latency) inside the
// captured predict graph. Wave per (b, h-pair), lanes strided over T.
template <typename T>
__global__ void pool_concat_infer_kernel(const T* __restrict__ out,
                                         const float* __restrict__ hlast,
                                         T* __restrict__ feat, int B,
                                         int Tseq, int H, int Hp, int n_dir) {
    const int HP2 = H / 2;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * (blockDim.x >> 6) + wave;
    if (idx >= B * HP2) return;
    const int b = idx / HP2;
    const int h2 = (idx % HP2) * 2;
    const int HD = n_dir * H;
    const T* p = out + (long)b * Tseq * HD + h2;
    float mx0 = -3.4e38f, mx1 = -3.4e38f, s0 = 0.0f, s1 = 0.0f;
    for (int t = lane; t < Tseq; t += 64) {
        const T* pt = p + (long)t * HD;
        struct alignas(2 * sizeof(T)) Pair { T x, y; };
        const Pair v2 = *(const Pair*)pt;
        float v0 = to_f32<T>(v2.x), v1 = to_f32<T>(v2.y);
        if (n_dir == 2) {
            const Pair w2 = *(const Pair*)(pt + H);
            v0 += to_f32<T>(w2.x);
            v1 += to_f32<T>(w2.y);
        }
        s0 += v0; s1 += v1;
        if (v0 > mx0) mx0 = v0;
        if (v1 > mx1) mx1 = v1;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float omx0 = __shfl_xor(mx0, d), omx1 = __shfl_xor(mx1, d);
        s0 += __shfl_xor(s0, d);
        s1 += __shfl_xor(s1, d);
        if (omx0 > mx0) mx0 = omx0;
        if (omx1 > mx1) mx1 = omx1;
    }
    if (lane == 0) {
        float hl0 = hlast[(long)b * Hp + h2];
        float hl1 = hlast[(long)b * Hp + h2 + 1];
        if (n_dir == 2) {
            hl0 += hlast[((long)B + b) * Hp + h2];
            hl1 += hlast[((long)B + b) * Hp + h2 + 1];
        }
        T* fr = feat + (long)b * 3 * H;
        fr[h2] = from_f32<T>(hl0);
        fr[h2 + 1] = from_f32<T>(hl1);
        fr[H + h2] = from_f32<T>(mx0);
        fr[H + h2 + 1] = from_f32<T>(mx1);
        fr[2 * H + h2] = from_f32<T>(s0 / (float)Tseq);
        fr[2 * H + h2 + 1] = from_f32<T>(s1 / (float)Tseq);
    }
}

extern "C" int fmda_pool_concat_launch(int is_bf16, const void* out,
                                       const float* hlast, void* feat, int B,
                                       int Tseq, int H, int Hp, int n_dir,
                                       hipStream_t stream) {
    const int n = B * (H / 2);
    const dim3 grid((n + 3) / 4);
    if (is_bf16)
        pool_concat_infer_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
            (const __hip_bfloat16*)out, hlast, (__hip_bfloat16*)feat, B,
            Tseq, H, Hp, n_dir);
    else
        pool_concat_infer_kernel<float><<<grid, 256, 0, stream>>>(
            (const float*)out, hlast, (float*)feat, B, Tseq, H, Hp, n_dir);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// logits = x @ W^T + b -> sigmoid, emitted directly as probabilities
// (predict.py:178-186 forward + sigmoid). Wave per (b, c), lanes over K.
template <typename T>
__global__ void head_sigmoid_kernel(const T* __restrict__ x,
                                    const T* __restrict__ W,
                                    const T* __restrict__ bias,
                                    float* __restrict__ probs, int B, int K,
                                    int C) {
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * (blockDim.x >> 6) + wave;
    if (idx >= B * C) return;
    const int b = idx / C, c = idx % C;
    const T* xr = x + (long)b * K;
    const T* wr = W + (long)c * K;
    float acc = 0.0f;
    for (int k = lane; k < K; k += 64)
        acc += to_f32<T>(xr[k]) * to_f32<T>(wr[k]);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) acc += __shfl_xor(acc, d);
    if (lane == 0) probs[idx] = sigmoidf(acc + to_f32<T>(bias[c]));
}

extern "C" int fmda_head_sigmoid_launch(int is_bf16, const void* x,
                                        const void* W, const void* bias,
                                        float* probs, int B, int K, int C,
                                        hipStream_t stream) {
    const int n = B * C;
    const dim3 grid((n + 3) / 4);
    if (is_bf16)
        head_sigmoid_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
            (const __hip_bfloat16*)x, (const __hip_bfloat16*)W,
            (const __hip_bfloat16*)bias, probs, B, K, C);
    else
        head_sigmoid_kernel<float><<<grid, 256, 0, stream>>>(
            (const float*)x, (const float*)W, (const float*)bias, probs, B,
            K, C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// head_sigmoid over a bank of heads W (M, C, K), bias (M, C): row b uses
// the head of slot[b]. Same lane-over-K sum and shuffle order as
// head_sigmoid_kernel, so a row gets the bits that kernel gives with that
// head alone.
__global__ void head_sigmoid_bank_kernel(
        const __hip_bfloat16* __restrict__ x, const int* __restrict__ slot,
        const __hip_bfloat16* __restrict__ W,
        const __hip_bfloat16* __restrict__ bias, float* __restrict__ probs,
        int B, int K, int C, int M) {
    using T = __hip_bfloat16;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * (blockDim.x >> 6) + wave;
    if (idx >= B * C) return;
    const int b = idx / C, c = idx % C;
    const long m = bank_slot(slot, b, M);
    const T* xr = x + (long)b * K;
    const T* wr = W + (m * C + c) * K;
    float acc = 0.0f;
    for (int k = lane; k < K; k += 64)
        acc += to_f32<T>(xr[k]) * to_f32<T>(wr[k]);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) acc += __shfl_xor(acc, d);
    if (lane == 0) probs[idx] = sigmoidf(acc + to_f32<T>(bias[m * C + c]));
}

extern "C" int fmda_head_sigmoid_bank_launch(const void* x, const int* slot,
                                             const void* W, const void* bias,
                                             float* probs, int B, int K,
                                             int C, int M,
                                             hipStream_t stream) {
    if (B < 1 || K < 1 || C < 1 || M < 1) return -1;
    const int n = B * C;
    head_sigmoid_bank_kernel<<<dim3((n + 3) / 4), 256, 0, stream>>>(
        (const __hip_bfloat16*)x, slot, (const __hip_bfloat16*)W,
        (const __hip_bfloat16*)bias, probs, B, K, C, M);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ===========================================================================
// Fused classifier head + BCEWithLogitsLoss (weight, pos_weight).
// Replaces nn.Linear (biGRU_model.py:137) + the notebook's
// BCEWithLogitsLoss(weight, pos_weight) (cell 29) forward/backward chain
// (~12 eager launches) with:
//   fwd: logits = x @ W^T + b; s = sigmoid(logits); per-element loss
//        l = -w[ pw*y*log(s) + (1-y)*log(1-s) ], reduced to one partial
//        per block (summed host-side). C = #classes (4), 3H small.
//   bwd: dlogits = gscale * w[ s(1 - y + pw*y) - pw*y ];
//        dx = dlogits @ W (tiny K) in one elementwise-ish kernel.
//   (dW/db reduce over B on the host via the split-K helpers.)
// ===========================================================================
template <typename T>
__global__ void head_loss_fwd_kernel(const T* __restrict__ x,
                                     const T* __restrict__ W,
                                     const T* __restrict__ bias,
                                     const float* __restrict__ y,
                                     const float* __restrict__ wgt,
                                     const float* __restrict__ pw,
                                     float* __restrict__ logits,
                                     float* __restrict__ sig,
                                     float* __restrict__ loss_sum, int B,
                                     int K, int C) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    float l = 0.0f;
    if (idx < B * C) {
        const int r = idx / C, c = idx % C;
        const T* xr = x + (long)r * K;
        const T* wr = W + (long)c * K;
        float acc = to_f32<T>(bias[c]);
        for (int k = 0; k < K; ++k)
            acc += to_f32<T>(xr[k]) * to_f32<T>(wr[k]);
        logits[idx] = acc;
        const float s = sigmoidf(acc);
        sig[idx] = s;
        const float yy = y[idx];
        // numerically-stable log-sigmoid forms
        const float m = acc > 0.0f ? acc : 0.0f;
        const float lse = m + __builtin_logf(fast_exp2(-m * FMDA_LOG2E) +
                                             fast_exp2((acc - m) * FMDA_LOG2E));
        const float log_s = acc - lse;      // log sigmoid(acc)
        const float log_1ms = -lse;         // log(1 - sigmoid(acc))
        l = -wgt[c] * (pw[c] * yy * log_s + (1.0f - yy) * log_1ms);
    }
    // block-reduce partials, one store per block into loss_sum[blockIdx.x]
    // (gridDim.x entries); the host sums them in a fixed order, so the loss
    // is bitwise reproducible (a float atomicAdd across blocks is not)
    __shared__ float red[4];
    float v = l;
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
        loss_sum[blockIdx.x] = t;
    }
}

// dx[r][k] = sum_c dlogit(r,c) * W[c][k];  dlogits written for host dW/db.
template <typename T>
__global__ void head_loss_bwd_kernel(const float* __restrict__ sig,
                                     const float* __restrict__ y,
                                     const float* __restrict__ wgt,
                                     const float* __restrict__ pw,
                                     const float* __restrict__ gscale,
                                     const T* __restrict__ W,
                                     float* __restrict__ dlogits,
                                     T* __restrict__ dx, int B, int K, int C) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * K) return;
    const int r = idx / K, k = idx % K;
    const float g = *gscale / (float)(B * C);
    float acc = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float s = sig[r * C + c];
        const float yy = y[r * C + c];
        const float dl = g * wgt[c] * (s * (1.0f - yy + pw[c] * yy) -
                                       pw[c] * yy);
        if (k == 0) dlogits[r * C + c] = dl;
        acc += dl * to_f32<T>(W[(long)c * K + k]);
    }
    dx[idx] = from_f32<T>(acc);
}

extern "C" int fmda_head_fwd_launch(int is_bf16, const void* x, const void* W,
                                    const void* bias, const float* y,
                                    const float* wgt, const float* pw,
                                    float* logits, float* sig,
                                    float* loss_sum, int B, int K, int C,
                                    hipStream_t stream) {
    const int n = B * C;
    const dim3 grid((n + 255) / 256);
    if (is_bf16)
        head_loss_fwd_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
            (const __hip_bfloat16*)x, (const __hip_bfloat16*)W,
            (const __hip_bfloat16*)bias, y, wgt, pw, logits, sig, loss_sum,
            B, K, C);
    else
        head_loss_fwd_kernel<float><<<grid, 256, 0, stream>>>(
            (const float*)x, (const float*)W, (const float*)bias, y, wgt, pw,
            logits, sig, loss_sum, B, K, C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int fmda_head_bwd_launch(int is_bf16, const float* sig,
                                    const float* y, const float* wgt,
                                    const float* pw, const float* gscale,
                                    const void* W, float* dlogits, void* dx,
                                    int B, int K, int C, hipStream_t stream) {
    const int n = B * K;
    const dim3 grid((n + 255) / 256);
    if (is_bf16)
        head_loss_bwd_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
            sig, y, wgt, pw, gscale, (const __hip_bfloat16*)W, dlogits,
            (__hip_bfloat16*)dx, B, K, C);
    else
        head_loss_bwd_kernel<float><<<grid, 256, 0, stream>>>(
            sig, y, wgt, pw, gscale, (const float*)W, dlogits, (float*)dx,
            B, K, C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// MFMA layout self-test.
// ===========================================================================
__global__ void mfma_selftest_kernel(const __hip_bfloat16* __restrict__ A,
                                     const __hip_bfloat16* __restrict__ Bm,
                                     float* __restrict__ C) {
    const int lane = threadIdx.x & 63;
    bf16x8_t a, b;
    const __bf16* ap = (const __bf16*)A;
    const __bf16* bp = (const __bf16*)Bm;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        a[e] = ap[(lane & 15) * 32 + 8 * (lane >> 4) + e];
        b[e] = bp[(8 * (lane >> 4) + e) * 16 + (lane & 15)];
    }
    f32x4_t acc = f32x4_t{0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
#pragma unroll
    for (int v = 0; v < 4; ++v)
        C[(4 * (lane >> 4) + v) * 16 + (lane & 15)] = acc[v];
}

// ===========================================================================
// Host launchers.
// ===========================================================================

// Tile / LDS-residency policy of the generic kernels, one row per (dtype, Hp)
// they serve: X(is_bf16, Hp, BT, WLDS, NT). The forward dispatch, the
// backward dispatch and the partials-table row count all expand this list.
// bf16 Hp=128 is not here: it runs the v3 kernels.
#define FMDA_GRU_GENERIC_ROWS(X)                                               \
    X(1, 32, 32, true, 256)                                                    \
    X(1, 64, 32, true, 256)                                                    \
    X(1, 256, 32, false, 512)                                                  \
    X(1, 512, 16, false, 512)                                                  \
    X(0, 16, 32, false, 256)                                                   \
    X(0, 32, 32, false, 256)                                                   \
    X(0, 64, 32, false, 256)                                                   \
    X(0, 128, 32, false, 256)                                                  \
    X(0, 256, 16, false, 256)                                                  \
    X(0, 512, 16, false, 256)

template <int BF>
using row_t = std::conditional_t<BF != 0, __hip_bfloat16, float>;

template <typename T, int BT, int Hp, bool WLDS, int NT>
static int launch_fwd(const void* gi, const void* w, const float* bhh,
                      void* out, float* hlast, int B, int Tseq, int n_dir,
                      const float* h0, long gi_pitch, hipStream_t stream) {
    constexpr size_t lds = FwdLds<T, BT, Hp, WLDS>::bytes;
    auto k = gru_fwd_kernel<T, BT, Hp, WLDS, NT>;
    (void)hipFuncSetAttribute((const void*)k,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 grid((B + BT - 1) / BT, n_dir);
    k<<<grid, NT, lds, stream>>>((const T*)gi, (const T*)w, bhh, (T*)out,
                                 hlast, B, Tseq, n_dir, h0, gi_pitch);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

template <typename T, int BT, int Hp, bool WLDS, int NT>
static int launch_bwd(const void* gi, const void* w, const float* bhh,
                      const void* out, const void* dout, const float* dhT,
                      void* dgi, void* dgh, float* dh0, float* dbhh, int B,
                      int Tseq, int n_dir, const float* h0, void* dgh0,
                      hipStream_t stream) {
    // fp32 BPTT at Hp=512 would need ~264 KB of LDS: there is no such
    // kernel, and the branch keeps the table's forward-only row from
    // instantiating one.
    if constexpr (sizeof(T) == 4 && Hp > 256) {
        return -3;
    } else {
        constexpr size_t lds = BwdLds<T, BT, Hp, WLDS>::bytes;
        auto k = gru_bwd_kernel<T, BT, Hp, WLDS, NT>;
        (void)hipFuncSetAttribute((const void*)k,
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        const dim3 grid((B + BT - 1) / BT, n_dir);
        k<<<grid, NT, lds, stream>>>((const T*)gi, (const T*)w, bhh,
                                     (const T*)out, (const T*)dout, dhT,
                                     (T*)dgi, (T*)dgh, dh0, dbhh, B, Tseq,
                                     n_dir, h0, (T*)dgh0);
        return hipGetLastError() == hipSuccess ? 0 : -4;
    }
}

// Forward: BT=16 / NT=256, two 4-wave blocks per CU.
static int launch_fwd_v3_128(const void* gi, const void* w, const float* bhh,
                      void* out, float* hlast, int B, int Tseq, int n_dir,
                      const float* h0, void* out_drop, unsigned int drop_thr,
                      float drop_scale, unsigned long long drop_seed,
                      long gi_pitch, hipStream_t stream) {
    constexpr int BT = 16, Hp = 128, NT = 256;
    constexpr size_t lds = FwdV3Lds<BT, Hp>::bytes;
    auto k = gru_fwd_v3_kernel<BT, Hp, NT, 2>;
    (void)hipFuncSetAttribute((const void*)k,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 grid((B + BT - 1) / BT, n_dir);
    k<<<grid, NT, lds, stream>>>((const __hip_bfloat16*)gi,
                                 (const __hip_bfloat16*)w, bhh,
                                 (__hip_bfloat16*)out, hlast, B, Tseq, n_dir,
                                 h0, (__hip_bfloat16*)out_drop, drop_thr,
                                 drop_scale, drop_seed, gi_pitch);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// Backward: BT = BWD_V3_BT (32) / NT=512, one 8-wave block per CU. POOLED
// takes d_out and d_hlast from dfeat (row pitch ld elements) and amax inside
// the kernel, and dout / dhT / dropout from nowhere; dense takes no dfeat.
template <bool POOLED>
static int launch_bwd_v3(const void* gi, const void* w, const void* wt,
                         const float* bhh, const void* out, const void* dout,
                         const float* dhT, void* dgi, void* dgh, float* dh0,
                         float* dbhh, int B, int Tseq, int n_dir,
                         unsigned int drop_thr, float drop_scale,
                         unsigned long long drop_seed, const float* h0,
                         void* dgh0, const void* dfeat, const int* amax,
                         long ld, hipStream_t stream) {
    constexpr int BT = BWD_V3_BT, Hp = 128, NT = 512;
    constexpr size_t lds = BwdV3Lds<BT, Hp, POOLED>::bytes;
    auto k = gru_bwd_v3_kernel<BT, Hp, NT, 2, POOLED>;
    (void)hipFuncSetAttribute((const void*)k,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 grid((B + BT - 1) / BT, n_dir);
    k<<<grid, NT, lds, stream>>>(
        (const __hip_bfloat16*)gi, (const __hip_bfloat16*)w,
        (const __hip_bfloat16*)wt, bhh,
        (const __hip_bfloat16*)out, (const __hip_bfloat16*)dout, dhT,
        (__hip_bfloat16*)dgi, (__hip_bfloat16*)dgh, dh0, dbhh, B, Tseq,
        n_dir, drop_thr, drop_scale, drop_seed, h0,
        (__hip_bfloat16*)dgh0, (const __hip_bfloat16*)dfeat, amax, ld);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

static int launch_bwd_v3_128(const void* gi, const void* w, const void* wt,
                      const float* bhh, const void* out, const void* dout,
                      const float* dhT, void* dgi, void* dgh, float* dh0,
                      float* dbhh, int B, int Tseq, int n_dir,
                      unsigned int drop_thr, float drop_scale,
                      unsigned long long drop_seed, const float* h0,
                      void* dgh0, hipStream_t stream) {
    return launch_bwd_v3<false>(gi, w, wt, bhh, out, dout, dhT, dgi, dgh,
                                dh0, dbhh, B, Tseq, n_dir, drop_thr,
                                drop_scale, drop_seed, h0, dgh0, nullptr,
                                nullptr, 0L, stream);
}

// Dynamic LDS of a batch-1 / streams / bank launch, or 0 when the sequence is
// too long to stay LDS-resident (150 KB cap).
template <int Hp>
static size_t b1_lds_bytes(int Tseq) {
    if (Tseq < 0) return 0;
    const size_t lds = (size_t)B1Lds<Hp>(Tseq).bytes;
    return lds > 150 * 1024 ? 0 : lds;
}

extern "C" int fmda_gru_fwd_b1_launch(const void* gi, const void* w,
                                      const float* bhh, void* out,
                                      float* hlast, int Tseq, int n_dir,
                                      const float* h0, hipStream_t stream) {
    constexpr int Hp = 128;
    const size_t lds = b1_lds_bytes<Hp>(Tseq);
    if (lds == 0) return -5;   // sequence too long for LDS residency
    // A/B note: a 2-wave NT=128 variant (halved barrier width, CPW 4) was
    // measured 1.75x SLOWER — the doubled wA fragment hoist (192 VGPRs)
    // blows the register budget and the spill reloads dominate. 4 waves
    // with CPW=2 stays the right split.
    auto k = gru_fwd_b1_kernel<Hp, 256>;
    (void)hipFuncSetAttribute((const void*)k,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    k<<<dim3(n_dir), 256, lds, stream>>>(
        (const __hip_bfloat16*)gi, (const __hip_bfloat16*)w, bhh,
        (__hip_bfloat16*)out, hlast, Tseq, n_dir, h0);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// S streams on a (n_dir, S) grid; same LDS requirement and cap as the
// batch-1 launch. Above the cap nothing is launched.
extern "C" int fmda_gru_fwd_streams_launch(const void* gi, const void* w,
                                           const float* bhh, void* out,
                                           float* hlast, int S, int Tseq,
                                           int n_dir, hipStream_t stream) {
    constexpr int Hp = 128;
    const size_t lds = b1_lds_bytes<Hp>(Tseq);
    if (lds == 0) return -5;   // sequence too long for LDS residency
    if (S < 1 || S > 65535) return -1;   // gridDim.y
    auto k = gru_fwd_streams_kernel<Hp, 256>;
    (void)hipFuncSetAttribute((const void*)k,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    k<<<dim3(n_dir, S), 256, lds, stream>>>(
        (const __hip_bfloat16*)gi, (const __hip_bfloat16*)w, bhh,
        (__hip_bfloat16*)out, hlast, Tseq, n_dir);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// The same launch over a bank of M models; slot is int32 (S) on the device.
extern "C" int fmda_gru_fwd_streams_bank_launch(
        const void* gi, const int* slot, int M, const void* w,
        const float* bhh, void* out, float* hlast, int S, int Tseq,
        int n_dir, hipStream_t stream) {
    constexpr int Hp = 128;
    const size_t lds = b1_lds_bytes<Hp>(Tseq);
    if (lds == 0) return -5;   // sequence too long for LDS residency
    if (S < 1 || S > 65535 || M < 1) return -1;   // gridDim.y
    auto k = gru_fwd_streams_bank_kernel<Hp, 256>;
    (void)hipFuncSetAttribute((const void*)k,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    k<<<dim3(n_dir, S), 256, lds, stream>>>(
        (const __hip_bfloat16*)gi, slot, M, (const __hip_bfloat16*)w, bhh,
        (__hip_bfloat16*)out, hlast, Tseq, n_dir);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// Grouped input projection; the load width follows what K and the base
// pointers keep aligned (see gi_proj_bank_kernel).
extern "C" int fmda_gi_proj_bank_launch(const void* x, const int* slot,
                                        const void* W, const void* b,
                                        void* gi, int S, int Tseq, int K,
                                        int N, int M, hipStream_t stream) {
    if (S < 1 || S > 65535 || Tseq < 1 || K < 1 || M < 1 || N < 16 ||
        N % 16 != 0)
        return -1;
    if (((uintptr_t)gi & 7) != 0) return -1;     // 8-byte stores
    const uintptr_t a = (uintptr_t)x | (uintptr_t)W;
    const int row_tiles = (Tseq - 1) / 32 + 1;
    if (row_tiles > 65535) return -1;            // gridDim.z
    const dim3 grid((N + 255) / 256, S, row_tiles);
#define FMDA_GI_BANK(VEC)                                                    \
    gi_proj_bank_kernel<VEC><<<grid, 256, 0, stream>>>(                      \
        (const __hip_bfloat16*)x, slot, (const __hip_bfloat16*)W,            \
        (const __hip_bfloat16*)b, (__hip_bfloat16*)gi, Tseq, K, N, M)
    if (K % 8 == 0 && (a & 15) == 0) FMDA_GI_BANK(8);
    else if (K % 4 == 0 && (a & 7) == 0) FMDA_GI_BANK(4);
    else FMDA_GI_BANK(1);
#undef FMDA_GI_BANK
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

extern "C" int fmda_gru_fwd_launch(int is_bf16, int Hp, const void* gi,
                                   const void* w, const float* bhh, void* out,
                                   float* hlast, int B, int Tseq, int n_dir,
                                   const float* h0, void* out_drop,
                                   unsigned int drop_thr, float drop_scale,
                                   unsigned long long drop_seed,
                                   long gi_pitch, hipStream_t stream) {
    if (out_drop != nullptr && !(is_bf16 && Hp == 128))
        return -6;   // fused fwd dropout only on the bf16 Hp=128 path
    if (is_bf16 && Hp == 16)
        return -7;   // KK = Hp/32 = 0: zero-trip MFMA loop
    if (is_bf16 && Hp == 128) {
        if (B == 1 && out_drop == nullptr &&
            fmda_gru_fwd_b1_launch(gi, w, bhh, out, hlast, Tseq, n_dir, h0,
                                   stream) == 0)
            return 0;   // LDS-resident batch-1 kernel took it
        return launch_fwd_v3_128(gi, w, bhh, out, hlast, B, Tseq, n_dir, h0,
                                 out_drop, drop_thr, drop_scale, drop_seed,
                                 gi_pitch, stream);
    }
#define X(BF, HPV, BTV, WL, NTV)                                               \
    if ((is_bf16 != 0) == (BF != 0) && Hp == HPV)                              \
        return launch_fwd<row_t<BF>, BTV, HPV, WL, NTV>(                       \
            gi, w, bhh, out, hlast, B, Tseq, n_dir, h0, gi_pitch, stream);
    FMDA_GRU_GENERIC_ROWS(X)
#undef X
    return -1;
}

extern "C" int fmda_gru_bwd_cs_launch(const void* gi, const void* w,
                                      const void* wt, const float* bhh,
                                      const void* out, const void* dout,
                                      const float* dhT, void* dgi, void* dgh,
                                      float* dh0, float* dbhh, void* gpub,
                                      unsigned int* cnt, int B, int Tseq,
                                      int n_dir, unsigned int drop_thr,
                                      float drop_scale,
                                      unsigned long long drop_seed,
                                      hipStream_t stream) {
    constexpr int BR = CS_BR, Hp = 512, CS = 32, NT = CS_NT;
    const int GB = (B + BR - 1) / BR;
    constexpr size_t lds = CsLds<BR, Hp, CS>::bytes;
    auto k = gru_bwd_cs_kernel<BR, Hp, CS, NT>;
    (void)hipFuncSetAttribute((const void*)k,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 grid(GB * (Hp / CS) * n_dir);
    k<<<grid, NT, lds, stream>>>(
        (const __hip_bfloat16*)gi, (const __hip_bfloat16*)w,
        (const __hip_bfloat16*)wt, bhh, (const __hip_bfloat16*)out,
        (const __hip_bfloat16*)dout, dhT, (__hip_bfloat16*)dgi,
        (__hip_bfloat16*)dgh, dh0, dbhh, (__hip_bfloat16*)gpub, cnt, B,
        Tseq, n_dir, GB, drop_thr, drop_scale, drop_seed);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Rows of the bias-grad partials table (rows, n_dir, 4Hp) that the backward
// launch for this shape writes: one per batch tile (grid.x of the
// batch-parallel kernels), or one per (batch group, wave) for the
// column-split kernel. 0 for a shape no backward kernel serves.
extern "C" int fmda_gru_bwd_db_rows(int is_bf16, int Hp, int B,
                                    int column_split) {
    if (column_split) return (CS_NT / 64) * ((B + CS_BR - 1) / CS_BR);
    int bt = 0;
    if (is_bf16 && Hp == 128) bt = BWD_V3_BT;
#define X(BF, HPV, BTV, WL, NTV)                                               \
    if ((is_bf16 != 0) == (BF != 0) && Hp == HPV) bt = BTV;
    FMDA_GRU_GENERIC_ROWS(X)
#undef X
    return bt ? (B + bt - 1) / bt : 0;
}

// Sums the partials table (rows, n_dir, 4Hp) over rows in a fixed order and
// scatters the packed slots [dr, dz, dhn | dn] straight into db_hh (slots
// 0..2) and db_ih (slots 0,1,3), both (n_dir, 3Hp). 64 columns per block,
// DB_RG waves striding the rows, combined through LDS in wave order.
constexpr int DB_RG = 16;
__global__ void db_reduce_kernel(const float* __restrict__ part, int rows,
                                 int n_dir, int Hp,
                                 float* __restrict__ dbhh,
                                 float* __restrict__ dbih) {
    __shared__ float red[DB_RG][64];
    const int ncol = n_dir * 4 * Hp;
    const int col = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rg = threadIdx.x >> 6;
    float s = 0.0f;
    if (col < ncol) {
        // independent loads issued ahead of the (ordered) adds
#pragma unroll 8
        for (int r = rg; r < rows; r += DB_RG)
            s += part[(long)r * ncol + col];
    }
    red[rg][threadIdx.x & 63] = s;
    __syncthreads();
    if (rg == 0 && col < ncol) {
        float t = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < DB_RG; ++k) t += red[k][threadIdx.x];
        const int dir = col / (4 * Hp);
        const int g = (col % (4 * Hp)) / Hp;
        const int j = col % Hp;
        if (g < 3) dbhh[(long)dir * 3 * Hp + g * Hp + j] = t;
        if (g != 2)
            dbih[(long)dir * 3 * Hp + (g == 3 ? 2 : g) * Hp + j] = t;
    }
}

extern "C" int fmda_gru_db_reduce_launch(const float* part, int rows,
                                         int n_dir, int Hp, float* dbhh,
                                         float* dbih, hipStream_t stream) {
    const int ncol = n_dir * 4 * Hp;
    db_reduce_kernel<<<dim3((ncol + 63) / 64), 64 * DB_RG, 0, stream>>>(
        part, rows, n_dir, Hp, dbhh, dbih);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int fmda_gru_bwd_launch(int is_bf16, int Hp, const void* gi,
                                   const void* w, const void* wt,
                                   const float* bhh,
                                   const void* out, const void* dout,
                                   const float* dhT, void* dgi, void* dgh,
                                   float* dh0, float* dbhh, int B, int Tseq,
                                   int n_dir, unsigned int drop_thr,
                                   float drop_scale,
                                   unsigned long long drop_seed,
                                   const float* h0, void* dgh0,
                                   hipStream_t stream) {
    if (!is_bf16 && Hp > 256) return -3;
    if (drop_thr != 0u && !(is_bf16 && Hp == 128))
        return -6;   // fused dropout-backward only on the bf16 Hp=128 path
    if (is_bf16 && Hp == 16)
        return -7;   // KK = Hp/32 = 0: zero-trip MFMA loop
    if (is_bf16 && Hp == 128)
        return launch_bwd_v3_128(gi, w, wt, bhh, out, dout, dhT, dgi, dgh,
                                 dh0, dbhh, B, Tseq, n_dir, drop_thr,
                                 drop_scale, drop_seed, h0, dgh0, stream);
#define X(BF, HPV, BTV, WL, NTV)                                               \
    if ((is_bf16 != 0) == (BF != 0) && Hp == HPV)                              \
        return launch_bwd<row_t<BF>, BTV, HPV, WL, NTV>(                       \
            gi, w, bhh, out, dout, dhT, dgi, dgh, dh0, dbhh, B, Tseq, n_dir,   \
            h0, dgh0, stream);
    FMDA_GRU_GENERIC_ROWS(X)
#undef X
    return -1;
}

// Backward of a bf16 Hp=128 layer whose out feeds pool_features_fwd alone:
// d_out / d_hlast are synthesised in the kernel from dfeat (B, 3Hp) with
// row pitch ld (elements, a multiple of 8 on a 16-byte aligned base) and
// amax (B, Hp). One byte per amax entry: Tseq <= 256. No dropout.
extern "C" int fmda_gru_bwd_pooled_launch(const void* gi, const void* w,
                                          const void* wt, const float* bhh,
                                          const void* out, const void* dfeat,
                                          const int* amax, long ld, void* dgi,
                                          void* dgh, float* dh0, float* dbhh,
                                          int B, int Tseq, int n_dir,
                                          const float* h0, void* dgh0,
                                          hipStream_t stream) {
    if (Tseq < 1 || Tseq > 256 || ld < 3 * 128 || ld % 8 != 0) return -9;
    return launch_bwd_v3<true>(gi, w, wt, bhh, out, nullptr, nullptr, dgi,
                               dgh, dh0, dbhh, B, Tseq, n_dir, 0u, 1.0f, 0ull,
                               h0, dgh0, dfeat, amax, ld, stream);
}

extern "C" int fmda_mfma_selftest_launch(const void* A, const void* Bm,
                                         float* C, hipStream_t stream) {
    mfma_selftest_kernel<<<1, 64, 0, stream>>>((const __hip_bfloat16*)A,
                                               (const __hip_bfloat16*)Bm, C);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace fmda