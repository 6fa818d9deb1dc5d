// fmda_amd glue kernels for MI355X (gfx950): the small per-step passes
// around the recurrence and the library GEMMs, each done in one launch.
//
// A training step re-derives everything below from the fp32 master weights
// (Adam moves them every step), so none of it can be cached:
//   pack_gru_layer       masters -> padded, direction-stacked compute-dtype
//                        weights (+ W_hh^T for the BPTT carry GEMM)
//   finalize_gru_wgrads  split-K GEMM partials -> the four master-shaped
//                        fp32 weight gradients of a layer
//   head_*_master        classifier head + loss reading the fp32 masters
//   head_wgrads          dW / db of the head, two-stage over the batch
//   *_eager kernels      the two weight-grad reductions over 64 split-K
//                        chunks in the order of torch's own sum: the eager
//                        chain's bits in one launch
//   subset_accuracy      the step's exact-match metric in one launch
// All sums run in a fixed order: results are bitwise reproducible.
// Inference side: normalize_table, the raw (N, F) table -> normalised
// compute-dtype table in one pass (windowed evaluation of whole chunks).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdint>

#include "dropout_common.h"   // mix64, drop_hit, drop_apply
#include "fmda_launch.h"

#define FMDA_DEV __device__ __forceinline__

namespace fmda {
namespace {

#define FMDA_LOG2E 1.4426950408889634f

FMDA_DEV float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
FMDA_DEV float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
// same formula as the head kernels in gru_kernels.hip (bit-identical sig)
FMDA_DEV float sigmoidf(float x) {
    return fast_rcp(1.0f + fast_exp2(-x * FMDA_LOG2E));
}

template <typename T> FMDA_DEV float to_f32(T v);
template <> FMDA_DEV float to_f32<float>(float v) { return v; }
template <> FMDA_DEV float to_f32<__hip_bfloat16>(__hip_bfloat16 v) {
    return __bfloat162float(v);
}
template <typename T> FMDA_DEV T from_f32(float v);
template <> FMDA_DEV float from_f32<float>(float v) { return v; }
template <> FMDA_DEV __hip_bfloat16 from_f32<__hip_bfloat16>(float v) {
    return __float2bfloat16(v);   // round to nearest even, like .to(bf16)
}
// fp32 master value as the compute dtype sees it
template <typename T> FMDA_DEV float round_to(float v) {
    return to_f32<T>(from_f32<T>(v));
}
// 16 bytes moved as one vector load / store
struct alignas(16) chunk16 { unsigned int u[4]; };

// ===========================================================================
// pack_gru_layer
// ===========================================================================
struct GruMasters {
    const float* w_ih[2];   // (3H, F)
    const float* w_hh[2];   // (3H, H)
    const float* b_ih[2];   // (3H)
    const float* b_hh[2];   // (3H)
};

// One flat index space over the five outputs, walked grid-stride. Padded
// gate row g*Hp + j reads master row g*H + j; rows j >= H and recurrent
// columns >= H are zero.
template <typename T>
__global__ void pack_gru_layer_kernel(GruMasters m, T* __restrict__ w_ih_cat,
                                      T* __restrict__ b_ih_cat,
                                      T* __restrict__ w_hh_cat,
                                      float* __restrict__ b_hh_cat,
                                      T* __restrict__ wt, int D, int H,
                                      int Hp, int F) {
    const long G3 = 3L * Hp;
    const long n_ih = (long)D * G3 * F;
    const long n_hh = (long)D * G3 * Hp;
    const long n_b = (long)D * G3;
    const long total = n_ih + 2 * n_hh + 2 * n_b;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += stride) {
        if (i < n_ih) {
            const int d = (int)(i / (G3 * F));
            const long rem = i % (G3 * F);
            const int row = (int)(rem / F), col = (int)(rem % F);
            const int g = row / Hp, j = row % Hp;
            const float v =
                j < H ? m.w_ih[d][((long)g * H + j) * F + col] : 0.0f;
            w_ih_cat[i] = from_f32<T>(v);
        } else if (i < n_ih + n_hh) {
            const long o = i - n_ih;
            const int d = (int)(o / (G3 * Hp));
            const long rem = o % (G3 * Hp);
            const int row = (int)(rem / Hp), col = (int)(rem % Hp);
            const int g = row / Hp, j = row % Hp;
            const float v = (j < H && col < H)
                ? m.w_hh[d][((long)g * H + j) * H + col] : 0.0f;
            w_hh_cat[o] = from_f32<T>(v);
        } else if (i < n_ih + 2 * n_hh) {
            // wt[d][k][n] = w_hh_cat[d][n][k]
            const long o = i - n_ih - n_hh;
            const int d = (int)(o / (G3 * Hp));
            const long rem = o % (G3 * Hp);
            const int k = (int)(rem / G3), n = (int)(rem % G3);
            const int g = n / Hp, j = n % Hp;
            const float v = (j < H && k < H)
                ? m.w_hh[d][((long)g * H + j) * H + k] : 0.0f;
            wt[o] = from_f32<T>(v);
        } else {
            long o = i - n_ih - 2 * n_hh;
            const bool hh = o >= n_b;
            if (hh) o -= n_b;
            const int d = (int)(o / G3);
            const int row = (int)(o % G3);
            const int g = row / Hp, j = row % Hp;
            const float* src = hh ? m.b_hh[d] : m.b_ih[d];
            const float v = j < H ? src[g * H + j] : 0.0f;
            if (hh) b_hh_cat[o] = v;
            else b_ih_cat[o] = from_f32<T>(v);
        }
    }
}

// ===========================================================================
// finalize_gru_wgrads
// ===========================================================================
struct GruWgrads {
    float* dw_ih[2];   // (3H, F)
    float* dw_hh[2];   // (3H, H)
};

// One thread per output element. part_ih: (c_ih, D*3Hp, F) partials of
// dGi^T x; part_hh: (c_hh, D*3Hp, D*Hp) partials of dGh^T out, of which
// only the diagonal direction blocks are read. Chunks are summed in fp32 in
// ascending order; gate rows (and dW_hh columns) are unpadded on the way.
template <typename PT>
__global__ void finalize_gru_wgrads_kernel(const PT* __restrict__ part_ih,
                                           int c_ih,
                                           const PT* __restrict__ part_hh,
                                           int c_hh, GruWgrads o, int D,
                                           int H, int Hp, int F) {
    const long n_ih = 3L * H * F;
    const long n_hh = 3L * H * H;
    const long per_dir = n_ih + n_hh;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)D * per_dir) return;
    const int d = (int)(idx / per_dir);
    const long r = idx % per_dir;
    float acc = 0.0f;
    if (r < n_ih) {
        const int row = (int)(r / F), col = (int)(r % F);
        const long prow = (long)d * 3 * Hp + (long)(row / H) * Hp + row % H;
        const PT* p = part_ih + prow * F + col;
        const long cs = (long)D * 3 * Hp * F;
#pragma unroll 8
        for (int k = 0; k < c_ih; ++k) acc += to_f32<PT>(p[k * cs]);
        o.dw_ih[d][r] = acc;
    } else {
        const long q = r - n_ih;
        const int row = (int)(q / H), col = (int)(q % H);
        const long prow = (long)d * 3 * Hp + (long)(row / H) * Hp + row % H;
        const long pitch = (long)D * Hp;
        const PT* p = part_hh + prow * pitch + (long)d * Hp + col;
        const long cs = (long)D * 3 * Hp * pitch;
#pragma unroll 8
        for (int k = 0; k < c_hh; ++k) acc += to_f32<PT>(p[k * cs]);
        o.dw_hh[d][q] = acc;
    }
}

// ---------------------------------------------------------------------------
// The same reductions in the order of torch's `parts.float().sum(dim=0)`
// for c = 64 chunks, so the result equals the eager chain bit for bit.
// ATen's reduce kernel (slow-dimension reduction, contiguous outputs, at
// least 512 of them and a multiple of 4) runs a 64 x 2 block: row y of the
// block takes the chunks k = y + 2m, m = 0..31, in four accumulators that
// start at 0.0f, accumulator i taking m = i (mod 4) in ascending m; the
// accumulators are combined as ((a0 + a1) + a2) + a3 and the two rows are
// added once. The launchers' callers check those conditions.
// ---------------------------------------------------------------------------
constexpr int EAGER_SUM_CHUNKS = 64;

template <int BYTES> struct raw_vec;
template <> struct raw_vec<2> { using type = unsigned short; };
template <> struct raw_vec<4> { using type = unsigned int; };
template <> struct raw_vec<8> { using type = uint2; };
template <> struct raw_vec<16> { using type = uint4; };

// out[j] = sum over the 64 chunks of p[k * cs + j], j < V, in that order.
// p + k * cs is aligned to V elements.
template <typename PT, int V>
FMDA_DEV void eager_order_sum64(const PT* __restrict__ p, long cs,
                                float (&out)[V]) {
    using raw_t = typename raw_vec<V * (int)sizeof(PT)>::type;
    float row[2][V];
#pragma unroll
    for (int y = 0; y < 2; ++y) {
        float a[4][V];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < V; ++j) a[i][j] = 0.0f;
#pragma unroll
        for (int n = 0; n < EAGER_SUM_CHUNKS / 8; ++n) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                alignas(V * sizeof(PT)) PT v[V];
                *(raw_t*)v = *(const raw_t*)(p + (y + 2 * (4 * n + i)) * cs);
#pragma unroll
                for (int j = 0; j < V; ++j) a[i][j] += to_f32<PT>(v[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j)
            row[y][j] = ((a[0][j] + a[1][j]) + a[2][j]) + a[3][j];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) out[j] = row[0][j] + row[1][j];
}

// finalize_gru_wgrads_kernel with eager_order_sum64 over c = 64 chunks of
// both partials. One thread per V consecutive outputs of one row (V divides
// H and F, so a vector never leaves its row).
template <typename PT, int V>
__global__ void __launch_bounds__(256) finalize_gru_wgrads_eager_kernel(
        const PT* __restrict__ part_ih, const PT* __restrict__ part_hh,
        GruWgrads o, int D, int H, int Hp, int F) {
    const long n_ih = 3L * H * F;
    const long n_hh = 3L * H * H;
    const long per_dir = n_ih + n_hh;
    const long idx = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (idx >= (long)D * per_dir) return;
    const int d = (int)(idx / per_dir);
    const long r = idx % per_dir;
    float acc[V];
    float* dst;
    if (r < n_ih) {
        const int row = (int)(r / F), col = (int)(r % F);
        const long prow = (long)d * 3 * Hp + (long)(row / H) * Hp + row % H;
        eager_order_sum64<PT, V>(part_ih + prow * F + col,
                                 (long)D * 3 * Hp * F, acc);
        dst = o.dw_ih[d] + r;
    } else {
        const long q = r - n_ih;
        const int row = (int)(q / H), col = (int)(q % H);
        const long prow = (long)d * 3 * Hp + (long)(row / H) * Hp + row % H;
        const long pitch = (long)D * Hp;
        eager_order_sum64<PT, V>(part_hh + prow * pitch + (long)d * Hp + col,
                                 (long)D * 3 * Hp * pitch, acc);
        dst = o.dw_hh[d] + q;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) dst[j] = acc[j];
}

// Head weight grads from the (64, C, K) split-K partials of
// round_T(dlogits)^T x: dW = fp32(T(sum of the chunks in the eager order)),
// and db = fp32(T(db_sum)) for the batch sum torch already made. That is
// chunked_outer(...).to(fp32) and dlogits.sum(0).to(T).to(fp32).
template <typename T>
__global__ void head_wgrads_eager_kernel(const T* __restrict__ parts,
                                         const float* __restrict__ db_sum,
                                         float* __restrict__ dW,
                                         float* __restrict__ db, int n_w,
                                         int C) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n_w) {
        float s[1];
        eager_order_sum64<T, 1>(parts + idx, (long)n_w, s);
        dW[idx] = round_to<T>(s[0]);
    } else if (idx < n_w + C) {
        db[idx - n_w] = round_to<T>(db_sum[idx - n_w]);
    }
}

// ===========================================================================
// Classifier head + BCEWithLogitsLoss(weight, pos_weight) on the fp32
// master W / b. The arithmetic is head_loss_{fwd,bwd}_kernel's
// (gru_kernels.hip) with each master value rounded to the compute dtype T
// in registers, so logits, sig, loss and dx are bit-identical to casting W
// and b first.
// ===========================================================================
template <typename T>
__global__ void head_fwd_master_kernel(const T* __restrict__ x,
                                       const float* __restrict__ W,
                                       const float* __restrict__ bias,
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
        const float* wr = W + (long)c * K;
        float acc = round_to<T>(bias[c]);
        for (int k = 0; k < K; ++k)
            acc += to_f32<T>(xr[k]) * round_to<T>(wr[k]);
        logits[idx] = acc;
        const float s = sigmoidf(acc);
        sig[idx] = s;
        const float yy = y[idx];
        const float m = acc > 0.0f ? acc : 0.0f;
        const float lse = m + __builtin_logf(fast_exp2(-m * FMDA_LOG2E) +
                                             fast_exp2((acc - m) * FMDA_LOG2E));
        const float log_s = acc - lse;
        const float log_1ms = -lse;
        l = -wgt[c] * (pw[c] * yy * log_s + (1.0f - yy) * log_1ms);
    }
    // one partial per block, summed by the caller in a fixed order
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

// head_fwd_master_kernel with its operands staged in LDS. The mapping of
// threads to (row, class), each thread's serial chain over ascending k, the
// loss expression and the block's butterfly are those of the kernel above,
// so logits, sig and every block partial are the same bits. What differs is
// where the chain reads from: above, a wave's lanes walk 64/C rows that lie
// K*sizeof(T) bytes apart, one element per load. Here the block copies its
// rows of x (contiguous in memory) into LDS with coalesced 16-byte loads,
// KT columns at a time, next to the rounded W tile, and the chains run from
// LDS 16 bytes per read. Row pitches are padded (16 bytes for x, 4 floats
// for W) to spread the rows over the banks.
// Dynamic LDS: rows_cap * (KT*sizeof(T) + 16) + C * (KT + 4) * 4 bytes.
// K and KT are multiples of 16/sizeof(T); x is 16-byte aligned.
template <typename T>
__global__ void head_fwd_master_staged_kernel(
        const T* __restrict__ x, const float* __restrict__ W,
        const float* __restrict__ bias, const float* __restrict__ y,
        const float* __restrict__ wgt, const float* __restrict__ pw,
        float* __restrict__ logits, float* __restrict__ sig,
        float* __restrict__ loss_sum, int B, int K, int C, int KT,
        int rows_cap) {
    constexpr int V = 16 / (int)sizeof(T);
    extern __shared__ __align__(16) unsigned char head_smem[];
    const int xpitch = KT * (int)sizeof(T) + 16;   // bytes
    const int wpitch = KT + 4;                     // floats
    unsigned char* xs = head_smem;
    float* ws = (float*)(head_smem + (size_t)rows_cap * xpitch);

    const int first = blockIdx.x * blockDim.x;     // < B * C by the grid
    const int idx = first + threadIdx.x;
    const int last = min(first + (int)blockDim.x, B * C) - 1;
    const int r0 = first / C;
    const int nrows = last / C - r0 + 1;           // <= rows_cap
    const bool valid = idx < B * C;
    const int r = valid ? idx / C : r0, c = valid ? idx % C : 0;
    float acc = round_to<T>(bias[c]);
    for (int k0 = 0; k0 < K; k0 += KT) {
        const int kt = min(KT, K - k0);
        const int cpr = kt / V;                    // 16-byte chunks per row
        if (k0 > 0) __syncthreads();               // the last tile is read
        for (int j = threadIdx.x; j < nrows * cpr; j += blockDim.x) {
            const int row = j / cpr, cc = j % cpr;
            *(chunk16*)(xs + row * xpitch + cc * 16) =
                *(const chunk16*)(x + (long)(r0 + row) * K + k0 + cc * V);
        }
        for (int j = threadIdx.x; j < C * kt; j += blockDim.x) {
            const int cw = j / kt, kk = j % kt;
            ws[cw * wpitch + kk] = round_to<T>(W[(long)cw * K + k0 + kk]);
        }
        __syncthreads();
        if (valid) {
            const unsigned char* xr = xs + (r - r0) * xpitch;
            const float* wr = ws + c * wpitch;
            for (int kk = 0; kk < kt; kk += V) {
                alignas(16) T xv[V];
                alignas(16) float wv[V];
                *(chunk16*)xv = *(const chunk16*)(xr + kk * (int)sizeof(T));
#pragma unroll
                for (int q = 0; q < V / 4; ++q)
                    *(chunk16*)(wv + 4 * q) =
                        *(const chunk16*)(wr + kk + 4 * q);
                // the direct kernel's `acc += x * w` compiles to one fused
                // multiply-add per k; written out here, because with the
                // operands in vectors the compiler would otherwise pair the
                // products into packed multiplies and round them
#pragma unroll
                for (int j = 0; j < V; ++j)
                    acc = __builtin_fmaf(to_f32<T>(xv[j]), wv[j], acc);
            }
        }
    }
    float l = 0.0f;
    if (valid) {
        logits[idx] = acc;
        const float s = sigmoidf(acc);
        sig[idx] = s;
        const float yy = y[idx];
        const float m = acc > 0.0f ? acc : 0.0f;
        const float lse = m + __builtin_logf(fast_exp2(-m * FMDA_LOG2E) +
                                             fast_exp2((acc - m) * FMDA_LOG2E));
        const float log_s = acc - lse;
        const float log_1ms = -lse;
        l = -wgt[c] * (pw[c] * yy * log_s + (1.0f - yy) * log_1ms);
    }
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

template <typename T>
__global__ void head_bwd_master_kernel(const float* __restrict__ sig,
                                       const float* __restrict__ y,
                                       const float* __restrict__ wgt,
                                       const float* __restrict__ pw,
                                       const float* __restrict__ gscale,
                                       const float* __restrict__ W,
                                       float* __restrict__ dlogits,
                                       T* __restrict__ dlogits_t,
                                       T* __restrict__ dx, int B, int K,
                                       int C) {
    // dlogits_t (may be null): dlogits rounded to T, the operand of the
    // dW GEMM, exactly dlogits.to(T)
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
        if (k == 0) {
            dlogits[r * C + c] = dl;
            if (dlogits_t != nullptr) dlogits_t[r * C + c] = from_f32<T>(dl);
        }
        acc += dl * round_to<T>(W[(long)c * K + k]);
    }
    dx[idx] = from_f32<T>(acc);
}

// ---------------------------------------------------------------------------
// head_wgrads: dW[c][k] = sum_r round_T(dlogits[r][c]) * x[r][k] and
// db[c] = sum_r dlogits[r][c], in fp32 and in two stages with a fixed
// order: stage 1 sums slabs of HEAD_SLAB batch rows, stage 2 sums the slabs.
// Both stages carry a compensation term (Neumaier), and stage 1 also keeps
// the fp32 rounding error of each product (zero for bf16 inputs, whose
// products are exact in fp32), so the result does not depend on B beyond
// the last bit or two.
// ---------------------------------------------------------------------------
constexpr int HEAD_SLAB = 64;

struct CompSum {
    float s = 0.0f, c = 0.0f;
    FMDA_DEV void add(float v) {
#pragma clang fp contract(off)
        const float t = s + v;
        // the smaller-magnitude operand's low bits are what t dropped
        c += fabsf(s) >= fabsf(v) ? (s - t) + v : (v - t) + s;
        s = t;
    }
    FMDA_DEV float value() const { return s + c; }
};

// grid (ceil(K/128), n_slabs, C), 128 threads: thread = one k column
template <typename T>
__global__ void head_wgrads_stage1_kernel(const float* __restrict__ dlogits,
                                          const T* __restrict__ x,
                                          float* __restrict__ dw_part,
                                          float* __restrict__ db_part, int B,
                                          int K, int C) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int slab = blockIdx.y, c = blockIdx.z;
    const int r0 = slab * HEAD_SLAB;
    const int r1 = min(r0 + HEAD_SLAB, B);
    CompSum dw, db;
#pragma unroll 8
    for (int r = r0; r < r1; ++r) {
#pragma clang fp contract(off)
        const float dl32 = dlogits[(long)r * C + c];
        const float dl = round_to<T>(dl32);
        const float xv = to_f32<T>(x[(long)r * K + k]);
        const float p = dl * xv;                 // rounded product ...
        dw.add(p);
        dw.c += __builtin_fmaf(dl, xv, -p);      // ... and what it dropped
        db.add(dl32);
    }
    dw_part[((long)slab * C + c) * K + k] = dw.value();
    if (k == 0) db_part[slab * C + c] = db.value();
}

// one thread per dW element, then C threads for db
__global__ void head_wgrads_stage2_kernel(const float* __restrict__ dw_part,
                                          const float* __restrict__ db_part,
                                          float* __restrict__ dW,
                                          float* __restrict__ db, int n_slabs,
                                          int K, int C) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int n_w = C * K;
    if (idx >= n_w + C) return;
    CompSum a;
    if (idx < n_w) {
#pragma unroll 8
        for (int s = 0; s < n_slabs; ++s) a.add(dw_part[(long)s * n_w + idx]);
        dW[idx] = a.value();
    } else {
        const int c = idx - n_w;
        for (int s = 0; s < n_slabs; ++s) a.add(db_part[s * C + c]);
        db[c] = a.value();
    }
}

// ===========================================================================
// subset_accuracy
// ===========================================================================
// Exact-match ratio of a (B, C) multilabel batch in one launch and one
// block: out = count(rows whose labels all match) * inv_b. The count is an
// integer, so the order it is summed in does not matter; the scaling is
// torch's mean, which multiplies the sum by the float 1/B (computed on the
// host). A target element counts as set when it is non-zero, like
// .to(torch.bool). TT: float or unsigned char (bool storage).
constexpr int SUBSET_ACC_THREADS = 1024;

template <typename TT>
__global__ void subset_accuracy_kernel(const TT* __restrict__ target,
                                       const unsigned char* __restrict__ pred,
                                       float* __restrict__ out, int B, int C,
                                       float inv_b) {
    int cnt = 0;
    for (int r = threadIdx.x; r < B; r += blockDim.x) {
        const TT* t = target + (long)r * C;
        const unsigned char* p = pred + (long)r * C;
        bool all = true;
        for (int c = 0; c < C; ++c)
            all = all && ((t[c] != (TT)0) == (p[c] != 0));
        cnt += all ? 1 : 0;
    }
    cnt += __shfl_xor(cnt, 1); cnt += __shfl_xor(cnt, 2);
    cnt += __shfl_xor(cnt, 4); cnt += __shfl_xor(cnt, 8);
    cnt += __shfl_xor(cnt, 16); cnt += __shfl_xor(cnt, 32);
    __shared__ int red[SUBSET_ACC_THREADS / 64];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) total += red[w];
        out[0] = (float)total * inv_b;
    }
}

// ===========================================================================
// normalize_table
// ===========================================================================
// y[n][f] = T((nan_to_num(x[n][f]) - xmin[f]) / (xmax[f] - xmin[f])): the
// table-sized counterpart of ingest_row_kernel, and bit for bit what
// BatchLoader computes (nan_to_num(nan=0): NaN -> 0, +-inf -> +-FLT_MAX;
// each of the two subtractions and the division rounded once in fp32, then
// one rounding to T). Flat grid-stride walk over N*F elements.
template <typename T>
__global__ void normalize_table_kernel(const float* __restrict__ x,
                                       const float* __restrict__ xmin,
                                       const float* __restrict__ xmax,
                                       T* __restrict__ y, long total, int F) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += stride) {
        const int f = (int)(i % F);
        float v = x[i];
        if (v != v) v = 0.0f;
        else if (v == __builtin_inff()) v = 3.402823466e+38f;
        else if (v == -__builtin_inff()) v = -3.402823466e+38f;
        const float mn = xmin[f];
        y[i] = from_f32<T>(__fdiv_rn(__fsub_rn(v, mn), __fsub_rn(xmax[f], mn)));
    }
}

// ===========================================================================
// window_batch
// ===========================================================================
// out (B, T, F) = the windows table[starts[b] : starts[b] + T] of a
// normalised (N, F) table, with the model's input dropout applied on the
// way: one write pass, the table stays cache resident. A window is one
// contiguous slab of the table, so out.flat[b*TF + r] = table.flat[
// starts[b]*F + r]. The masks are those of dropout_kernel (MODE 1: one draw
// per flat output octet) and spatial_dropout_kernel (MODE 2: channel id
// b*F + f) in gru_kernels.hip, through the same dropout_common.h helpers,
// so the result equals theirs on the materialised batch bit for bit.
//
// A thread owns 16 output bytes (V = 8 bf16 / 4 fp32 elements; for bf16
// that is the dropout octet). The output is 16-byte aligned; the source is
// not: a window starts at any row and rows are F*sizeof(T) bytes. LB is the
// width in bytes of the source loads, picked by the launcher from the real
// alignment of the base pointer and the row pitch. LB > 0 needs TF % V == 0:
// then no vector straddles two windows and there is no tail. LB == 0 is the
// element-wise path for everything else: a vector may straddle windows
// (two unrelated source addresses) and the last one may be partial.

template <int LB>
FMDA_DEV void load16(void* dst, const void* src) {
    if constexpr (LB == 16) {
        *(chunk16*)dst = *(const chunk16*)src;
    } else if constexpr (LB == 8) {
        ((uint2*)dst)[0] = ((const uint2*)src)[0];
        ((uint2*)dst)[1] = ((const uint2*)src)[1];
    } else {
        static_assert(LB == 4, "load16: LB is 16, 8 or 4");
#pragma unroll
        for (int k = 0; k < 4; ++k)
            ((unsigned int*)dst)[k] = ((const unsigned int*)src)[k];
    }
}

template <typename T, int LB, int MODE>
__global__ void window_batch_kernel(const T* __restrict__ table,
                                    const long* __restrict__ starts,
                                    T* __restrict__ out, long n, long TF,
                                    int F, unsigned int thr, float scale,
                                    unsigned long long seed) {
    constexpr int V = 16 / (int)sizeof(T);
    static_assert(MODE == 0 || V == 8, "dropout octets are 8 bf16 elements");
    const long o = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (o >= n) return;
    const long b = o / TF;
    const long r = o - b * TF;
    const int cnt = (o + V <= n) ? V : (int)(n - o);
    alignas(16) T v[V];
    if constexpr (LB > 0) {
        // r + V <= TF: the 16 bytes lie inside window b, hence in the table
        load16<LB>(v, table + starts[b] * F + r);
    } else {
        long bb = b, rr = r;
        const T* src = table + starts[bb] * F;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (k >= cnt) break;
            v[k] = src[rr];
            if (++rr == TF && k + 1 < cnt) {   // o + k + 1 < n: bb + 1 < B
                rr = 0;
                src = table + starts[++bb] * F;
            }
        }
    }
    if constexpr (MODE == 1) {
        const unsigned long long draw =
            mix64(seed ^ (unsigned long long)(o >> 3));
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (k >= cnt) break;
            v[k] = from_f32<T>(drop_apply(to_f32<T>(v[k]),
                                          drop_hit(draw, k, thr), scale));
        }
    } else if constexpr (MODE == 2) {
        long bb = b, rr = r;
        int f = (int)(r % F);
        unsigned long long q_last = ~0ull, draw = 0;   // c >> 3 is never ~0
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (k >= cnt) break;
            const long c = bb * F + f;                 // channel id (b, f)
            const unsigned long long q = (unsigned long long)(c >> 3);
            if (q != q_last) {
                draw = mix64(seed ^ q);
                q_last = q;
            }
            v[k] = from_f32<T>(drop_apply(
                to_f32<T>(v[k]), drop_hit(draw, (int)c & 7, thr), scale));
            if (++f == F) f = 0;
            if (++rr == TF) {
                rr = 0;
                ++bb;
            }
        }
    }
    if (cnt == V) {
        *(chunk16*)(out + o) = *(const chunk16*)v;
    } else {
        for (int k = 0; k < cnt; ++k) out[o + k] = v[k];
    }
}

template <typename T, int MODE>
void window_batch_dispatch(int lb, dim3 grid, hipStream_t stream,
                           const void* table, const long* starts, void* out,
                           long n, long TF, int F, unsigned int thr,
                           float scale, unsigned long long seed) {
#define FMDA_WB(LB)                                                        \
    window_batch_kernel<T, LB, MODE><<<grid, 256, 0, stream>>>(            \
        (const T*)table, starts, (T*)out, n, TF, F, thr, scale, seed)
    if (lb == 16) {
        FMDA_WB(16);
    } else if (lb == 8) {
        FMDA_WB(8);
    } else {
        // 4-byte loads are a vector path only for 2-byte elements
        if constexpr (sizeof(T) < 4) {
            if (lb == 4) {
                FMDA_WB(4);
                return;
            }
        }
        FMDA_WB(0);
    }
#undef FMDA_WB
}

inline int launch_ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

}  // namespace
}  // namespace fmda

using namespace fmda;

extern "C" int fmda_pack_gru_layer_launch(
        int is_bf16, const float* const* masters, void* w_ih_cat,
        void* b_ih_cat, void* w_hh_cat, float* b_hh_cat, void* wt, int D,
        int H, int Hp, int F, hipStream_t stream) {
    // masters: [w_ih, w_hh, b_ih, b_hh] per direction
    GruMasters m = {};
    for (int d = 0; d < D; ++d) {
        m.w_ih[d] = masters[4 * d + 0];
        m.w_hh[d] = masters[4 * d + 1];
        m.b_ih[d] = masters[4 * d + 2];
        m.b_hh[d] = masters[4 * d + 3];
    }
    const long total = (long)D * 3 * Hp * ((long)F + 2L * Hp + 2);
    const long blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048));
    if (is_bf16)
        pack_gru_layer_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
            m, (__hip_bfloat16*)w_ih_cat, (__hip_bfloat16*)b_ih_cat,
            (__hip_bfloat16*)w_hh_cat, b_hh_cat, (__hip_bfloat16*)wt, D, H,
            Hp, F);
    else
        pack_gru_layer_kernel<float><<<grid, 256, 0, stream>>>(
            m, (float*)w_ih_cat, (float*)b_ih_cat, (float*)w_hh_cat,
            b_hh_cat, (float*)wt, D, H, Hp, F);
    return launch_ok();
}

extern "C" int fmda_finalize_gru_wgrads_launch(
        int part_bf16, const void* part_ih, int c_ih, const void* part_hh,
        int c_hh, float* const* grads, int D, int H, int Hp, int F,
        hipStream_t stream) {
    // grads: [dw_ih, dw_hh] per direction
    GruWgrads o = {};
    for (int d = 0; d < D; ++d) {
        o.dw_ih[d] = grads[2 * d + 0];
        o.dw_hh[d] = grads[2 * d + 1];
    }
    const long total = (long)D * 3 * H * ((long)F + H);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (part_bf16)
        finalize_gru_wgrads_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
            (const __hip_bfloat16*)part_ih, c_ih,
            (const __hip_bfloat16*)part_hh, c_hh, o, D, H, Hp, F);
    else
        finalize_gru_wgrads_kernel<float><<<grid, 256, 0, stream>>>(
            (const float*)part_ih, c_ih, (const float*)part_hh, c_hh, o, D,
            H, Hp, F);
    return launch_ok();
}

// finalize_gru_wgrads in the order of the eager chunk sum. Both partials
// have EAGER_SUM_CHUNKS chunks (the caller checks that, and the output
// counts the order depends on).
extern "C" int fmda_finalize_gru_wgrads_eager_launch(
        int part_bf16, const void* part_ih, const void* part_hh,
        float* const* grads, int D, int H, int Hp, int F,
        hipStream_t stream) {
    GruWgrads o = {};
    for (int d = 0; d < D; ++d) {
        o.dw_ih[d] = grads[2 * d + 0];
        o.dw_hh[d] = grads[2 * d + 1];
    }
    const long total = (long)D * 3 * H * ((long)F + H);
    // vectors of 4 when no vector can leave its row
    const bool vec = H % 4 == 0 && F % 4 == 0;
    const long threads = vec ? total / 4 : total;
    const dim3 grid((unsigned)((threads + 255) / 256));
#define FMDA_FIN(PT, V)                                                    \
    finalize_gru_wgrads_eager_kernel<PT, V><<<grid, 256, 0, stream>>>(     \
        (const PT*)part_ih, (const PT*)part_hh, o, D, H, Hp, F)
    if (part_bf16) {
        if (vec) FMDA_FIN(__hip_bfloat16, 4);
        else FMDA_FIN(__hip_bfloat16, 1);
    } else {
        if (vec) FMDA_FIN(float, 4);
        else FMDA_FIN(float, 1);
    }
#undef FMDA_FIN
    return launch_ok();
}

extern "C" int fmda_eager_sum_chunks() { return EAGER_SUM_CHUNKS; }

// parts: (EAGER_SUM_CHUNKS, C, K) in the compute dtype
extern "C" int fmda_head_wgrads_eager_launch(
        int is_bf16, const void* parts, const float* db_sum, float* dW,
        float* db, int K, int C, hipStream_t stream) {
    const int n_w = C * K;
    const dim3 grid((n_w + C + 255) / 256);
    if (is_bf16)
        head_wgrads_eager_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
            (const __hip_bfloat16*)parts, db_sum, dW, db, n_w, C);
    else
        head_wgrads_eager_kernel<float><<<grid, 256, 0, stream>>>(
            (const float*)parts, db_sum, dW, db, n_w, C);
    return launch_ok();
}

// target_is_float: fp32 target, else bool storage; pred: bool storage
extern "C" int fmda_subset_accuracy_launch(
        int target_is_float, const void* target, const void* pred,
        float* out, int B, int C, hipStream_t stream) {
    const float inv_b = 1.0f / (float)B;
    if (target_is_float)
        subset_accuracy_kernel<float><<<1, SUBSET_ACC_THREADS, 0, stream>>>(
            (const float*)target, (const unsigned char*)pred, out, B, C,
            inv_b);
    else
        subset_accuracy_kernel<unsigned char>
            <<<1, SUBSET_ACC_THREADS, 0, stream>>>(
                (const unsigned char*)target, (const unsigned char*)pred,
                out, B, C, inv_b);
    return launch_ok();
}

// Column tile KT of head_fwd_master_staged_kernel for these shapes: the
// largest multiple of 8 (at most K) whose x and W tiles fit in 64 KB of LDS
// next to each other, or 0 when the staged kernel does not apply (rows that
// are not whole 16-byte vectors, an unaligned x, or no room for a tile).
static int head_fwd_stage_tile(const void* x, int es, int B, int K, int C,
                               int* rows_cap) {
    const int V = 16 / es;
    if (B < 1 || C < 1 || K % V != 0 || (uintptr_t)x % 16 != 0) return 0;
    // a block's 256 consecutive (row, class) pairs touch at most this many
    // rows
    const int rc = 255 / C + 2 < B ? 255 / C + 2 : B;
    // 1 KB short of 64 KB: the kernel's static LDS comes on top
    const long budget = 64512 - 16L * rc - 16L * C;
    long kt = budget / ((long)rc * es + 4L * C);
    if (kt > K) kt = K;
    if (kt < K) kt -= kt % 8;          // K itself is a multiple of V
    *rows_cap = rc;
    return kt >= 8 || kt == K ? (int)kt : 0;
}

// staged != 0: head_fwd_master_staged_kernel where it applies (same bits,
// operands read through LDS); 0: always the direct kernel.
extern "C" int fmda_head_fwd_master_launch(
        int is_bf16, const void* x, const float* W, const float* bias,
        const float* y, const float* wgt, const float* pw, float* logits,
        float* sig, float* loss_sum, int B, int K, int C, int staged,
        hipStream_t stream) {
    // same launch shape as fmda_head_fwd_launch: the per-block loss
    // partials (and their sum) must not change
    const dim3 grid((B * C + 255) / 256);
    int rows_cap = 0;
    const int es = is_bf16 ? 2 : 4;
    const int kt = staged ? head_fwd_stage_tile(x, es, B, K, C, &rows_cap) : 0;
    if (kt > 0) {
        const size_t lds = (size_t)rows_cap * (kt * es + 16) +
                           (size_t)C * (kt + 4) * 4;
        if (is_bf16)
            head_fwd_master_staged_kernel<__hip_bfloat16>
                <<<grid, 256, lds, stream>>>(
                    (const __hip_bfloat16*)x, W, bias, y, wgt, pw, logits,
                    sig, loss_sum, B, K, C, kt, rows_cap);
        else
            head_fwd_master_staged_kernel<float><<<grid, 256, lds, stream>>>(
                (const float*)x, W, bias, y, wgt, pw, logits, sig, loss_sum,
                B, K, C, kt, rows_cap);
        return launch_ok();
    }
    if (is_bf16)
        head_fwd_master_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
            (const __hip_bfloat16*)x, W, bias, y, wgt, pw, logits, sig,
            loss_sum, B, K, C);
    else
        head_fwd_master_kernel<float><<<grid, 256, 0, stream>>>(
            (const float*)x, W, bias, y, wgt, pw, logits, sig, loss_sum, B,
            K, C);
    return launch_ok();
}

extern "C" int fmda_head_bwd_master_launch(
        int is_bf16, const float* sig, const float* y, const float* wgt,
        const float* pw, const float* gscale, const float* W,
        float* dlogits, void* dlogits_t, void* dx, int B, int K, int C,
        hipStream_t stream) {
    // dlogits_t: optional (B, C) copy of dlogits in the compute dtype
    const dim3 grid((B * K + 255) / 256);
    if (is_bf16)
        head_bwd_master_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
            sig, y, wgt, pw, gscale, W, dlogits, (__hip_bfloat16*)dlogits_t,
            (__hip_bfloat16*)dx, B, K, C);
    else
        head_bwd_master_kernel<float><<<grid, 256, 0, stream>>>(
            sig, y, wgt, pw, gscale, W, dlogits, (float*)dlogits_t,
            (float*)dx, B, K, C);
    return launch_ok();
}

extern "C" int fmda_normalize_table_launch(
        int out_bf16, const float* x, const float* xmin, const float* xmax,
        void* y, long N, int F, hipStream_t stream) {
    const long total = N * (long)F;
    if (total == 0) return 0;
    const long blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
    if (out_bf16)
        normalize_table_kernel<__hip_bfloat16><<<grid, 256, 0, stream>>>(
            x, xmin, xmax, (__hip_bfloat16*)y, total, F);
    else
        normalize_table_kernel<float><<<grid, 256, 0, stream>>>(
            x, xmin, xmax, (float*)y, total, F);
    return launch_ok();
}

// Width in bytes of the source loads window_batch may use: the largest
// power of two <= 16 that divides both the table's base address (storage
// offset included) and its row pitch F*es, since a window starts at any
// row. 0 = element-wise: the alignment allows nothing wider than one
// element, or T*F is no multiple of the 16-byte vector.
extern "C" int fmda_window_batch_load_bytes(const void* table, long TF,
                                            long F, int es) {
    if (TF % (16 / es) != 0) return 0;
    const uintptr_t addr = (uintptr_t)table;
    const uintptr_t pitch = (uintptr_t)(F * es);
    int a = 16;
    while (a > es && (addr % a != 0 || pitch % a != 0)) a >>= 1;
    return a > es ? a : 0;
}

// mode: 0 gather only, 1 dropout_kernel's mask, 2 spatial_dropout_kernel's
// (bf16 only, like those kernels). (thr, scale) from drop_params().
extern "C" int fmda_window_batch_launch(
        int is_bf16, const void* table, const long* starts, void* out,
        long B, long Tlen, long F, int mode, unsigned int thr, float scale,
        unsigned long long seed, hipStream_t stream) {
    if (mode < 0 || mode > 2 || (mode != 0 && !is_bf16)) return -2;
    const int es = is_bf16 ? 2 : 4;
    const long TF = Tlen * F;
    const long n = B * TF;
    if (n == 0) return 0;
    const int lb = fmda_window_batch_load_bytes(table, TF, F, es);
    const long threads = (n + 16 / es - 1) / (16 / es);
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (!is_bf16)
        window_batch_dispatch<float, 0>(lb, grid, stream, table, starts, out,
                                        n, TF, (int)F, thr, scale, seed);
    else if (mode == 0)
        window_batch_dispatch<__hip_bfloat16, 0>(
            lb, grid, stream, table, starts, out, n, TF, (int)F, thr, scale,
            seed);
    else if (mode == 1)
        window_batch_dispatch<__hip_bfloat16, 1>(
            lb, grid, stream, table, starts, out, n, TF, (int)F, thr, scale,
            seed);
    else
        window_batch_dispatch<__hip_bfloat16, 2>(
            lb, grid, stream, table, starts, out, n, TF, (int)F, thr, scale,
            seed);
    return launch_ok();
}

extern "C" int fmda_head_wgrads_slabs(int B) {
    return (B + HEAD_SLAB - 1) / HEAD_SLAB;
}

extern "C" int fmda_head_wgrads_launch(
        int is_bf16, const float* dlogits, const void* x, float* dw_part,
        float* db_part, float* dW, float* db, int B, int K, int C,
        hipStream_t stream) {
    const int n_slabs = fmda_head_wgrads_slabs(B);
    const dim3 grid1((K + 127) / 128, n_slabs, C);
    if (is_bf16)
        head_wgrads_stage1_kernel<__hip_bfloat16><<<grid1, 128, 0, stream>>>(
            dlogits, (const __hip_bfloat16*)x, dw_part, db_part, B, K, C);
    else
        head_wgrads_stage1_kernel<float><<<grid1, 128, 0, stream>>>(
            dlogits, (const float*)x, dw_part, db_part, B, K, C);
    if (launch_ok() != 0) return -1;
    const dim3 grid2((C * K + C + 255) / 256);
    head_wgrads_stage2_kernel<<<grid2, 256, 0, stream>>>(
        dw_part, db_part, dW, db, n_slabs, K, C);
    return launch_ok();
}
