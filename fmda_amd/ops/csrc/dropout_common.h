// Counter-based dropout draw shared by every kernel that applies or
// recomputes a dropout mask (dropout_kernel, spatial_dropout_kernel and the
// fused recurrence epilogues in gru_kernels.hip; window_batch_kernel in
// glue_kernels.hip). One definition, so the masks agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace fmda {

// splitmix64 finaliser: the draw of octet `i` under `seed` is mix64(seed ^ i)
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// Byte k (0..7) of a draw against the 8-bit threshold of drop_params():
// true = the element is dropped.
__device__ __forceinline__ bool drop_hit(unsigned long long r, int k,
                                         unsigned int thr) {
    return ((unsigned int)(r >> (8 * k)) & 0xFF) < thr;
}

// Dropped -> 0, kept -> v * scale (fp32; the caller rounds once to its type).
__device__ __forceinline__ float drop_apply(float v, bool hit, float scale) {
    return hit ? 0.0f : v * scale;
}

}  // namespace fmda
