// Torch bindings for the fmda_amd HIP kernels (MI355X / gfx950).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "fmda_launch.h"

namespace {

// gi is the dense (B, T, n_dir*3Hp) tensor, or with `table` the
// (R, n_dir*3Hp) table of per-row projections that gru_fwd_windows slides
// over; B and T are then the caller's and stay untouched.
void check_common(const torch::Tensor& gi, const torch::Tensor& w,
                  const torch::Tensor& bhh, int& B, int& T, int& n_dir,
                  int& Hp, bool& is_bf16, bool table = false) {
    TORCH_CHECK(gi.is_cuda() && w.is_cuda() && bhh.is_cuda(),
                "fmda gru: tensors must be on GPU");
    TORCH_CHECK(gi.is_contiguous() && w.is_contiguous() && bhh.is_contiguous(),
                "fmda gru: tensors must be contiguous");
    TORCH_CHECK(gi.dim() == (table ? 2 : 3) && w.dim() == 3,
                "fmda gru: bad ranks");
    TORCH_CHECK(w.scalar_type() == gi.scalar_type(), "fmda gru: dtype mismatch");
    TORCH_CHECK(bhh.scalar_type() == torch::kFloat32, "bhh must be fp32");
    n_dir = w.size(0);
    Hp = w.size(2);
    TORCH_CHECK(w.size(1) == 3 * Hp, "w must be (n_dir, 3H, H)");
    if (!table) {
        B = gi.size(0);
        T = gi.size(1);
    }
    TORCH_CHECK(gi.size(-1) == (int64_t)n_dir * 3 * Hp, "gi last dim mismatch");
    TORCH_CHECK(n_dir == 1 || n_dir == 2, "n_dir must be 1 or 2");
    is_bf16 = gi.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(is_bf16 || gi.scalar_type() == torch::kFloat32,
                "fmda gru: dtype must be bf16 or fp32");
    // the bf16 recurrence tiles MFMA K=32: Hp=16 would silently drop the
    // recurrent term (KK = Hp/32 = 0) — pad to Hp >= 32 instead
    TORCH_CHECK(!(is_bf16 && Hp < 32),
                "fmda gru: bf16 requires Hp >= 32 (MFMA K=32); pad the "
                "hidden size");
}

// The one place where a dropout probability becomes kernel arguments. Every
// dropout path (dropout_fused, spatial_dropout_fused and the fused
// epilogues of gru_fwd / gru_bwd) goes through it, so they agree bitwise.
//   thr:   8-bit draw threshold, (unsigned)(float(p) * 256.0f)
//   scale: keep scale 1/(1-p) evaluated in DOUBLE and rounded once to fp32
//          (torch.nn.functional.dropout's value: p=0.6 -> 2.5 exactly; the
//          float expression 1.0f/(1.0f-p) gives 2.5000002 there)
struct DropParams {
    unsigned int thr;
    float scale;
};

DropParams drop_params(double p) {
    if (!(p > 0.0)) return {0u, 1.0f};
    return {(unsigned int)((float)p * 256.0f), (float)(1.0 / (1.0 - p))};
}

// Forward dispatch shared by gru_fwd (dense gi, gi_pitch = T*n_dir*3Hp) and
// gru_fwd_windows (table of projections, gi_pitch = stride*n_dir*3Hp).
// gi_pitch is in elements; the kernels read 16-byte chunks through it.
std::vector<torch::Tensor> gru_fwd_dispatch(
        const torch::Tensor& gi, const torch::Tensor& w,
        const torch::Tensor& bhh, int B, int T, int n_dir, int Hp,
        bool is_bf16, int64_t gi_pitch,
        const c10::optional<torch::Tensor>& h0_opt, double drop_p,
        int64_t drop_seed) {
    // a multiple of 16 bytes for every Hp the kernels take (Hp >= 16)
    TORCH_CHECK((gi_pitch * gi.element_size()) % 16 == 0,
                "fmda gru: gi batch pitch must be a multiple of 16 bytes");
    const float* h0 = nullptr;
    if (h0_opt.has_value()) {
        auto& h = h0_opt.value();
        TORCH_CHECK(h.is_cuda() && h.is_contiguous() &&
                    h.scalar_type() == torch::kFloat32 &&
                    h.sizes() == torch::IntArrayRef({n_dir, B, Hp}),
                    "h0 must be contiguous fp32 (n_dir, B, Hp)");
        h0 = h.data_ptr<float>();
    }
    auto out = torch::empty({B, T, (int64_t)n_dir * Hp}, gi.options());
    auto hlast = torch::empty({n_dir, B, Hp},
                              gi.options().dtype(torch::kFloat32));
    // fused forward dropout: emit out AND the dropped copy (the layer
    // above's input) from the store epilogue, replacing the separate
    // full-tensor dropout pass. Quantized exactly like dropout_kernel.
    const DropParams dp = drop_params(drop_p);
    const unsigned int drop_thr = dp.thr;
    const float drop_scale = dp.scale;
    torch::Tensor out_drop;
    void* out_drop_ptr = nullptr;
    if (drop_thr != 0u) {
        TORCH_CHECK(is_bf16 && (Hp == 128 || Hp == 512),
                    "fused fwd dropout requires bf16 Hp=128/512");
        TORCH_CHECK(Hp == 128 || h0 == nullptr,
                    "fused fwd dropout with h0 requires Hp=128");
        out_drop = torch::empty_like(out);
        out_drop_ptr = out_drop.data_ptr();
    }
    auto stream = at::hip::getCurrentHIPStream();
    int rc;
    // the column-split Hp=512 kernel pre-publishes h_{-1}=0; with a real
    // h0 the batch-parallel kernel takes the (rare) call instead
    if (is_bf16 && Hp == 512 && h0 == nullptr) {
        // column-split persistent kernel: publication ring + group counters
        const int BR = 256;
        const int GB = (B + BR - 1) / BR;
        const int G = GB * n_dir;
        auto hpub = torch::empty({2, G, BR, (int64_t)Hp}, gi.options());
        auto cnt = torch::zeros({G}, gi.options().dtype(torch::kUInt32));
        rc = fmda_gru_fwd_cs_launch(gi.data_ptr(), w.data_ptr(),
                                    bhh.data_ptr<float>(), out.data_ptr(),
                                    hlast.data_ptr<float>(), hpub.data_ptr(),
                                    (unsigned int*)cnt.data_ptr(), B, T,
                                    n_dir, out_drop_ptr, drop_thr,
                                    drop_scale,
                                    (unsigned long long)drop_seed,
                                    (long)gi_pitch, stream.stream());
    } else {
        rc = fmda_gru_fwd_launch(is_bf16 ? 1 : 0, Hp, gi.data_ptr(),
                                 w.data_ptr(), bhh.data_ptr<float>(),
                                 out.data_ptr(), hlast.data_ptr<float>(), B, T,
                                 n_dir, h0, out_drop_ptr, drop_thr,
                                 drop_scale,
                                 (unsigned long long)drop_seed,
                                 (long)gi_pitch, stream.stream());
    }
    TORCH_CHECK(rc == 0, "fmda gru_fwd launch failed rc=", rc, " Hp=", Hp);
    if (out_drop_ptr != nullptr)
        return {out, hlast, out_drop};
    return {out, hlast};
}

}  // namespace

std::vector<torch::Tensor> gru_fwd(torch::Tensor gi, torch::Tensor w,
                                   torch::Tensor bhh,
                                   c10::optional<torch::Tensor> h0_opt,
                                   double drop_p, int64_t drop_seed) {
    int B, T, n_dir, Hp;
    bool is_bf16;
    check_common(gi, w, bhh, B, T, n_dir, Hp, is_bf16);
    return gru_fwd_dispatch(gi, w, bhh, B, T, n_dir, Hp, is_bf16,
                            (int64_t)T * n_dir * 3 * Hp, h0_opt, drop_p,
                            drop_seed);
}

// Recurrence over sliding windows of a table of input projections: window b
// covers rows [b*stride, b*stride + T) of gi_rows (R, n_dir*3Hp), so
// overlapping windows read the same rows instead of a materialised
// (B, T, n_dir*3Hp) copy. B = (R - T) / stride + 1; trailing rows are
// ignored. Same kernels and dispatch as gru_fwd with h0 = None and no
// dropout; out (B, T, n_dir*Hp) and h_last (n_dir, B, Hp) as from gru_fwd.
std::vector<torch::Tensor> gru_fwd_windows(torch::Tensor gi_rows,
                                           torch::Tensor w, torch::Tensor bhh,
                                           int64_t T, int64_t stride) {
    int B = 0, T_ = 0, n_dir, Hp;
    bool is_bf16;
    check_common(gi_rows, w, bhh, B, T_, n_dir, Hp, is_bf16, true);
    const int64_t R = gi_rows.size(0), row = gi_rows.size(1);
    TORCH_CHECK(T >= 1 && stride >= 1,
                "gru_fwd_windows: T and stride must be >= 1");
    TORCH_CHECK(R >= T, "gru_fwd_windows: table has ", R,
                " rows, fewer than the window T=", T);
    const int64_t nB = (R - T) / stride + 1;
    TORCH_CHECK(nB <= INT_MAX && T <= INT_MAX,
                "gru_fwd_windows: too many windows");
    // a row-slice of a larger table starts on a row boundary
    TORCH_CHECK(reinterpret_cast<uintptr_t>(gi_rows.data_ptr()) % 16 == 0,
                "gru_fwd_windows: gi_rows must be 16-byte aligned");
    return gru_fwd_dispatch(gi_rows, w, bhh, (int)nB, (int)T, n_dir, Hp,
                            is_bf16, stride * row, c10::nullopt, 0.0, 0);
}

// dout (B, T, n_dir*Hp) and dhT (n_dir, B, Hp) fp32 are the layer's output
// gradients. A top layer whose out feeds pool_features_fwd alone passes
// dfeat (B, 3Hp) bf16 and amax (B, Hp) int32 instead (dout = dhT = None):
// the kernel then synthesises what pool_features_bwd would have written.
std::vector<torch::Tensor> gru_bwd(torch::Tensor gi, torch::Tensor w,
                                   torch::Tensor bhh, torch::Tensor out,
                                   c10::optional<torch::Tensor> dout_opt,
                                   c10::optional<torch::Tensor> dhT_opt,
                                   double drop_p, int64_t drop_seed,
                                   c10::optional<torch::Tensor> h0_opt,
                                   c10::optional<torch::Tensor> wt_opt,
                                   c10::optional<torch::Tensor> dfeat_opt,
                                   c10::optional<torch::Tensor> amax_opt) {
    int B, T, n_dir, Hp;
    bool is_bf16;
    check_common(gi, w, bhh, B, T, n_dir, Hp, is_bf16);
    const bool pooled = dfeat_opt.has_value() || amax_opt.has_value();
    torch::Tensor dout, dhT, dfeat, amax;
    long dfeat_ld = 0;
    if (pooled) {
        TORCH_CHECK(dfeat_opt.has_value() && amax_opt.has_value() &&
                    !dout_opt.has_value() && !dhT_opt.has_value(),
                    "fmda gru_bwd: pass either (dout, dhT) or (dfeat, amax)");
        dfeat = dfeat_opt.value();
        amax = amax_opt.value();
        TORCH_CHECK(is_bf16 && Hp == 128,
                    "fmda gru_bwd: the pooled path needs bf16 and "
                    "H == Hp == 128, got Hp=", Hp);
        TORCH_CHECK(T <= 256, "fmda gru_bwd: the pooled path keeps amax in "
                    "one byte, T=", T, " > 256");
        TORCH_CHECK(drop_p == 0.0,
                    "fmda gru_bwd: the pooled path has no dropout");
        TORCH_CHECK(dfeat.is_cuda() && dfeat.dim() == 2 &&
                    dfeat.scalar_type() == torch::kBFloat16 &&
                    dfeat.size(0) == B && dfeat.size(1) == 3 * Hp,
                    "fmda gru_bwd: dfeat must be bf16 (B, 3H) on the GPU");
        TORCH_CHECK(amax.is_cuda() && amax.is_contiguous() &&
                    amax.scalar_type() == torch::kInt32 && amax.dim() == 2 &&
                    amax.size(0) == B && amax.size(1) == Hp,
                    "fmda gru_bwd: amax must be contiguous int32 (B, H)");
        TORCH_CHECK(dfeat.stride(1) == 1,
                    "fmda gru_bwd: dfeat needs unit column stride");
        dfeat_ld = B == 1 ? 3L * Hp : (long)dfeat.stride(0);
        // 16-byte row loads: whole 8-element groups on an aligned base
        TORCH_CHECK(dfeat_ld >= 3 * Hp && dfeat_ld % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(dfeat.data_ptr()) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(amax.data_ptr()) % 16 == 0,
                    "fmda gru_bwd: dfeat needs a row pitch >= 3H that is a "
                    "multiple of 8 and 16-byte aligned data");
        TORCH_CHECK(out.is_cuda() && out.scalar_type() == gi.scalar_type() &&
                    out.dim() == 3 && out.size(0) == B && out.size(1) == T &&
                    out.size(2) == (int64_t)n_dir * Hp,
                    "fmda gru_bwd: out must be (B, T, n_dir*Hp)");
    } else {
        TORCH_CHECK(dout_opt.has_value() && dhT_opt.has_value(),
                    "fmda gru_bwd: dout and dhT are required");
        dout = dout_opt.value();
        dhT = dhT_opt.value();
    }
    const float* h0 = nullptr;
    torch::Tensor dgh0;
    void* dgh0_ptr = nullptr;
    if (h0_opt.has_value()) {
        auto& h = h0_opt.value();
        TORCH_CHECK(h.is_cuda() && h.is_contiguous() &&
                    h.scalar_type() == torch::kFloat32 &&
                    h.sizes() == torch::IntArrayRef({n_dir, B, Hp}),
                    "h0 must be contiguous fp32 (n_dir, B, Hp)");
        h0 = h.data_ptr<float>();
        dgh0 = torch::empty({n_dir, B, (int64_t)3 * Hp}, gi.options());
        dgh0_ptr = dgh0.data_ptr();
    }
    TORCH_CHECK(out.is_contiguous() &&
                (pooled || (dout.is_contiguous() && dhT.is_contiguous())),
                "fmda gru_bwd: tensors must be contiguous");
    TORCH_CHECK(pooled || dhT.scalar_type() == torch::kFloat32,
                "dhT must be fp32");
    // fp32 BPTT at Hp=512 needs ~264 KB of LDS staging — architecturally
    // out of budget (160 KB/CU); bf16 (the training dtype) covers H>256.
    TORCH_CHECK(is_bf16 || Hp <= 256,
                "fp32 backward unsupported for Hp > 256 (LDS budget); "
                "train in bf16 for hidden sizes above 256");
    torch::Tensor dgi, dgh;
    if (getenv("FMDA_ZERO_GRADS")) {   // debug: expose unwritten positions
        dgi = torch::zeros_like(gi);
        dgh = torch::zeros_like(gi);
    } else {
        dgi = torch::empty_like(gi);
        dgh = torch::empty_like(gi);
    }
    auto dh0 = torch::empty({n_dir, B, Hp},
                            gi.options().dtype(torch::kFloat32));
    // packed bias-grad sums: [dr, dz, dhn | dn] per direction; db_hh and
    // db_ih are assembled from slices below (dr/dz shared).
    // Each batch tile of the launch stores its sums into a row of its own
    // and the rows are summed below in a fixed order, which keeps the bias
    // grads bitwise reproducible. The launcher reports how many rows its
    // grid writes for this shape.
    const bool column_split = is_bf16 && Hp == 512 && h0 == nullptr;
    const int64_t db_rows = fmda_gru_bwd_db_rows(is_bf16 ? 1 : 0, Hp, B,
                                                 column_split ? 1 : 0);
    // The batch-parallel kernels (gru_bwd_kernel, gru_bwd_v3_kernel) run a
    // (batch tile, dir) grid, and every block's epilogue stores all 4 slots
    // of all Hp / 16 column tiles of its row (the tiles are dealt out
    // ct = wave + NW * i over all NW waves), so the table needs no fill.
    // The column-split kernel's rows keep their zero fill.
    auto dbopts = gi.options().dtype(torch::kFloat32);
    auto dbpart = column_split
        ? torch::zeros({db_rows, n_dir, 4 * Hp}, dbopts)
        : torch::empty({db_rows, n_dir, 4 * Hp}, dbopts);
    // W^T for the carry GEMM's B fragments (v3 kernel streams them from
    // L2 as contiguous bf16x8 rows instead of hoisting 48 VGPRs). A caller
    // that packed the weights with pack_gru_layer already has it.
    torch::Tensor wt;
    const void* wt_ptr = nullptr;
    if (is_bf16 && (Hp == 128 || Hp == 512)) {
        if (wt_opt.has_value()) {
            wt = wt_opt.value();
            TORCH_CHECK(wt.is_cuda() && wt.is_contiguous() &&
                        wt.scalar_type() == w.scalar_type() &&
                        wt.sizes() == torch::IntArrayRef(
                            {n_dir, Hp, (int64_t)3 * Hp}),
                        "wt must be contiguous (n_dir, Hp, 3Hp) in w's dtype");
        } else {
            wt = w.transpose(1, 2).contiguous();
        }
        wt_ptr = wt.data_ptr();
    }
    auto stream = at::hip::getCurrentHIPStream();
    int rc;
    // fused inter-layer dropout backward (d_out is w.r.t. the DROPPED
    // activations; the kernels recompute the counter-based mask at the
    // dout read instead of a separate full-tensor pass). drop_params()
    // quantizes EXACTLY like the forward paths, so the recomputed backward
    // mask can never disagree with the forward one at a rounding boundary.
    const DropParams dp = drop_params(drop_p);
    if (pooled) {
        TORCH_CHECK(wt_ptr != nullptr, "fmda gru_bwd: pooled path needs wt");
        rc = fmda_gru_bwd_pooled_launch(
            gi.data_ptr(), w.data_ptr(), wt_ptr, bhh.data_ptr<float>(),
            out.data_ptr(), dfeat.data_ptr(), amax.data_ptr<int>(), dfeat_ld,
            dgi.data_ptr(), dgh.data_ptr(), dh0.data_ptr<float>(),
            dbpart.data_ptr<float>(), B, T, n_dir, h0, dgh0_ptr,
            stream.stream());
    } else if (column_split) {
        const unsigned int cs_thr = dp.thr;
        const float cs_scale = dp.scale;
        const int BR = 256;
        const int GB = (B + BR - 1) / BR;
        const int G = GB * n_dir;
        auto gpub = torch::empty({2, G, BR, (int64_t)3 * Hp}, gi.options());
        auto cnt = torch::zeros({G}, gi.options().dtype(torch::kUInt32));
        rc = fmda_gru_bwd_cs_launch(
            gi.data_ptr(), w.data_ptr(), wt_ptr, bhh.data_ptr<float>(),
            out.data_ptr(), dout.data_ptr(), dhT.data_ptr<float>(),
            dgi.data_ptr(), dgh.data_ptr(), dh0.data_ptr<float>(),
            dbpart.data_ptr<float>(), gpub.data_ptr(),
            (unsigned int*)cnt.data_ptr(), B, T, n_dir, cs_thr, cs_scale,
            (unsigned long long)drop_seed, stream.stream());
    } else {
        const unsigned int drop_thr = dp.thr;
        const float drop_scale = dp.scale;
        TORCH_CHECK(drop_thr == 0u || (is_bf16 && Hp == 128),
                    "fused dropout-backward on this path requires bf16 "
                    "Hp=128");
        rc = fmda_gru_bwd_launch(is_bf16 ? 1 : 0, Hp, gi.data_ptr(),
                                 w.data_ptr(), wt_ptr, bhh.data_ptr<float>(),
                                 out.data_ptr(), dout.data_ptr(),
                                 dhT.data_ptr<float>(), dgi.data_ptr(),
                                 dgh.data_ptr(), dh0.data_ptr<float>(),
                                 dbpart.data_ptr<float>(), B, T,
                                 n_dir, drop_thr, drop_scale,
                                 (unsigned long long)drop_seed, h0, dgh0_ptr,
                                 stream.stream());
    }
    TORCH_CHECK(rc == 0, "fmda gru_bwd launch failed rc=", rc, " Hp=", Hp);
    // fixed-order row sum + slot scatter: db_hh = [dr, dz, dhn],
    // db_ih = [dr, dz, dn] (dr/dz shared); every element is written
    auto dbhh = torch::empty({n_dir, 3 * Hp},
                             gi.options().dtype(torch::kFloat32));
    auto dbih = torch::empty_like(dbhh);
    rc = fmda_gru_db_reduce_launch(dbpart.data_ptr<float>(), (int)db_rows,
                                   n_dir, Hp, dbhh.data_ptr<float>(),
                                   dbih.data_ptr<float>(), stream.stream());
    TORCH_CHECK(rc == 0, "fmda gru db reduce launch failed");
    if (dgh0_ptr != nullptr)
        return {dgi, dgh, dh0, dbhh, dbih, dgh0};
    return {dgi, dgh, dh0, dbhh, dbih};
}

torch::Tensor mfma_selftest(torch::Tensor A, torch::Tensor Bm) {
    TORCH_CHECK(A.is_cuda() && A.scalar_type() == torch::kBFloat16);
    TORCH_CHECK(A.sizes() == torch::IntArrayRef({16, 32}) &&
                Bm.sizes() == torch::IntArrayRef({32, 16}));
    auto C = torch::empty({16, 16}, A.options().dtype(torch::kFloat32));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_mfma_selftest_launch(A.contiguous().data_ptr(),
                                       Bm.contiguous().data_ptr(),
                                       C.data_ptr<float>(), stream.stream());
    TORCH_CHECK(rc == 0, "mfma selftest launch failed");
    return C;
}

// act_dtype: return max / avg in out's dtype instead of fp32 (the kernel
// rounds where the caller's .to(out.dtype) would have).
// serial: always a thread-per-column kernel (T summed in ascending order),
// also for the small grids that by default get the wave-per-pair kernel.
std::vector<torch::Tensor> pool_fwd(torch::Tensor out, int64_t n_dir,
                                    bool act_dtype, bool serial) {
    TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 3);
    const bool bf16 = out.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(bf16 || out.scalar_type() == torch::kFloat32);
    const int B = out.size(0), T = out.size(1);
    const int H = out.size(2) / n_dir;
    TORCH_CHECK(H % 2 == 0, "pool_fwd pairs columns: H must be even "
                "(odd H uses the eager path)");
    const bool act_io = act_dtype && bf16;   // fp32 activations: same thing
    auto pooled = out.options().dtype(act_io ? torch::kBFloat16
                                             : torch::kFloat32);
    auto maxv = torch::empty({B, H}, pooled);
    auto avgv = torch::empty({B, H}, pooled);
    auto amax = torch::empty({B, H}, out.options().dtype(torch::kInt32));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_pool_fwd_launch(bf16 ? 1 : 0, out.data_ptr(),
                                  maxv.data_ptr(), avgv.data_ptr(),
                                  amax.data_ptr<int>(), B, T, H, (int)n_dir,
                                  act_io ? 1 : 0, serial ? 1 : 0,
                                  stream.stream());
    TORCH_CHECK(rc == 0, "pool_fwd launch failed");
    return {maxv, avgv, amax};
}

// Pooled-head features in one kernel: out (B, T, D*H) bf16 and the raw
// h_last (D, B, H) fp32 of the top layer -> feat (B, 3H) bf16 =
// [dirsum(h_last) | max_T | avg_T] and amax (B, H) int32. The same bits as
// pool_fwd(act_dtype, serial) plus the eager h_n cast / direction sum / cat.
std::vector<torch::Tensor> pool_features_fwd(torch::Tensor out,
                                             torch::Tensor hlast) {
    TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 3 &&
                out.scalar_type() == torch::kBFloat16,
                "pool_features_fwd: out must be contiguous bf16 (B, T, D*H) "
                "on the GPU");
    TORCH_CHECK(hlast.is_cuda() && hlast.is_contiguous() &&
                hlast.dim() == 3 && hlast.scalar_type() == torch::kFloat32,
                "pool_features_fwd: h_last must be contiguous fp32 (D, B, H)");
    const int64_t B = out.size(0), T = out.size(1);
    const int64_t D = hlast.size(0), H = hlast.size(2);
    TORCH_CHECK((D == 1 || D == 2) && hlast.size(1) == B &&
                out.size(2) == D * H, "pool_features_fwd: shape mismatch");
    TORCH_CHECK(H % 8 == 0 && H >= 8 && T >= 1 && B >= 1,
                "pool_features_fwd: needs H % 8 == 0 and a non-empty input");
    TORCH_CHECK(T <= INT_MAX && B * (H / 8) <= INT_MAX - 256,
                "pool_features_fwd: too large");
    auto feat = torch::empty({B, 3 * H}, out.options());
    auto amax = torch::empty({B, H}, out.options().dtype(torch::kInt32));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_pool_features_fwd_launch(
        out.data_ptr(), hlast.data_ptr<float>(), feat.data_ptr(),
        amax.data_ptr<int>(), (int)B, (int)T, (int)H, (int)D,
        stream.stream());
    TORCH_CHECK(rc == 0, "pool_features_fwd launch failed rc=", rc);
    return {feat, amax};
}

// Backward of pool_features_fwd in one kernel: dfeat (B, 3H) bf16, rows
// possibly pitched -> d_out (B, T, D*H) bf16 as pool_bwd writes it, and
// d_hlast (D, B, H) fp32 = float(dfeat[:, :H]) for every direction.
std::vector<torch::Tensor> pool_features_bwd(torch::Tensor dfeat,
                                             torch::Tensor amax, int64_t T,
                                             int64_t n_dir) {
    TORCH_CHECK(dfeat.is_cuda() && dfeat.dim() == 2 &&
                dfeat.scalar_type() == torch::kBFloat16 &&
                amax.is_cuda() && amax.is_contiguous() && amax.dim() == 2 &&
                amax.scalar_type() == torch::kInt32,
                "pool_features_bwd: dfeat must be bf16 (B, 3H), amax "
                "contiguous int32 (B, H), both on the GPU");
    const int64_t B = amax.size(0), H = amax.size(1);
    TORCH_CHECK(dfeat.size(0) == B && dfeat.size(1) == 3 * H,
                "pool_features_bwd: shape mismatch");
    TORCH_CHECK(dfeat.stride(1) == 1 &&
                (B == 1 || dfeat.stride(0) >= 3 * H),
                "pool_features_bwd: dfeat needs unit column stride");
    TORCH_CHECK((n_dir == 1 || n_dir == 2) && H % 8 == 0 && H >= 8 &&
                T >= 1 && B >= 1 && T <= INT_MAX &&
                B * (H / 8) <= INT_MAX - 256,
                "pool_features_bwd: unsupported shape");
    auto dout = torch::empty({B, T, n_dir * H}, dfeat.options());
    auto dhlast = torch::empty({n_dir, B, H},
                               dfeat.options().dtype(torch::kFloat32));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_pool_features_bwd_launch(
        dfeat.data_ptr(), amax.data_ptr<int>(), dout.data_ptr(),
        dhlast.data_ptr<float>(), (int)B, (int)T, (int)H, (int)n_dir,
        B == 1 ? 3 * H : (long)dfeat.stride(0), stream.stream());
    TORCH_CHECK(rc == 0, "pool_features_bwd launch failed rc=", rc);
    return {dout, dhlast};
}

torch::Tensor pool_bwd(torch::Tensor dmax, torch::Tensor davg,
                       torch::Tensor amax, int64_t T, int64_t n_dir,
                       torch::ScalarType dtype) {
    // rows may be pitched (column slices of the pooled-feature gradient)
    TORCH_CHECK(dmax.is_cuda() && davg.is_cuda() && dmax.dim() == 2 &&
                davg.sizes() == dmax.sizes() && amax.sizes() == dmax.sizes() &&
                amax.is_contiguous(), "pool_bwd: shape mismatch");
    const int B = dmax.size(0), H = dmax.size(1);
    TORCH_CHECK((H == 1 || (dmax.stride(1) == 1 && davg.stride(1) == 1)) &&
                (B == 1 || (dmax.stride(0) >= H && davg.stride(0) >= H)),
                "pool_bwd: dmax / davg need unit column stride");
    const bool bf16 = dtype == torch::kBFloat16;
    // dmax / davg come in fp32, or for bf16 activations in bf16 as well
    const bool act_io = bf16 && dmax.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(dmax.scalar_type() == davg.scalar_type() &&
                (act_io || dmax.scalar_type() == torch::kFloat32),
                "pool_bwd: dmax / davg must both be fp32, or both bf16 with "
                "bf16 activations");
    auto dout = torch::empty({B, T, n_dir * H}, dmax.options().dtype(dtype));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_pool_bwd_launch(bf16 ? 1 : 0, dmax.data_ptr(),
                                  davg.data_ptr(), amax.data_ptr<int>(),
                                  dout.data_ptr(), B, (int)T, H, (int)n_dir,
                                  act_io ? 1 : 0,
                                  B == 1 ? H : (long)dmax.stride(0),
                                  B == 1 ? H : (long)davg.stride(0),
                                  stream.stream());
    TORCH_CHECK(rc == 0, "pool_bwd launch failed");
    return dout;
}

// chunks: int64 tensor (n_chunks, 5) holding {p, g, m, v, n} built by
// fmda_amd.optim.FusedClipAdam (device buffer; pointers as int64).
torch::Tensor fused_clip_adam(torch::Tensor chunks, int64_t n_chunks,
                              double clip, double lr, double beta1,
                              double beta2, double eps, int64_t step) {
    TORCH_CHECK(chunks.is_cuda() && chunks.scalar_type() == torch::kInt64);
    auto f32 = chunks.options().dtype(torch::kFloat32);
    torch::Tensor norm2;
    auto stream = at::hip::getCurrentHIPStream();
    if (clip > 0) {
        // one partial per block of the launch grid (min(n_chunks, 2048)
        // blocks, every block stores its entry), summed in a fixed order
        auto part = torch::empty({std::min<int64_t>(n_chunks, 2048)}, f32);
        int rc = fmda_opt_norm2_launch(chunks.data_ptr(), (int)n_chunks,
                                       part.data_ptr<float>(),
                                       stream.stream());
        TORCH_CHECK(rc == 0, "opt norm2 launch failed");
        norm2 = part.sum().reshape({1});
    } else {
        norm2 = torch::zeros({1}, f32);
    }
    const float bc1 = 1.0f - powf((float)beta1, (float)step);
    const float bc2 = 1.0f - powf((float)beta2, (float)step);
    int rc = fmda_opt_adam_launch(chunks.data_ptr(), (int)n_chunks,
                                  norm2.data_ptr<float>(), (float)clip,
                                  (float)lr, (float)beta1, (float)beta2,
                                  (float)eps, bc1, bc2, stream.stream());
    TORCH_CHECK(rc == 0, "opt adam launch failed");
    return norm2;
}

std::vector<torch::Tensor> head_loss_fwd(torch::Tensor x, torch::Tensor W,
                                         torch::Tensor b, torch::Tensor y,
                                         torch::Tensor wgt, torch::Tensor pw) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && W.is_contiguous());
    const bool bf16 = x.scalar_type() == torch::kBFloat16;
    const int B = x.size(0), K = x.size(1), C = W.size(0);
    auto f32 = x.options().dtype(torch::kFloat32);
    auto logits = torch::empty({B, C}, f32);
    auto sig = torch::empty({B, C}, f32);
    // one partial per block of the launch grid ((B*C + 255) / 256 blocks,
    // every block stores its entry), summed here in a fixed order
    auto part = torch::empty({((int64_t)B * C + 255) / 256}, f32);
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_head_fwd_launch(
        bf16 ? 1 : 0, x.data_ptr(), W.data_ptr(), b.data_ptr(),
        y.data_ptr<float>(), wgt.data_ptr<float>(), pw.data_ptr<float>(),
        logits.data_ptr<float>(), sig.data_ptr<float>(),
        part.data_ptr<float>(), B, K, C, stream.stream());
    TORCH_CHECK(rc == 0, "head fwd launch failed");
    return {logits, sig, part.sum().reshape({1})};
}

std::vector<torch::Tensor> head_loss_bwd(torch::Tensor sig, torch::Tensor y,
                                         torch::Tensor wgt, torch::Tensor pw,
                                         torch::Tensor gscale,
                                         torch::Tensor W,
                                         torch::ScalarType xdtype) {
    const int B = sig.size(0), C = sig.size(1), K = W.size(1);
    const bool bf16 = xdtype == torch::kBFloat16;
    auto dlogits = torch::empty_like(sig);
    auto dx = torch::empty({B, K}, sig.options().dtype(xdtype));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_head_bwd_launch(
        bf16 ? 1 : 0, sig.data_ptr<float>(), y.data_ptr<float>(),
        wgt.data_ptr<float>(), pw.data_ptr<float>(),
        gscale.data_ptr<float>(), W.data_ptr(), dlogits.data_ptr<float>(),
        dx.data_ptr(), B, K, C, stream.stream());
    TORCH_CHECK(rc == 0, "head bwd launch failed");
    return {dlogits, dx};
}

torch::Tensor dropout_fused(torch::Tensor x, double p, int64_t seed) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                x.scalar_type() == torch::kBFloat16);
    auto y = torch::empty_like(x);
    auto stream = at::hip::getCurrentHIPStream();
    const DropParams dp = drop_params(p);
    int rc = fmda_dropout_launch(1, x.data_ptr(), y.data_ptr(), x.numel(),
                                 dp.thr, dp.scale, (unsigned long long)seed,
                                 stream.stream());
    TORCH_CHECK(rc == 0, "dropout launch failed");
    return y;
}

torch::Tensor spatial_dropout_fused(torch::Tensor x, double p,
                                    int64_t seed) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 3 &&
                x.scalar_type() == torch::kBFloat16);
    auto y = torch::empty_like(x);
    auto stream = at::hip::getCurrentHIPStream();
    const DropParams dp = drop_params(p);
    int rc = fmda_spatial_dropout_launch(
        1, x.data_ptr(), y.data_ptr(), x.size(0), x.size(1), x.size(2),
        dp.thr, dp.scale, (unsigned long long)seed, stream.stream());
    TORCH_CHECK(rc == 0, "spatial dropout launch failed");
    return y;
}

// (N, F) fp32 raw table -> (nan_to_num(x, 0) - x_min) / (x_max - x_min) in
// `dtype` (fp32 or bf16), one pass; bitwise what BatchLoader computes.
torch::Tensor normalize_table(torch::Tensor x, torch::Tensor x_min,
                              torch::Tensor x_max, torch::ScalarType dtype) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2 &&
                x.scalar_type() == torch::kFloat32,
                "normalize_table: x must be a contiguous (N, F) fp32 GPU "
                "tensor");
    const int64_t N = x.size(0), F = x.size(1);
    for (const torch::Tensor* t : {&x_min, &x_max})
        TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->scalar_type() == torch::kFloat32 && t->numel() == F,
                    "normalize_table: x_min / x_max must be fp32 (F) on GPU");
    TORCH_CHECK(dtype == torch::kBFloat16 || dtype == torch::kFloat32,
                "normalize_table: dtype must be bf16 or fp32");
    TORCH_CHECK(F >= 1 && F <= INT_MAX, "normalize_table: bad F");
    auto y = torch::empty({N, F}, x.options().dtype(dtype));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_normalize_table_launch(
        dtype == torch::kBFloat16 ? 1 : 0, x.data_ptr<float>(),
        x_min.data_ptr<float>(), x_max.data_ptr<float>(), y.data_ptr(),
        (long)N, (int)F, stream.stream());
    TORCH_CHECK(rc == 0, "normalize_table launch failed");
    return y;
}

// (B, window, F) batch of the windows table[starts[b] : starts[b] + window]
// of a normalised (N, F) table, in the table's dtype, with input dropout
// fused into the one write pass: for bf16 and p > 0 the result is bitwise
// dropout_fused / spatial_dropout_fused (same seed) of the materialised
// gather. fp32 only gathers (p must be 0). The table's rows must be dense
// (a row-slice view is fine). The values of `starts` are the caller's to
// validate: 0 <= starts[b] <= N - window.
torch::Tensor window_batch(torch::Tensor table, torch::Tensor starts,
                           int64_t window, double p, int64_t seed,
                           bool spatial) {
    TORCH_CHECK(table.is_cuda() && table.dim() == 2,
                "window_batch: table must be an (N, F) GPU tensor");
    const bool bf16 = table.scalar_type() == torch::kBFloat16;
    TORCH_CHECK(bf16 || table.scalar_type() == torch::kFloat32,
                "window_batch: table must be bf16 or fp32");
    const int64_t N = table.size(0), F = table.size(1);
    TORCH_CHECK(F >= 1 && table.stride(1) == 1 &&
                (N == 1 || table.stride(0) == F),
                "window_batch: table rows must be contiguous");
    TORCH_CHECK(starts.is_cuda() && starts.device() == table.device() &&
                starts.scalar_type() == torch::kInt64 && starts.dim() == 1 &&
                starts.is_contiguous(),
                "window_batch: starts must be a contiguous (B) int64 tensor "
                "on the table's device");
    const int64_t B = starts.size(0);
    TORCH_CHECK(B >= 1, "window_batch: no windows");
    TORCH_CHECK(window >= 1 && N >= window,
                "window_batch: window must be in [1, N]");
    TORCH_CHECK(window <= INT_MAX / F, "window_batch: window * F too large");
    TORCH_CHECK(p >= 0.0 && p < 1.0, "window_batch: p must be in [0, 1)");
    TORCH_CHECK(bf16 || p == 0.0,
                "window_batch: dropout is bf16-only; fp32 takes p == 0");
    auto out = torch::empty({B, window, F}, table.options());
    auto stream = at::hip::getCurrentHIPStream();
    const DropParams dp = drop_params(p);
    const int mode = p > 0.0 ? (spatial ? 2 : 1) : 0;
    int rc = fmda_window_batch_launch(
        bf16 ? 1 : 0, table.data_ptr(),
        (const long*)starts.data_ptr<int64_t>(), out.data_ptr(), (long)B,
        (long)window, (long)F, mode, dp.thr, dp.scale,
        (unsigned long long)seed, stream.stream());
    TORCH_CHECK(rc == 0, "window_batch launch failed rc=", rc);
    return out;
}

void ingest_row(torch::Tensor ring, torch::Tensor row, torch::Tensor xmin,
                torch::Tensor xrng) {
    TORCH_CHECK(ring.is_cuda() && ring.is_contiguous() && ring.dim() == 2 &&
                ring.scalar_type() == torch::kBFloat16,
                "ring must be (T, F) bf16 on GPU");
    TORCH_CHECK(row.is_cuda() && row.is_contiguous() &&
                row.scalar_type() == torch::kFloat32 &&
                row.numel() == ring.size(1));
    TORCH_CHECK(xmin.is_cuda() && xmin.is_contiguous() &&
                xmin.scalar_type() == torch::kFloat32 &&
                xmin.numel() == ring.size(1), "xmin must be fp32 (F) on GPU");
    TORCH_CHECK(xrng.is_cuda() && xrng.is_contiguous() &&
                xrng.scalar_type() == torch::kFloat32 &&
                xrng.numel() == ring.size(1), "xrng must be fp32 (F) on GPU");
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_ingest_row_launch(
        ring.data_ptr(), row.data_ptr<float>(), xmin.data_ptr<float>(),
        xrng.data_ptr<float>(), ring.size(0), ring.size(1), stream.stream());
    TORCH_CHECK(rc == 0, "ingest_row launch failed rc=", rc);
}

// Batched ingest_row: rings (S, T, F) bf16, rows (S, F) fp32, active (S)
// int32, xmin / xrng (S, F) fp32. Ring s is shifted and gets rows[s]
// normalized with its own table iff active[s] != 0.
void ingest_rows(torch::Tensor rings, torch::Tensor rows,
                 torch::Tensor active, torch::Tensor xmin,
                 torch::Tensor xrng) {
    TORCH_CHECK(rings.is_cuda() && rings.is_contiguous() &&
                rings.dim() == 3 &&
                rings.scalar_type() == torch::kBFloat16,
                "rings must be (S, T, F) bf16 on GPU");
    const int64_t S = rings.size(0), T = rings.size(1), F = rings.size(2);
    TORCH_CHECK(S >= 1 && T >= 1 && F >= 1 && S <= INT_MAX,
                "ingest_rows: empty rings");
    TORCH_CHECK((T - 1) * F <= 48 * 1024,
                "ingest_rows: (T-1)*F = ", (T - 1) * F,
                " exceeds the one-workgroup bound 49152");
    TORCH_CHECK(rows.is_cuda() && rows.is_contiguous() &&
                rows.scalar_type() == torch::kFloat32 && rows.dim() == 2 &&
                rows.size(0) == S && rows.size(1) == F,
                "rows must be fp32 (S, F) on GPU");
    TORCH_CHECK(active.is_cuda() && active.is_contiguous() &&
                active.scalar_type() == torch::kInt32 &&
                active.dim() == 1 && active.size(0) == S,
                "active must be int32 (S) on GPU");
    TORCH_CHECK(xmin.is_cuda() && xmin.is_contiguous() &&
                xmin.scalar_type() == torch::kFloat32 && xmin.dim() == 2 &&
                xmin.size(0) == S && xmin.size(1) == F,
                "xmin must be fp32 (S, F) on GPU");
    TORCH_CHECK(xrng.is_cuda() && xrng.is_contiguous() &&
                xrng.scalar_type() == torch::kFloat32 && xrng.dim() == 2 &&
                xrng.size(0) == S && xrng.size(1) == F,
                "xrng must be fp32 (S, F) on GPU");
    TORCH_CHECK(rows.device() == rings.device() &&
                active.device() == rings.device() &&
                xmin.device() == rings.device() &&
                xrng.device() == rings.device(),
                "ingest_rows: tensors must share a device");
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_ingest_rows_launch(
        rings.data_ptr(), rows.data_ptr<float>(), active.data_ptr<int>(),
        xmin.data_ptr<float>(), xrng.data_ptr<float>(), (int)S, (int)T,
        (int)F, stream.stream());
    TORCH_CHECK(rc == 0, "ingest_rows launch failed rc=", rc);
}

// The batch-1 LDS-resident recurrence over S independent sequences: gi
// (S, T, n_dir*3*128) bf16, w (n_dir, 384, 128) bf16, bhh (n_dir, 384) fp32
// -> out (S, T, n_dir*128) bf16, h_last (n_dir, S, 128) fp32. Zero h0, no
// dropout. Stream s gets the bits gru_fwd gives on gi[s:s+1].
std::vector<torch::Tensor> gru_fwd_streams(torch::Tensor gi, torch::Tensor w,
                                           torch::Tensor bhh) {
    TORCH_CHECK(gi.is_cuda() && gi.is_contiguous() && gi.dim() == 3 &&
                gi.scalar_type() == torch::kBFloat16,
                "gru_fwd_streams: gi must be (S, T, n_dir*384) bf16 on GPU");
    TORCH_CHECK(w.is_cuda() && w.is_contiguous() && w.dim() == 3 &&
                w.scalar_type() == torch::kBFloat16 && w.size(2) == 128 &&
                w.size(1) == 3 * 128 && (w.size(0) == 1 || w.size(0) == 2),
                "gru_fwd_streams: w must be (n_dir, 384, 128) bf16 on GPU");
    const int64_t n_dir = w.size(0), Hp = 128;
    TORCH_CHECK(bhh.is_cuda() && bhh.is_contiguous() &&
                bhh.scalar_type() == torch::kFloat32 &&
                bhh.numel() == n_dir * 3 * Hp,
                "gru_fwd_streams: bhh must be fp32 (n_dir, 384) on GPU");
    TORCH_CHECK(w.device() == gi.device() && bhh.device() == gi.device(),
                "gru_fwd_streams: tensors must share a device");
    const int64_t S = gi.size(0), T = gi.size(1);
    TORCH_CHECK(S >= 1 && S <= 65535 && T >= 1 && T <= INT_MAX,
                "gru_fwd_streams: S must be in [1, 65535] and T >= 1");
    TORCH_CHECK(gi.size(2) == n_dir * 3 * Hp,
                "gru_fwd_streams: gi last dim must be n_dir*384");
    auto out = torch::empty({S, T, n_dir * Hp}, gi.options());
    auto hlast = torch::empty({n_dir, S, Hp},
                              gi.options().dtype(torch::kFloat32));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_gru_fwd_streams_launch(
        gi.data_ptr(), w.data_ptr(), bhh.data_ptr<float>(), out.data_ptr(),
        hlast.data_ptr<float>(), (int)S, (int)T, (int)n_dir,
        stream.stream());
    TORCH_CHECK(rc != -5, "gru_fwd_streams: T=", T,
                " does not fit the 150 KB LDS cap");
    TORCH_CHECK(rc == 0, "gru_fwd_streams launch failed rc=", rc);
    return {out, hlast};
}

torch::Tensor pool_concat_infer(torch::Tensor out, torch::Tensor hlast,
                                int64_t H) {
    TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 3);
    TORCH_CHECK(hlast.is_contiguous() &&
                hlast.scalar_type() == torch::kFloat32);
    const bool bf16 = out.scalar_type() == torch::kBFloat16;
    const int B = out.size(0), T = out.size(1);
    const int n_dir = hlast.size(0);
    const int Hp = hlast.size(2);
    auto feat = torch::empty({B, 3 * H}, out.options());
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_pool_concat_launch(bf16 ? 1 : 0, out.data_ptr(),
                                     hlast.data_ptr<float>(), feat.data_ptr(),
                                     B, T, (int)H, Hp, n_dir,
                                     stream.stream());
    TORCH_CHECK(rc == 0, "pool_concat launch failed");
    return feat;
}

torch::Tensor head_sigmoid(torch::Tensor x, torch::Tensor W,
                           torch::Tensor b) {
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && W.is_contiguous() &&
                b.is_contiguous());
    TORCH_CHECK(x.scalar_type() == W.scalar_type() &&
                x.scalar_type() == b.scalar_type());
    const bool bf16 = x.scalar_type() == torch::kBFloat16;
    const int B = x.size(0), K = x.size(1), C = W.size(0);
    auto probs = torch::empty({B, C}, x.options().dtype(torch::kFloat32));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_head_sigmoid_launch(bf16 ? 1 : 0, x.data_ptr(),
                                      W.data_ptr(), b.data_ptr(),
                                      probs.data_ptr<float>(), B, K, C,
                                      stream.stream());
    TORCH_CHECK(rc == 0, "head_sigmoid launch failed");
    return probs;
}

// ---- a bank of M models behind a per-stream slot index ----
// The three ops below read slot (int32 (S), on the device) inside the
// kernel, make no host sync and launch on the current stream, so a captured
// graph follows the index between replays. The kernels clamp what they read
// into [0, M); rejecting a bad index is the caller's job, before the write.

namespace {

void check_bank_slot(const torch::Tensor& slot, const torch::Tensor& like,
                     int64_t S, const char* op) {
    TORCH_CHECK(slot.is_cuda() && slot.is_contiguous() &&
                slot.scalar_type() == torch::kInt32 && slot.dim() == 1 &&
                slot.size(0) == S,
                op, ": slot must be int32 (S) on GPU");
    TORCH_CHECK(slot.device() == like.device(),
                op, ": tensors must share a device");
    TORCH_CHECK(S >= 1 && S <= 65535, op, ": S must be in [1, 65535]");
}

bool bf16_cuda(const torch::Tensor& t, int64_t rank) {
    return t.is_cuda() && t.is_contiguous() && t.dim() == rank &&
           t.scalar_type() == torch::kBFloat16;
}

}  // namespace

// gi[s] = x[s] @ W[slot[s]]^T + b[slot[s]]: x (S, T, K), W (M, N, K),
// b (M, N) -> gi (S, T, N), bf16 with fp32 accumulation.
torch::Tensor gi_proj_bank(torch::Tensor x, torch::Tensor slot,
                           torch::Tensor W, torch::Tensor b) {
    TORCH_CHECK(bf16_cuda(x, 3),
                "gi_proj_bank: x must be (S, T, K) bf16 on GPU");
    TORCH_CHECK(bf16_cuda(W, 3),
                "gi_proj_bank: W must be (M, N, K) bf16 on GPU");
    TORCH_CHECK(bf16_cuda(b, 2),
                "gi_proj_bank: b must be (M, N) bf16 on GPU");
    const int64_t S = x.size(0), T = x.size(1), K = x.size(2);
    const int64_t M = W.size(0), N = W.size(1);
    check_bank_slot(slot, x, S, "gi_proj_bank");
    TORCH_CHECK(W.device() == x.device() && b.device() == x.device(),
                "gi_proj_bank: tensors must share a device");
    TORCH_CHECK(M >= 1 && W.size(2) == K && b.size(0) == M && b.size(1) == N,
                "gi_proj_bank: W (M, N, K) and b (M, N) must agree with x's "
                "K and with each other, M >= 1");
    TORCH_CHECK(N >= 16 && N % 16 == 0 && N <= INT_MAX,
                "gi_proj_bank: N must be a multiple of 16");
    TORCH_CHECK(T >= 1 && T <= 65535 * 32 && K >= 1 && K <= INT_MAX &&
                M <= INT_MAX && M * N <= INT_MAX,
                "gi_proj_bank: T must be in [1, 65535*32] and K >= 1");
    auto gi = torch::empty({S, T, N}, x.options());
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_gi_proj_bank_launch(
        x.data_ptr(), slot.data_ptr<int>(), W.data_ptr(), b.data_ptr(),
        gi.data_ptr(), (int)S, (int)T, (int)K, (int)N, (int)M,
        stream.stream());
    TORCH_CHECK(rc == 0, "gi_proj_bank launch failed rc=", rc);
    return gi;
}

// gru_fwd_streams with stream s on the recurrent weights of slot[s]:
// w (M, n_dir, 384, 128) bf16, bhh (M, n_dir, 384) fp32. Stream s gets the
// bits gru_fwd_streams gives on gi[s:s+1] with w[slot[s]], bhh[slot[s]].
std::vector<torch::Tensor> gru_fwd_streams_bank(torch::Tensor gi,
                                                torch::Tensor slot,
                                                torch::Tensor w,
                                                torch::Tensor bhh) {
    TORCH_CHECK(bf16_cuda(gi, 3),
                "gru_fwd_streams_bank: gi must be (S, T, n_dir*384) bf16 on "
                "GPU");
    TORCH_CHECK(bf16_cuda(w, 4) && w.size(0) >= 1 && w.size(3) == 128 &&
                w.size(2) == 3 * 128 && (w.size(1) == 1 || w.size(1) == 2),
                "gru_fwd_streams_bank: w must be (M, n_dir, 384, 128) bf16 "
                "on GPU, M >= 1");
    const int64_t M = w.size(0), n_dir = w.size(1), Hp = 128;
    TORCH_CHECK(bhh.is_cuda() && bhh.is_contiguous() &&
                bhh.scalar_type() == torch::kFloat32 && bhh.dim() == 3 &&
                bhh.size(0) == M && bhh.size(1) == n_dir &&
                bhh.size(2) == 3 * Hp,
                "gru_fwd_streams_bank: bhh must be fp32 (M, n_dir, 384) on "
                "GPU");
    const int64_t S = gi.size(0), T = gi.size(1);
    check_bank_slot(slot, gi, S, "gru_fwd_streams_bank");
    TORCH_CHECK(w.device() == gi.device() && bhh.device() == gi.device(),
                "gru_fwd_streams_bank: tensors must share a device");
    TORCH_CHECK(T >= 1 && T <= INT_MAX && M <= INT_MAX,
                "gru_fwd_streams_bank: T must be >= 1");
    TORCH_CHECK(gi.size(2) == n_dir * 3 * Hp,
                "gru_fwd_streams_bank: gi last dim must be n_dir*384");
    auto out = torch::empty({S, T, n_dir * Hp}, gi.options());
    auto hlast = torch::empty({n_dir, S, Hp},
                              gi.options().dtype(torch::kFloat32));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_gru_fwd_streams_bank_launch(
        gi.data_ptr(), slot.data_ptr<int>(), (int)M, w.data_ptr(),
        bhh.data_ptr<float>(), out.data_ptr(), hlast.data_ptr<float>(),
        (int)S, (int)T, (int)n_dir, stream.stream());
    TORCH_CHECK(rc != -5, "gru_fwd_streams_bank: T=", T,
                " does not fit the 150 KB LDS cap");
    TORCH_CHECK(rc == 0, "gru_fwd_streams_bank launch failed rc=", rc);
    return {out, hlast};
}

// head_sigmoid with row s on the head of slot[s]: feat (S, K), W (M, C, K),
// b (M, C) bf16 -> probs (S, C) fp32.
torch::Tensor head_sigmoid_bank(torch::Tensor feat, torch::Tensor slot,
                                torch::Tensor W, torch::Tensor b) {
    TORCH_CHECK(bf16_cuda(feat, 2),
                "head_sigmoid_bank: feat must be (S, K) bf16 on GPU");
    TORCH_CHECK(bf16_cuda(W, 3),
                "head_sigmoid_bank: W must be (M, C, K) bf16 on GPU");
    TORCH_CHECK(bf16_cuda(b, 2),
                "head_sigmoid_bank: b must be (M, C) bf16 on GPU");
    const int64_t S = feat.size(0), K = feat.size(1);
    const int64_t M = W.size(0), C = W.size(1);
    check_bank_slot(slot, feat, S, "head_sigmoid_bank");
    TORCH_CHECK(W.device() == feat.device() && b.device() == feat.device(),
                "head_sigmoid_bank: tensors must share a device");
    TORCH_CHECK(M >= 1 && C >= 1 && K >= 1 && W.size(2) == K &&
                b.size(0) == M && b.size(1) == C,
                "head_sigmoid_bank: W (M, C, K) and b (M, C) must agree "
                "with feat's K and with each other, M >= 1");
    TORCH_CHECK(K <= INT_MAX && S * C <= INT_MAX && M * C <= INT_MAX,
                "head_sigmoid_bank: sizes exceed int range");
    auto probs = torch::empty({S, C}, feat.options().dtype(torch::kFloat32));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_head_sigmoid_bank_launch(
        feat.data_ptr(), slot.data_ptr<int>(), W.data_ptr(), b.data_ptr(),
        probs.data_ptr<float>(), (int)S, (int)K, (int)C, (int)M,
        stream.stream());
    TORCH_CHECK(rc == 0, "head_sigmoid_bank launch failed rc=", rc);
    return probs;
}

namespace {

void check_f32_cuda(const torch::Tensor& t, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                t.scalar_type() == torch::kFloat32,
                what, " must be a contiguous fp32 GPU tensor");
}

bool compute_dtype_is_bf16(torch::ScalarType dtype) {
    TORCH_CHECK(dtype == torch::kBFloat16 || dtype == torch::kFloat32,
                "compute dtype must be bf16 or fp32");
    return dtype == torch::kBFloat16;
}

}  // namespace

// masters: [w_ih (3H,F), w_hh (3H,H), b_ih (3H), b_hh (3H)] per direction,
// fp32. Returns {w_ih_cat (D*3Hp,F), b_ih_cat (D*3Hp), w_hh_cat (D,3Hp,Hp),
// b_hh_cat (D,3Hp) fp32, wt (D,Hp,3Hp)}: gate rows zero-padded H -> Hp, the
// first three and wt in `dtype`.
std::vector<torch::Tensor> pack_gru_layer(std::vector<torch::Tensor> masters,
                                          int64_t Hp,
                                          torch::ScalarType dtype) {
    TORCH_CHECK(masters.size() == 4 || masters.size() == 8,
                "pack_gru_layer: 4 masters per direction, 1 or 2 directions");
    const int64_t D = masters.size() / 4;
    for (auto& t : masters) check_f32_cuda(t, "pack_gru_layer: master");
    TORCH_CHECK(masters[0].dim() == 2 && masters[1].dim() == 2,
                "pack_gru_layer: bad weight ranks");
    const int64_t H = masters[1].size(1), F = masters[0].size(1);
    TORCH_CHECK(H <= Hp, "pack_gru_layer: H > Hp");
    const float* ptrs[8] = {};
    for (int64_t d = 0; d < D; ++d) {
        TORCH_CHECK(masters[4 * d].sizes() == torch::IntArrayRef({3 * H, F}) &&
                    masters[4 * d + 1].sizes() ==
                        torch::IntArrayRef({3 * H, H}) &&
                    masters[4 * d + 2].sizes() == torch::IntArrayRef({3 * H}) &&
                    masters[4 * d + 3].sizes() == torch::IntArrayRef({3 * H}),
                    "pack_gru_layer: master shapes disagree");
        for (int k = 0; k < 4; ++k)
            ptrs[4 * d + k] = masters[4 * d + k].data_ptr<float>();
    }
    const bool bf16 = compute_dtype_is_bf16(dtype);
    auto opt = masters[0].options().dtype(dtype);
    auto w_ih_cat = torch::empty({D * 3 * Hp, F}, opt);
    auto b_ih_cat = torch::empty({D * 3 * Hp}, opt);
    auto w_hh_cat = torch::empty({D, 3 * Hp, Hp}, opt);
    auto b_hh_cat = torch::empty({D, 3 * Hp}, masters[0].options());
    auto wt = torch::empty({D, Hp, 3 * Hp}, opt);
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_pack_gru_layer_launch(
        bf16 ? 1 : 0, ptrs, w_ih_cat.data_ptr(), b_ih_cat.data_ptr(),
        w_hh_cat.data_ptr(), b_hh_cat.data_ptr<float>(), wt.data_ptr(),
        (int)D, (int)H, (int)Hp, (int)F, stream.stream());
    TORCH_CHECK(rc == 0, "pack_gru_layer launch failed");
    return {w_ih_cat, b_ih_cat, w_hh_cat, b_hh_cat, wt};
}

// Whether the native kernels know the order in which torch sums these
// (c, N, K) split-K partials over c. It is derived for ATen's 64 x 2 reduce
// block: 64 chunks, at least 512 outputs, whole vectors of 4.
bool eager_sum_applies(torch::Tensor parts) {
    if (parts.dim() != 3 || parts.size(0) != fmda_eager_sum_chunks())
        return false;
    const int64_t outputs = parts.size(1) * parts.size(2);
    return outputs >= 512 && outputs % 4 == 0;
}

// part_ih: (c, D*3Hp, F) split-K partials of dGi^T x; part_hh:
// (c, D*3Hp, D*Hp) partials of dGh^T out. Returns the fp32 master-shaped
// {dW_ih[0] (3H,F), dW_hh[0] (3H,H), dW_ih[1], dW_hh[1]}.
// eager_order: sum the chunks in the order of parts.float().sum(dim=0), so
// the grads equal the eager chain's bit for bit; only for partials
// eager_sum_applies() accepts.

std::vector<torch::Tensor> finalize_gru_wgrads(torch::Tensor part_ih,
                                               torch::Tensor part_hh,
                                               int64_t D, int64_t H,
                                               int64_t Hp,
                                               bool eager_order) {
    TORCH_CHECK(part_ih.is_cuda() && part_hh.is_cuda() &&
                part_ih.is_contiguous() && part_hh.is_contiguous() &&
                part_ih.dim() == 3 && part_hh.dim() == 3,
                "finalize_gru_wgrads: partials must be contiguous (c, N, K) "
                "GPU tensors");
    TORCH_CHECK(part_ih.scalar_type() == part_hh.scalar_type(),
                "finalize_gru_wgrads: partial dtypes disagree");
    const bool bf16 = compute_dtype_is_bf16(part_ih.scalar_type());
    TORCH_CHECK((D == 1 || D == 2) && H >= 1 && H <= Hp,
                "finalize_gru_wgrads: bad D / H / Hp");
    const int64_t F = part_ih.size(2);
    TORCH_CHECK(part_ih.size(1) == D * 3 * Hp &&
                part_hh.size(1) == D * 3 * Hp && part_hh.size(2) == D * Hp,
                "finalize_gru_wgrads: partial shapes disagree with D / Hp");
    auto f32 = part_ih.options().dtype(torch::kFloat32);
    std::vector<torch::Tensor> grads;
    float* ptrs[4] = {};
    for (int64_t d = 0; d < D; ++d) {
        grads.push_back(torch::empty({3 * H, F}, f32));
        grads.push_back(torch::empty({3 * H, H}, f32));
        ptrs[2 * d] = grads[2 * d].data_ptr<float>();
        ptrs[2 * d + 1] = grads[2 * d + 1].data_ptr<float>();
    }
    auto stream = at::hip::getCurrentHIPStream();
    int rc;
    if (eager_order) {
        TORCH_CHECK(eager_sum_applies(part_ih) && eager_sum_applies(part_hh),
                    "finalize_gru_wgrads: the eager sum order is known only "
                    "for 64 chunks of >= 512 outputs, a multiple of 4");
        rc = fmda_finalize_gru_wgrads_eager_launch(
            bf16 ? 1 : 0, part_ih.data_ptr(), part_hh.data_ptr(), ptrs,
            (int)D, (int)H, (int)Hp, (int)F, stream.stream());
    } else {
        rc = fmda_finalize_gru_wgrads_launch(
            bf16 ? 1 : 0, part_ih.data_ptr(), (int)part_ih.size(0),
            part_hh.data_ptr(), (int)part_hh.size(0), ptrs, (int)D, (int)H,
            (int)Hp, (int)F, stream.stream());
    }
    TORCH_CHECK(rc == 0, "finalize_gru_wgrads launch failed");
    return grads;
}

// head_loss_fwd on the fp32 master W (C, K) and b (C): each value is rounded
// to x's dtype in registers, so the results equal head_loss_fwd on W.to(x),
// b.to(x) bit for bit.
std::vector<torch::Tensor> head_loss_fwd_master(
        torch::Tensor x, torch::Tensor W, torch::Tensor b, torch::Tensor y,
        torch::Tensor wgt, torch::Tensor pw, bool staged) {
    // staged: read x and W through LDS (same bits); false keeps the direct
    // kernel reachable as the reference
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2);
    const bool bf16 = compute_dtype_is_bf16(x.scalar_type());
    check_f32_cuda(W, "head W"); check_f32_cuda(b, "head b");
    check_f32_cuda(y, "head y"); check_f32_cuda(wgt, "head weight");
    check_f32_cuda(pw, "head pos_weight");
    const int B = x.size(0), K = x.size(1), C = W.size(0);
    TORCH_CHECK(W.size(1) == K && b.numel() == C && y.numel() == (int64_t)B * C
                && wgt.numel() == C && pw.numel() == C,
                "head_loss_fwd_master: shape mismatch");
    auto f32 = x.options().dtype(torch::kFloat32);
    auto logits = torch::empty({B, C}, f32);
    auto sig = torch::empty({B, C}, f32);
    auto part = torch::empty({((int64_t)B * C + 255) / 256}, f32);
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_head_fwd_master_launch(
        bf16 ? 1 : 0, x.data_ptr(), W.data_ptr<float>(), b.data_ptr<float>(),
        y.data_ptr<float>(), wgt.data_ptr<float>(), pw.data_ptr<float>(),
        logits.data_ptr<float>(), sig.data_ptr<float>(),
        part.data_ptr<float>(), B, K, C, staged ? 1 : 0, stream.stream());
    TORCH_CHECK(rc == 0, "head fwd (master) launch failed");
    return {logits, sig, part.sum().reshape({1}), part};
}

std::vector<torch::Tensor> head_loss_bwd_master(
        torch::Tensor sig, torch::Tensor y, torch::Tensor wgt,
        torch::Tensor pw, torch::Tensor gscale, torch::Tensor W,
        torch::ScalarType xdtype, bool emit_cast) {
    // emit_cast: also return dlogits.to(xdtype), written by the same kernel
    // (dlogits itself when xdtype is fp32)
    check_f32_cuda(sig, "head sig"); check_f32_cuda(y, "head y");
    check_f32_cuda(wgt, "head weight"); check_f32_cuda(pw, "head pos_weight");
    check_f32_cuda(gscale, "head gscale"); check_f32_cuda(W, "head W");
    const int B = sig.size(0), C = sig.size(1), K = W.size(1);
    TORCH_CHECK(W.size(0) == C && y.numel() == sig.numel() &&
                wgt.numel() == C && pw.numel() == C && gscale.numel() == 1,
                "head_loss_bwd_master: shape mismatch");
    const bool bf16 = compute_dtype_is_bf16(xdtype);
    auto dlogits = torch::empty_like(sig);
    auto dx = torch::empty({B, K}, sig.options().dtype(xdtype));
    torch::Tensor dl_t;
    if (emit_cast && bf16)
        dl_t = torch::empty({B, C}, sig.options().dtype(xdtype));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_head_bwd_master_launch(
        bf16 ? 1 : 0, sig.data_ptr<float>(), y.data_ptr<float>(),
        wgt.data_ptr<float>(), pw.data_ptr<float>(),
        gscale.data_ptr<float>(), W.data_ptr<float>(),
        dlogits.data_ptr<float>(), dl_t.defined() ? dl_t.data_ptr() : nullptr,
        dx.data_ptr(), B, K, C, stream.stream());
    TORCH_CHECK(rc == 0, "head bwd (master) launch failed");
    if (!emit_cast) return {dlogits, dx};
    return {dlogits, dx, bf16 ? dl_t : dlogits};
}

// dW (C, K) and db (C) of the head as the eager chain leaves them: parts
// (64, C, K) are the split-K partials of dlogits.to(x)^T x, db_sum is
// dlogits.sum(0). dW = parts.float().sum(0).to(x).to(fp32) in that sum's
// order, db = db_sum.to(x).to(fp32); one launch.
std::vector<torch::Tensor> head_wgrads_eager(torch::Tensor parts,
                                             torch::Tensor db_sum) {
    TORCH_CHECK(parts.is_cuda() && parts.is_contiguous() &&
                eager_sum_applies(parts),
                "head_wgrads_eager: parts must be contiguous (64, C, K) GPU "
                "partials with C*K >= 512, a multiple of 4");
    check_f32_cuda(db_sum, "head db_sum");
    const bool bf16 = compute_dtype_is_bf16(parts.scalar_type());
    const int C = parts.size(1), K = parts.size(2);
    TORCH_CHECK(db_sum.numel() == C && db_sum.is_contiguous(),
                "head_wgrads_eager: shape mismatch");
    auto f32 = db_sum.options();
    auto dW = torch::empty({C, K}, f32);
    auto db = torch::empty({C}, f32);
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_head_wgrads_eager_launch(
        bf16 ? 1 : 0, parts.data_ptr(), db_sum.data_ptr<float>(),
        dW.data_ptr<float>(), db.data_ptr<float>(), K, C, stream.stream());
    TORCH_CHECK(rc == 0, "head_wgrads_eager launch failed");
    return {dW, db};
}

// Exact-match ratio of a (B, C) batch: target fp32 or bool, pred bool, both
// contiguous. 0-dim fp32, the value of
// (target.bool() == pred).all(1).float().mean().
torch::Tensor subset_accuracy(torch::Tensor target, torch::Tensor pred) {
    TORCH_CHECK(target.is_cuda() && pred.is_cuda() && target.dim() == 2 &&
                target.sizes() == pred.sizes() && target.is_contiguous() &&
                pred.is_contiguous() && pred.scalar_type() == torch::kBool &&
                target.device() == pred.device(),
                "subset_accuracy: need contiguous (B, C) GPU tensors, pred "
                "bool");
    const bool tf = target.scalar_type() == torch::kFloat32;
    TORCH_CHECK(tf || target.scalar_type() == torch::kBool,
                "subset_accuracy: target must be fp32 or bool");
    const int64_t B = target.size(0), C = target.size(1);
    // one block walks the rows; the count stays exact in fp32
    TORCH_CHECK(B >= 1 && B <= (1 << 16) && C >= 1 && C <= (1 << 16),
                "subset_accuracy: 1 <= B, C <= 65536");
    auto out = torch::empty({}, target.options().dtype(torch::kFloat32));
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_subset_accuracy_launch(
        tf ? 1 : 0, target.data_ptr(), pred.data_ptr(),
        out.data_ptr<float>(), (int)B, (int)C, stream.stream());
    TORCH_CHECK(rc == 0, "subset_accuracy launch failed");
    return out;
}

// dW (C, K) = round_x(dlogits)^T x and db (C) = sum_rows dlogits, both fp32,
// reduced over the batch in two fixed-order stages.
std::vector<torch::Tensor> head_wgrads(torch::Tensor dlogits,
                                       torch::Tensor x) {
    check_f32_cuda(dlogits, "head dlogits");
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2 &&
                dlogits.dim() == 2 && dlogits.size(0) == x.size(0),
                "head_wgrads: shape mismatch");
    const bool bf16 = compute_dtype_is_bf16(x.scalar_type());
    const int B = x.size(0), K = x.size(1), C = dlogits.size(1);
    const int64_t n_slabs = fmda_head_wgrads_slabs(B);
    auto f32 = dlogits.options();
    auto dw_part = torch::empty({n_slabs, C, K}, f32);
    auto db_part = torch::empty({n_slabs, C}, f32);
    auto dW = torch::empty({C, K}, f32);
    auto db = torch::empty({C}, f32);
    auto stream = at::hip::getCurrentHIPStream();
    int rc = fmda_head_wgrads_launch(
        bf16 ? 1 : 0, dlogits.data_ptr<float>(), x.data_ptr(),
        dw_part.data_ptr<float>(), db_part.data_ptr<float>(),
        dW.data_ptr<float>(), db.data_ptr<float>(), B, K, C,
        stream.stream());
    TORCH_CHECK(rc == 0, "head_wgrads launch failed");
    return {dW, db};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("gru_fwd", &gru_fwd, "fused biGRU recurrence forward (HIP/CDNA4)",
          py::arg("gi"), py::arg("w"), py::arg("bhh"),
          py::arg("h0") = py::none(), py::arg("drop_p") = 0.0,
          py::arg("drop_seed") = 0);
    m.def("gru_fwd_windows", &gru_fwd_windows,
          "biGRU recurrence forward over sliding windows of a projection "
          "table (shared rows, no materialised windows)",
          py::arg("gi_rows"), py::arg("w"), py::arg("bhh"), py::arg("T"),
          py::arg("stride") = 1);
    m.def("normalize_table", &normalize_table,
          "nan_to_num + min/max normalisation of a raw (N, F) table",
          py::arg("x"), py::arg("x_min"), py::arg("x_max"), py::arg("dtype"));
    m.def("window_batch", &window_batch,
          "gather windows of a table into a (B, T, F) batch with fused "
          "(spatial) input dropout",
          py::arg("table"), py::arg("starts"), py::arg("window"),
          py::arg("p"), py::arg("seed"), py::arg("spatial"));
    m.def("gru_bwd", &gru_bwd, "fused biGRU recurrence backward (HIP/CDNA4)",
          py::arg("gi"), py::arg("w"), py::arg("bhh"), py::arg("out"),
          py::arg("dout"), py::arg("dhT"), py::arg("drop_p") = 0.0,
          py::arg("drop_seed") = 0, py::arg("h0") = py::none(),
          py::arg("wt") = py::none(), py::arg("dfeat") = py::none(),
          py::arg("amax") = py::none());
    m.def("mfma_selftest", &mfma_selftest, "mfma fragment layout self-test");
    m.def("dropout_fused", &dropout_fused,
          "counter-based dropout (mask recomputed in backward)");
    m.def("spatial_dropout_fused", &spatial_dropout_fused,
          "channel (Dropout2d) dropout over (B, T, F) without permutes");
    m.def("ingest_row", &ingest_row,
          "streaming ingest: shift GPU window ring + normalize new row");
    m.def("ingest_rows", &ingest_rows,
          "fleet ingest: ingest_row on the active rings of (S, T, F), each "
          "with its own normalisation table",
          py::arg("rings"), py::arg("rows"), py::arg("active"),
          py::arg("xmin"), py::arg("xrng"));
    m.def("gru_fwd_streams", &gru_fwd_streams,
          "batch-1 LDS-resident recurrence over S independent sequences",
          py::arg("gi"), py::arg("w"), py::arg("bhh"));
    m.def("gi_proj_bank", &gi_proj_bank,
          "grouped input projection: stream s through W[slot[s]], b[slot[s]]",
          py::arg("x"), py::arg("slot"), py::arg("W"), py::arg("b"));
    m.def("gru_fwd_streams_bank", &gru_fwd_streams_bank,
          "gru_fwd_streams with stream s on the recurrent weights of slot[s]",
          py::arg("gi"), py::arg("slot"), py::arg("w"), py::arg("bhh"));
    m.def("head_sigmoid_bank", &head_sigmoid_bank,
          "head_sigmoid with row s on the head of slot[s]",
          py::arg("feat"), py::arg("slot"), py::arg("W"), py::arg("b"));
    m.def("pool_concat_infer", &pool_concat_infer,
          "fused [dirsum(h_last) | max | avg] concat for inference");
    m.def("head_sigmoid", &head_sigmoid,
          "linear head + sigmoid emitting probabilities");
    m.def("pool_fwd", &pool_fwd, "fused dirsum+max/avg pooling forward",
          py::arg("out"), py::arg("n_dir"), py::arg("act_dtype") = false,
          py::arg("serial") = false);
    m.def("pool_features_fwd", &pool_features_fwd,
          "[dirsum(h_last) | max | avg] features + argmax in one kernel",
          py::arg("out"), py::arg("h_last"));
    m.def("pool_features_bwd", &pool_features_bwd,
          "d_out and d_hlast of pool_features_fwd in one kernel",
          py::arg("dfeat"), py::arg("amax"), py::arg("T"), py::arg("n_dir"));
    m.def("pool_bwd", &pool_bwd, "fused pooling backward (d_out assembly)");
    m.def("head_loss_fwd", &head_loss_fwd, "fused head GEMM + BCE loss");
    m.def("head_loss_bwd", &head_loss_bwd, "fused head/loss backward");
    m.def("pack_gru_layer", &pack_gru_layer,
          "fp32 masters -> padded compute-dtype layer weights (+ W_hh^T)");
    m.def("finalize_gru_wgrads", &finalize_gru_wgrads,
          "split-K partials -> master-shaped fp32 dW_ih / dW_hh",
          py::arg("part_ih"), py::arg("part_hh"), py::arg("D"), py::arg("H"),
          py::arg("Hp"), py::arg("eager_order") = false);
    m.def("eager_sum_applies", &eager_sum_applies,
          "whether the eager chunk-sum order is known for these partials");
    m.def("head_loss_fwd_master", &head_loss_fwd_master,
          "fused head GEMM + BCE loss reading the fp32 master W / b; "
          "returns (logits, sig, loss_sum, block partials)",
          py::arg("x"), py::arg("W"), py::arg("b"), py::arg("y"),
          py::arg("wgt"), py::arg("pw"), py::arg("staged") = true);
    m.def("head_loss_bwd_master", &head_loss_bwd_master,
          "fused head/loss backward reading the fp32 master W",
          py::arg("sig"), py::arg("y"), py::arg("wgt"), py::arg("pw"),
          py::arg("gscale"), py::arg("W"), py::arg("xdtype"),
          py::arg("emit_cast") = false);
    m.def("head_wgrads_eager", &head_wgrads_eager,
          "head dW / db from the split-K partials, the eager chain's bits");
    m.def("subset_accuracy", &subset_accuracy,
          "exact-match ratio of a (B, C) multilabel batch in one kernel");
    m.def("head_wgrads", &head_wgrads,
          "head dW / db in fp32, two-stage fixed-order batch reduction");
    m.def("fused_clip_adam", &fused_clip_adam,
          "fused multi-tensor grad-clip + Adam step");
    m.def("save_state_dict_native", &fmda_ckpt::save_state_dict,
          "write a torch.load-compatible zip state_dict (native C++)");
    m.def("load_state_dict_native", &fmda_ckpt::load_state_dict,
          "read a torch.save zip state_dict (native C++)");
}
