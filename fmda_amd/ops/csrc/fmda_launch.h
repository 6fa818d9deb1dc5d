// The one declaration of every host entry point of the extension's .hip and
// .cpp files. bindings.cpp calls through it, and every file that defines a
// launcher includes it too: `extern "C"` symbols carry no signature, so only
// a shared declaration lets the compiler reject a definition whose parameter
// list has drifted from what the callers pass.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

// ---- gru_kernels.hip -------------------------------------------------------
extern "C" int fmda_gru_fwd_launch(int is_bf16, int Hp, const void* gi,
                                   const void* w, const float* bhh, void* out,
                                   float* hlast, int B, int Tseq, int n_dir,
                                   const float* h0, void* out_drop,
                                   unsigned int drop_thr, float drop_scale,
                                   unsigned long long drop_seed,
                                   long gi_pitch, hipStream_t stream);
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
                                   hipStream_t stream);
extern "C" int fmda_gru_bwd_db_rows(int is_bf16, int Hp, int B,
                                    int column_split);
extern "C" int fmda_gru_db_reduce_launch(const float* part, int rows,
                                         int n_dir, int Hp, float* dbhh,
                                         float* dbih, hipStream_t stream);
extern "C" int fmda_gru_bwd_pooled_launch(const void* gi, const void* w,
                                          const void* wt, const float* bhh,
                                          const void* out, const void* dfeat,
                                          const int* amax, long ld, void* dgi,
                                          void* dgh, float* dh0, float* dbhh,
                                          int B, int Tseq, int n_dir,
                                          const float* h0, void* dgh0,
                                          hipStream_t stream);
extern "C" int fmda_gru_fwd_b1_launch(const void* gi, const void* w,
                                      const float* bhh, void* out,
                                      float* hlast, int Tseq, int n_dir,
                                      const float* h0, hipStream_t stream);
extern "C" int fmda_gru_fwd_streams_launch(const void* gi, const void* w,
                                           const float* bhh, void* out,
                                           float* hlast, int S, int Tseq,
                                           int n_dir, hipStream_t stream);
extern "C" int fmda_gru_fwd_streams_bank_launch(
    const void* gi, const int* slot, int M, const void* w, const float* bhh,
    void* out, float* hlast, int S, int Tseq, int n_dir, hipStream_t stream);
extern "C" int fmda_gi_proj_bank_launch(const void* x, const int* slot,
                                        const void* W, const void* b,
                                        void* gi, int S, int Tseq, int K,
                                        int N, int M, hipStream_t stream);
extern "C" int fmda_head_sigmoid_bank_launch(const void* x, const int* slot,
                                             const void* W, const void* bias,
                                             float* probs, int B, int K,
                                             int C, int M,
                                             hipStream_t stream);

extern "C" int fmda_gru_fwd_cs_launch(const void* gi, const void* w,
                                      const float* bhh, void* out,
                                      float* hlast, void* hpub,
                                      unsigned int* cnt, int B, int Tseq,
                                      int n_dir, void* out_drop,
                                      unsigned int drop_thr,
                                      float drop_scale,
                                      unsigned long long drop_seed,
                                      long gi_pitch, hipStream_t stream);
extern "C" int fmda_gru_bwd_cs_launch(const void* gi, const void* w,
                                      const void* wt, const float* bhh,
                                      const void* out, const void* dout,
                                      const float* dhT, void* dgi, void* dgh,
                                      float* dh0, float* dbhh, void* gpub,
                                      unsigned int* cnt, int B, int Tseq,
                                      int n_dir, unsigned int drop_thr,
                                      float drop_scale,
                                      unsigned long long drop_seed,
                                      hipStream_t stream);
extern "C" int fmda_mfma_selftest_launch(const void* A, const void* Bm,
                                         float* C, hipStream_t stream);
extern "C" int fmda_pool_fwd_launch(int is_bf16, const void* out, void* maxv,
                                    void* avgv, int* amax, int B, int Tseq,
                                    int H, int n_dir, int act_io, int serial,
                                    hipStream_t stream);
extern "C" int fmda_pool_bwd_launch(int is_bf16, const void* dmax,
                                    const void* davg, const int* amax,
                                    void* dout, int B, int Tseq, int H,
                                    int n_dir, int act_io, long ld_max,
                                    long ld_avg, hipStream_t stream);
extern "C" int fmda_pool_features_fwd_launch(const void* out,
                                             const float* hlast, void* feat,
                                             int* amax, int B, int Tseq,
                                             int H, int n_dir,
                                             hipStream_t stream);
extern "C" int fmda_pool_features_bwd_launch(const void* dfeat,
                                             const int* amax, void* dout,
                                             float* dhlast, int B, int Tseq,
                                             int H, int n_dir, long ld,
                                             hipStream_t stream);
extern "C" int fmda_dropout_launch(int is_bf16, const void* x, void* y,
                                   long n, unsigned int thr, float scale,
                                   unsigned long long seed,
                                   hipStream_t stream);
extern "C" int fmda_spatial_dropout_launch(int is_bf16, const void* x,
                                           void* y, long B, long Tlen, long F,
                                           unsigned int thr, float scale,
                                           unsigned long long seed,
                                           hipStream_t stream);
extern "C" int fmda_ingest_row_launch(void* ring, const float* row,
                                      const float* xmin, const float* xrng,
                                      int Tseq, int F, hipStream_t stream);
extern "C" int fmda_ingest_rows_launch(void* rings, const float* rows,
                                       const int* active, const float* xmin,
                                       const float* xrng, int S, int Tseq,
                                       int F, hipStream_t stream);
extern "C" int fmda_pool_concat_launch(int is_bf16, const void* out,
                                       const float* hlast, void* feat, int B,
                                       int Tseq, int H, int Hp, int n_dir,
                                       hipStream_t stream);
extern "C" int fmda_head_sigmoid_launch(int is_bf16, const void* x,
                                        const void* W, const void* bias,
                                        float* probs, int B, int K, int C,
                                        hipStream_t stream);
extern "C" int fmda_head_fwd_launch(int is_bf16, const void* x, const void* W,
                                    const void* bias, const float* y,
                                    const float* wgt, const float* pw,
                                    float* logits, float* sig,
                                    float* loss_sum, int B, int K, int C,
                                    hipStream_t stream);
extern "C" int fmda_head_bwd_launch(int is_bf16, const float* sig,
                                    const float* y, const float* wgt,
                                    const float* pw, const float* gscale,
                                    const void* W, float* dlogits, void* dx,
                                    int B, int K, int C, hipStream_t stream);

// ---- glue_kernels.hip ------------------------------------------------------
extern "C" int fmda_pack_gru_layer_launch(
        int is_bf16, const float* const* masters, void* w_ih_cat,
        void* b_ih_cat, void* w_hh_cat, float* b_hh_cat, void* wt, int D,
        int H, int Hp, int F, hipStream_t stream);
extern "C" int fmda_finalize_gru_wgrads_launch(
        int part_bf16, const void* part_ih, int c_ih, const void* part_hh,
        int c_hh, float* const* grads, int D, int H, int Hp, int F,
        hipStream_t stream);
extern "C" int fmda_finalize_gru_wgrads_eager_launch(
        int part_bf16, const void* part_ih, const void* part_hh,
        float* const* grads, int D, int H, int Hp, int F,
        hipStream_t stream);
extern "C" int fmda_eager_sum_chunks();
extern "C" int fmda_head_wgrads_eager_launch(
        int is_bf16, const void* parts, const float* db_sum, float* dW,
        float* db, int K, int C, hipStream_t stream);
extern "C" int fmda_subset_accuracy_launch(
        int target_is_float, const void* target, const void* pred,
        float* out, int B, int C, hipStream_t stream);
extern "C" int fmda_head_fwd_master_launch(
        int is_bf16, const void* x, const float* W, const float* bias,
        const float* y, const float* wgt, const float* pw, float* logits,
        float* sig, float* loss_sum, int B, int K, int C, int staged,
        hipStream_t stream);
extern "C" int fmda_head_bwd_master_launch(
        int is_bf16, const float* sig, const float* y, const float* wgt,
        const float* pw, const float* gscale, const float* W,
        float* dlogits, void* dlogits_t, void* dx, int B, int K, int C,
        hipStream_t stream);
extern "C" int fmda_normalize_table_launch(
        int out_bf16, const float* x, const float* xmin, const float* xmax,
        void* y, long N, int F, hipStream_t stream);
extern "C" int fmda_window_batch_load_bytes(const void* table, long TF,
                                            long F, int es);
extern "C" int fmda_window_batch_launch(
        int is_bf16, const void* table, const long* starts, void* out,
        long B, long Tlen, long F, int mode, unsigned int thr, float scale,
        unsigned long long seed, hipStream_t stream);
extern "C" int fmda_head_wgrads_slabs(int B);
extern "C" int fmda_head_wgrads_launch(
        int is_bf16, const float* dlogits, const void* x, float* dw_part,
        float* db_part, float* dW, float* db, int B, int K, int C,
        hipStream_t stream);

// ---- optim_kernels.hip -----------------------------------------------------
extern "C" int fmda_opt_norm2_launch(const void* chunks, int n_chunks,
                                     float* out, hipStream_t stream);
extern "C" int fmda_opt_adam_launch(const void* chunks, int n_chunks,
                                    const float* norm2, float clip, float lr,
                                    float beta1, float beta2, float eps,
                                    float bc1, float bc2, hipStream_t stream);

// ---- checkpoint.cpp --------------------------------------------------------
// torch::Tensor is at::Tensor; the forward declaration keeps this header free
// of torch includes for the .hip files.
namespace at { class Tensor; }
namespace fmda_ckpt {
void save_state_dict(const std::string& path,
                     const std::vector<std::string>& keys,
                     const std::vector<at::Tensor>& tensors);
std::vector<std::pair<std::string, at::Tensor>> load_state_dict(
        const std::string& path);
}  // namespace fmda_ckpt
