// Functions that one file of the library defines and another calls, outside the C ABI.  The defining files (gemm.hip, norm.hip,
// elem.hip, attn_fused.hip) include this header as well as the callers, so a drifted signature does not compile, and the link
// refuses undefined symbols (-z defs).  Default arguments are stated here only.  At the end: the one device function two files
// share (the B-spline evaluation of the KAN forward and of the KAN grid update).
#pragma once
#include "hs_common.h"

namespace hs {

// ---- gemm.hip ----
// rg (optional, internal callers only): the residual is compact, see ResGather
int gemm_impl(const hs_gemm_params* p, hipStream_t stream, const ResGather* rg = nullptr);
int gemm_stat_rows(const hs_gemm_params* p);
int gemm_bn_finish_rows(const hs_gemm_params* p);
int gemm_tile_rows(const hs_gemm_params* p);
int gemm_bnb_finish_rows(const hs_gemm_params* p);
void gemm_group_set_immediate_hook(int (*fn)(void*), void* ctx);
struct GemmGroup;
GemmGroup* gemm_group_open(hipStream_t s, long long slot);   // slot: any key that is stable across steps (its device table is cached)
// k_cols (device, or NULL): the operands' K columns are chunk-compacted and the walk ends behind column *k_cols (GemmArgs.k_cols).
// Only a QUEUED problem can carry it -- one that would be launched on its own is refused -- and gemm_group_takes_k_cols() says
// beforehand whether K-contiguous bf16 problems are queued at all (they are unless a measurement override is armed).
int gemm_group_add(GemmGroup* g, const hs_gemm_params* p, hipStream_t s, const int* k_cols = nullptr);
bool gemm_group_takes_k_cols();
int gemm_group_flush(GemmGroup* g, hipStream_t s);
void gemm_group_upload_on_stream(GemmGroup* g);       // a changed problem table travels on the stream, no synchronise
long long gemm_group_uploads(const GemmGroup* g);
long long gemm_group_launches(const GemmGroup* g);

// ---- attn_fused.hip ----
int attention_bwd_fused(const hs_attn_desc& d, const void* q, const void* k, const void* v, const void* dO, void* dq, void* dk,
                        void* dv, const void* P, int ldP, void* scratch, long long scratch_bytes, const void* O, hipStream_t s,
                        const int* cu);
int attention_fwd_fused(const hs_attn_desc& d, const void* q, const void* k, const void* v, void* o, void* P, void* Pd, int ldP,
                        hipStream_t s, const int* cu);

// ---- norm.hip ----
// lean forms of the image tower's BatchNorm / max-pool passes (bf16 only, see img_lean in blocks.hip)
int bn_fwd_dsres(const hs_bn_params* p, const void* c_ds, const float* scale_ds, const float* shift_ds, hipStream_t s);
int bn_relu_maxpool_fwd(const void* c, const float* scale, const float* shift, void* y, void* idx, int N, int H, int W, int C,
                        hipStream_t s);
int bn_bwd_pooled(const hs_bn_bwd_params* p, const void* idx, int N, int H, int W, hipStream_t s);
long long bn_bwd_pair_ws_bytes(long long M, int C);
int bn_bwd_pair(const hs_bn_bwd_params* p, const hs_bn_bwd_params* pd, hipStream_t s);
// packed-row forms of the row-wise kernels (norm.hip, elem.hip): nrows / row_of / inv / packed_of NULL = every row, as the C ABI
// entries.  Kernels that SUM over rows (LayerNorm backward, column sums, the transposes a weight gradient reads) take inv and walk
// the padded rows, so that their sums have the padded tower's terms in the padded tower's order: the results are bitwise its results
int ln_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, long long M, int H,
           float eps, hipStream_t s, const int* nrows);
int ln_bwd(int dtype, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
           float* dbeta, float* ws, long long ws_bytes, long long M, int H, hipStream_t s, const int* inv);
int ln_bwd_pre(int dtype, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
               float* dgamma, float* dbeta, void* dx_dropped, float* dbias, float p, unsigned long long seed, float* ws,
               long long ws_bytes, long long M, int H, hipStream_t s, const int* inv);

// ---- elem.hip ----
int colsum_multi(int count, const int* dtype, const void* const* x, const long long* M, const int* N, const int* ld, float* const* out,
                 float* const* ws, hipStream_t s, int* launches);
int transpose_bf16_multi_rows(int count, const void* const* src, void* const* dst, const int32_t* R, const int32_t* Cc,
                              const int64_t* ld_src, const int64_t* ld_dst, const int* inv, const unsigned char* tok, const int* kc,
                              const int* kc_pos, hipStream_t stream);
int colsum_rows(int dtype, const void* x, long long M, int N, int ld, float* out, void* ws, long long ws_bytes, int accumulate,
                const int* inv, hipStream_t s);
int dropout_rows(int dtype, const void* x, void* out, long long M, int H, float p, unsigned long long seed, const int* nrows,
                 const int* row_of, hipStream_t s);
long long bert_row_map_bytes(int B, int L);
int bert_row_map(const int64_t* mask, int B, int L, int* map, hipStream_t s);
int bert_unpack_rows(const void* y, void* out, long long rows, long long row_bytes, const int* packed_of, hipStream_t s);
int bert_pack_rows(const void* dy, void* dst, long long rows, long long row_bytes, const int* nrows, const int* row_of,
                   const int* word_src, int* word_dst, hipStream_t s);
int bert_embed_fwd_rows(int dtype, const int64_t* ids, const float* word, const float* pos, const float* type0, const float* gamma,
                        const float* beta, void* sum_out, void* y, float* mean, float* rstd, long long tokens, int L, int H, int V,
                        float eps, float dropout_p, unsigned long long seed, const int* nrows, const int* row_of, hipStream_t stream);
int bert_embed_bwd_rows(int dtype, const int64_t* ids, const void* dsum, float* dword, float* dpos, int B, int L, int H, int V,
                        int pad_id, const int* nrows, const int* row_of, const int* packed_of, hipStream_t s);

// ---- kan_moe.hip, kan_grid.hip (device) ----
constexpr int KAN_MAXK = 32;   // knots per feature: grid_size + 2*order + 1 <= 32

// Cox-de Boor recursion exactly as kan1.py:92-103, carried in forward mode so the derivative equals what
// autograd produces for that formula: B (and dB/dx) of order `order`, nb = G + order values.  The forward, its backward and
// the re-fit of kan_grid.hip all evaluate their bases here, so a fit sees the values the forward produces.
__device__ __forceinline__ void bspline_eval(float x, const float* __restrict__ g, int nk, int order, float* B, float* dB) {
    const int n0 = nk - 1;
    for (int j = 0; j < n0; ++j) {
        B[j] = (x >= g[j] && x < g[j + 1]) ? 1.f : 0.f;
        dB[j] = 0.f;
    }
    for (int k = 1; k <= order; ++k) {
        const int n = n0 - k;
        for (int j = 0; j < n; ++j) {
            const float d1 = g[j + k] - g[j], d2 = g[j + k + 1] - g[j + 1];
            const float a = (x - g[j]) / d1, c = (g[j + k + 1] - x) / d2;
            const float nb = a * B[j] + c * B[j + 1];
            const float nd = B[j] / d1 + a * dB[j] - B[j + 1] / d2 + c * dB[j + 1];
            B[j] = nb;
            dB[j] = nd;
        }
    }
}

}  // namespace hs
