/*
 * hamspine.h -- C ABI of libhamspine_hip.so (MI355X / gfx950 only).
 *
 * This is the drop-in boundary underneath the reference's Python nn.Module surface
 * (reference: model.py:21-345, encoder.py:13-134, modules/fusion_blocks.py, modules/heads.py,
 * mibf_net/model_resnet.py:10-94, mibf_net/attention.py:31-70).  The reference has no FFI of its
 * own: every kernel it runs is an ATen/cuDNN/cuBLAS kernel chosen by torchvision / transformers /
 * torch.nn.  Each entry point below names the reference call site whose arithmetic it replaces.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; the caller owns every buffer (device memory).
 *   - `stream` is a hipStream_t passed as void*.
 *   - every function returns hs_status (0 = ok); hs_last_error() gives the text (thread local).
 *   - element types: HS_F32 (exact mode, f32-in MFMA == fmaf chain) or HS_BF16 (throughput mode,
 *     bf16-in MFMA, f32 accumulate).  Parameters, biases, norm scales, statistics, losses and
 *     parameter gradients are always f32.
 *   - image activations are NHWC ("channels_last") in memory.
 */
#ifndef HAMSPINE_H
#define HAMSPINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int hs_status;
enum { HS_OK = 0, HS_ERR_ARG = 1, HS_ERR_HIP = 2, HS_ERR_UNSUPPORTED = 3 };
enum { HS_F32 = 0, HS_BF16 = 1 };

const char* hs_last_error(void);
int hs_version(void);
/* 1 if a gfx950 device is visible; never throws. */
int hs_device_ok(void);

/* ------------------------------------------------------------------------------------------- */
/* GEMM / implicit-GEMM convolution core                                                        */
/*   D[m][n] = epilogue( alpha * sum_k A(m,k) * B(n,k) )                                        */
/* Replaces: torch.nn.functional.linear / conv2d and their backward (cuBLAS / cuDNN under the   */
/* reference's torchvision ResNet, encoder.py:35-42, and transformers BertLayer, encoder.py:131).*/
/* ------------------------------------------------------------------------------------------- */

/* how operand A supplies A(m,k) */
enum {
    HS_A_KC = 0,     /* A[m*lda + k]                      (k contiguous)                        */
    HS_A_RC = 1,     /* A[k*lda + m]                      (m contiguous; "transposed" operand)  */
    HS_A_CONV = 2,   /* im2col gather from an NHWC image: m=(n,p,q), k=(r,s,c)     (conv fwd)   */
    HS_A_DGRAD = 3   /* gather from dY (NPQK):            m=(n,h,w), k=(r,s,ko)    (conv dgrad) */
};
/* how operand B supplies B(n,k) */
enum {
    HS_B_KC = 0,     /* B[n*ldb + k]                                                            */
    HS_B_RC = 1,     /* B[k*ldb + n]                                                            */
    HS_B_WDGRAD = 2, /* filter KRSC read as n=c, k=(r,s,ko)                       (conv dgrad)  */
    HS_B_CONV = 3    /* im2col gather with n=(r,s,c), k=(n,p,q)                   (conv wgrad)  */
};
enum { HS_ACT_NONE = 0, HS_ACT_RELU = 1, HS_ACT_GELU = 2 };
/* epilogue multiplier modes (backward) */
enum { HS_MUL_NONE = 0, HS_MUL_GELU_GRAD = 1, HS_MUL_RELU_MASK = 2 };

typedef struct hs_conv_geom {
    int32_t N, H, W, C;      /* input image: batch, height, width, channels                     */
    int32_t P, Q, K;         /* output image: height, width, channels                           */
    int32_t R, S;            /* filter                                                          */
    int32_t stride, pad;
    int32_t row_pitch;       /* elements between input rows   (W*C unless pre-padded)           */
    int32_t img_pitch;       /* elements between input images (H*row_pitch)                     */
    int32_t qstep;           /* elements per output-column step (stride*C unless stem packing)  */
    int32_t no_bounds;       /* 1: the input is pre-padded, skip the h/w range test             */
} hs_conv_geom;

struct hs_bn_params;
typedef struct hs_gemm_params {
    int32_t dtype;           /* element type of A and B (HS_F32 | HS_BF16)                      */
    int32_t a_kind, b_kind;
    int32_t M, N, K;
    const void* A;
    const void* B;
    int64_t a_elems, b_elems; /* addressable elements behind A / B (bounds for buffer loads)    */
    int32_t lda, ldb;
    hs_conv_geom g;
    /* batching: blockIdx.z = b; operand offset = (b / batch_inner)*bs0 + (b % batch_inner)*bs1 */
    int32_t batch, batch_inner;
    int64_t a_bs0, a_bs1, b_bs0, b_bs1, d_bs0, d_bs1;
    /* split-K (batch must be 1): partial sums go to `splitk_ws` (f32, hs_gemm_splitk_ws_bytes(p) bytes: one M*N slab per
       slice plus, beyond 8 slices, one per group of 8).  bf16: reduced inside the launch (two-level last-arriver hand-off,
       fixed summation order) before the epilogue; f32: by a second kernel that applies the epilogue.  0/1 = off. */
    int32_t split_k;
    float* splitk_ws;
    /* epilogue */
    void* D;
    int32_t ldd;
    int32_t out_dtype;       /* HS_F32 | HS_BF16                                                */
    float alpha;
    const float* bias;       /* [N] or NULL                                                     */
    int32_t act;
    void* D_preact;          /* optional second output: value before `act` (same type/ld as D)  */
    const void* residual;    /* optional, added last; same type as D                            */
    int32_t ldr;
    float dropout_p;         /* applied after act, before residual                              */
    uint64_t dropout_seed;
    int32_t mul_mode;        /* backward multipliers                                            */
    const void* mul_src;     /* u (GELU input) or y (ReLU output); same type as A, ld = ldm     */
    int32_t ldm;
    int32_t accumulate;      /* 1: D += result (f32 outputs only)                               */
    /* segmented output (optional): rows [i*seg_rows, (i+1)*seg_rows) go to D_seg[i-1] for i = 1, 2 (row index
       rebased), rows below seg_rows to D.  Lets one GEMM write three parameter gradients (fused QKV wgrad). */
    int32_t seg_rows;
    void* D_seg[2];
    /* optional per-column scale applied before the bias: v = alpha * acc * colscale[n] + bias[n] (an eval-mode BatchNorm
       folded into the convolution), and residual_before_act = 1 to add `residual` before the activation
       (y = relu(bn(conv) + identity)) instead of after it */
    const float* colscale;
    int32_t residual_before_act;
    /* optional (bf16 operands, no split-K, no batching): per (row tile, column) statistics of the result for a following
       BatchNorm, written as (count, mean, M2) triples to colstats[(tile_row * N + n) * 3 ...]; hs_gemm_stat_rows(p) gives
       the number of tile rows.  Saves BatchNorm's own pass over the convolution output (hs_bn_params.partial_rows). */
    float* colstats;
    /* optional (bf16, a_kind = HS_A_RC, no split-K, batch 1): rowsum_a[m] = sum over k of A[k][m] in f32 -- with A = dY this
       is the bias gradient of the Linear whose weight gradient the GEMM computes, so db costs one extra MFMA per A
       fragment in the first tile column instead of a column-sum pass over dY.  With seg_rows the sums of segment i go to
       rowsum_seg[i-1] (row index rebased), like D_seg. */
    float* rowsum_a;
    float* rowsum_seg[2];
    /* optional (bf16 result, batch 1, plain epilogue: no bias / activation / residual / multiplier, alpha = 1; data-gradient
       layouts): the GEMM result is the gradient of relu(BatchNorm(c)) -- the epilogue also produces that BatchNorm's backward
       sums per (row tile, channel): bnb_partials[(tile_row * N + n) * 2 + {0, 1}] = sum over the tile's rows of dz and dz * xhat,
       dz = D * (fma(c, scale, shift) > 0), xhat = (c - mean) * invstd; hs_gemm_tile_rows(p) gives the number of tile rows.
       hs_bn_bwd_params.partial_rows then skips BatchNorm's own partial-sum pass (reference: the same sums torch's
       batch_norm_backward takes in its own kernel). */
    const void* bnb_x;          /* c: [M][N], leading dimension ldd, operand dtype */
    const float* bnb_scale;
    const float* bnb_shift;
    const float* bnb_mean;
    const float* bnb_invstd;
    float* bnb_partials;
    /* optional (with colstats, when hs_gemm_bn_finish_rows(p) > 0): the launch also FINISHES the statistics of the BatchNorm
       that follows -- the last workgroup of each column tile merges the tile rows' partials and writes bn_finish->save_mean /
       save_invstd / scale / shift and updates running_mean / running_var (train-mode arithmetic of hs_batchnorm_fwd: biased
       variance for normalisation, unbiased for running_var).  colstats must then hold hs_gemm_bn_finish_rows(p) rows.  The
       caller runs hs_batchnorm_fwd with stats_done = 1 (apply pass only): one launch per BatchNorm less on the stream. */
    const struct hs_bn_params* bn_finish;
    /* optional (with bnb_partials): the result is the gradient of relu(BatchNorm(c) + identity) -- a residual block's OUTPUT --
       so the ReLU mask is read from the saved output bnb_y ([M][N], leading dimension ldd: mask = y > 0) instead of being
       recomputed from c, and the launch may carry `residual` (the identity path's gradient, added BEFORE the sums are taken:
       reference torchvision Bottleneck.forward `out += identity; out = relu(out)`).  bnb_scale / bnb_shift are then unused. */
    const void* bnb_y;
    /* optional (with bnb_partials, when hs_gemm_bnb_finish_rows(p) > 0): the launch also FINISHES that BatchNorm's backward sums --
       the last workgroup of each column tile adds the tile rows' partials and writes bnb_finish->dbeta / dgamma and, behind
       the hs_gemm_bnb_finish_rows(p) rows of bnb_partials, the four per-channel coefficient vectors of the apply pass
       (gamma, M, training are read from *bnb_finish).  The caller then runs hs_batchnorm_bwd with ws = bnb_partials,
       partial_rows = hs_gemm_bnb_finish_rows(p) and sums_done = 1 (apply pass only): one launch per BatchNorm less on the
       stream (reference: torch's batch_norm_backward reduce + elementwise kernels). */
    const struct hs_bn_bwd_params* bnb_finish;
    /* optional (plain bf16 GEMMs, batch 1): row counts that live in DEVICE memory -- the BERT tower on its valid tokens only
       (hs_bert_desc.pack_rows).  The host never reads them: the grid, the tile shape and every buffer stay those of the padded
       M / K, and the kernels clamp what they read.  NULL = off.
         m_rows    the tokens are the rows of D: only rows < *m_rows are needed; tiles that start at or behind it are skipped
                   (the tile that holds row *m_rows is computed whole; rows >= *m_rows of D are then unspecified)
         drop_rows [M] int32: the dropout draw of output row m is the one of row drop_rows[m] (the padded position of a packed
                   row), so a packed and a padded run apply the same mask */
    const int32_t* m_rows;
    const int32_t* drop_rows;
} hs_gemm_params;

hs_status hs_gemm(const hs_gemm_params* p, void* stream);
/* workspace (bytes) hs_gemm needs in p->splitk_ws for the given p (0 when split_k <= 1). */
int64_t hs_gemm_splitk_ws_bytes(const hs_gemm_params* p);
/* number of row tiles hs_gemm will use for p (rows of a colstats buffer); 0 when p cannot produce colstats. */
int32_t hs_gemm_stat_rows(const hs_gemm_params* p);
/* rows the colstats buffer needs when the launch for p (colstats set) can also finish the BatchNorm statistics
   (hs_gemm_params.bn_finish): tile rows + merge rows; 0 when this launch cannot. */
int32_t hs_gemm_bn_finish_rows(const hs_gemm_params* p);
/* rows bnb_partials must hold (tile rows + merge rows) when the launch for p can also finish the BatchNorm-backward sums
   (hs_gemm_params.bnb_finish), else 0 (split-K launches, layouts without the rider). */
int32_t hs_gemm_bnb_finish_rows(const hs_gemm_params* p);
/* tile rows of the launch hs_gemm makes for p (p->split_k as it will be launched): rows of bnb_partials */
int32_t hs_gemm_tile_rows(const hs_gemm_params* p);
/* heuristic split-K factor for a (M,N,K) problem so that the grid fills 256 CUs. */
int32_t hs_gemm_suggest_split(int32_t M, int32_t N, int32_t K, int32_t dtype);
/* Optional timing of every GEMM-core launch with HIP events on its stream (measurement only).
   Classes: 0 bf16 GEMM, 1 bf16 implicit-GEMM conv, 2 f32 GEMM, 3 f32 conv.  hs_prof_collect synchronises the
   device, fills 4 entries of algorithmic flops / elapsed ms / launch counts and clears the records. */
/* measurement only: force a tile configuration (0 128x128, 1 128x64, 2 64x64, -1 auto) and ablation bits
   (16 = plain n-fastest tile order instead of the L2-grouped one; 32 = always the generic epilogue body instead of
   the specialised ones; results stay correct).  cfg also accepts 4 (256x128, 8 waves), 5 (128x128, BK 32), 6 (256x128, BK 32)
   for plain bf16 GEMMs. */
void hs_gemm_debug(int32_t cfg_override, int32_t ablate);
/* measurement only: while device_buffer is not NULL every bf16 hs_gemm launch writes 6 shader-clock stamps per workgroup
   (start, first DMA issued, first K tile landed, K loop done, epilogue done, unused) to it; size it 48 bytes x workgroups. */
void hs_gemm_debug_stamps(void* device_buffer);
void hs_prof_enable(int32_t on);
hs_status hs_prof_collect(double* flops, double* ms, int64_t* launches);
/* measurement only: append one CSV line per recorded launch (class, operand combo, tile cfg, M, N, K, batch, split_k,
   filter R, stride, milliseconds) to `path` and clear the records. */
hs_status hs_prof_dump(const char* path);
/* measurement only: mean elapsed time (us) of `n` empty kernels inside the profiler's event bracket, i.e. what the
   bracket adds to every timed launch. */
hs_status hs_prof_calibrate(void* stream, int32_t n, float* avg_us);

/* ------------------------------------------------------------------------------------------- */
/* BatchNorm2d over NHWC activations viewed as [M = N*H*W][C]                                    */
/* Replaces torch.nn.BatchNorm2d inside torchvision ResNet blocks (reference encoder.py:35-42,  */
/* mibf_net/model_resnet.py:15): train mode = batch statistics (biased var for normalisation,   */
/* unbiased for running_var, momentum 0.1), eval mode = running statistics.                     */
/* ------------------------------------------------------------------------------------------- */
typedef struct hs_bn_params {
    int32_t dtype;
    int32_t C;
    int64_t M;
    int32_t training;        /* 1: batch stats (+ running update), 0: running stats              */
    int32_t relu;            /* fuse ReLU into the apply pass                                    */
    float eps, momentum;
    const void* x;           /* [M][C]                                                           */
    const void* residual;    /* optional [M][C], added before the ReLU                           */
    void* y;                 /* [M][C] (NULL: statistics only)                                   */
    const float* gamma;
    const float* beta;
    float* running_mean;     /* may be NULL in training (no update)                              */
    float* running_var;
    float* save_mean;        /* [C] out                                                          */
    float* save_invstd;      /* [C] out                                                          */
    float* scale;            /* [C] out: gamma*invstd                                            */
    float* shift;            /* [C] out: beta - mean*gamma*invstd                                */
    void* ws;                /* hs_batchnorm_ws_bytes(M, C, dtype)                               */
    int64_t ws_bytes;
    int32_t partial_rows;    /* > 0: ws already holds that many rows of (count, mean, M2) partials per channel
                                (hs_gemm colstats): skip the statistics pass over x                */
    int32_t stats_done;      /* 1: save_mean / save_invstd / scale / shift (and the running statistics) are already
                                written (hs_gemm_params.bn_finish): apply pass only                 */
} hs_bn_params;

typedef struct hs_bn_bwd_params {
    int32_t dtype;
    int32_t C;
    int64_t M;
    int32_t training;
    int32_t relu;            /* forward fused a ReLU: dz = dy * (y > 0)                          */
    const void* dy;
    const void* y;           /* forward output (needed when relu, unless scale / shift are given) */
    const void* x;           /* forward input                                                    */
    const float* gamma;
    const float* save_mean;
    const float* save_invstd;
    void* dx;                /* [M][C] (NULL: parameter gradients only)                          */
    void* dres;              /* optional: gradient of the residual input (= dz)                  */
    float* dgamma;
    float* dbeta;
    void* ws;
    int64_t ws_bytes;
    /* optional, relu without a residual input: with y == NULL the ReLU mask is recomputed as fma(x, scale, shift) > 0 from the
       forward's scale / shift (hs_bn_params.scale / .shift of the same layer): one activation read less in both passes */
    const float* scale;
    const float* shift;
    /* > 0: ws already holds [partial_rows][C][2] backward sums (hs_gemm_params.bnb_partials): no partial pass is made */
    int32_t partial_rows;
    /* 1 (with partial_rows > 0): the producing GEMM also finished the sums (hs_gemm_params.bnb_finish): dgamma / dbeta are
       written and the coefficients sit behind the partial rows -- only the apply pass runs */
    int32_t sums_done;
} hs_bn_bwd_params;

/* Preconditions of both calls: C % 8 == 0 (bf16) / C % 4 == 0 (f32), refused otherwise; every per-channel vector
   (gamma, beta, running_*, save_*, scale, shift, dgamma, dbeta) is its own 16-byte aligned array -- the apply passes
   read scale / shift as 16-byte vectors.  A workspace smaller than hs_batchnorm_ws_bytes is refused. */
hs_status hs_batchnorm_fwd(const hs_bn_params* p, void* stream);
hs_status hs_batchnorm_bwd(const hs_bn_bwd_params* p, void* stream);
int64_t hs_batchnorm_ws_bytes(int64_t M, int32_t C, int32_t dtype);

/* LayerNorm over the last dim of [M][H]. Replaces torch.nn.LayerNorm (reference                */
/* modules/fusion_blocks.py:17-34, modules/heads.py:36; transformers Bert*Output.LayerNorm).    */
/* Preconditions: H % 8 == 0 and H <= 2048 (bf16) / H % 4 == 0 and H <= 1024 (f32), refused otherwise; M >= 1 (not
   checked); gamma, beta, dgamma, dbeta, dbias are 16-byte aligned arrays of H floats; mean / rstd (forward) and dx
   (backward) may be NULL; the backward's workspace holds hs_layernorm_bwd_ws_bytes(M, H) bytes. */
hs_status hs_layernorm_fwd(int32_t dtype, const void* x, const float* gamma, const float* beta, void* y,
                           float* mean, float* rstd, int64_t M, int32_t H, float eps, void* stream);
hs_status hs_layernorm_bwd(int32_t dtype, const void* dy, const void* x, const float* gamma, const float* mean,
                           const float* rstd, void* dx, float* dgamma, float* dbeta, void* ws, int64_t ws_bytes,
                           int64_t M, int32_t H, void* stream);
/* the same, also serving the layer in front of the LayerNorm (BertSelfOutput / BertOutput: y = LN(dropout(dense(h)) + x)):
   dx_dropped = dx * dropout mask (same (seed, element index) mask as the forward, the element index of dx[row][col] being
   row * H + col, i.e. hs_dropout over the [M][H] tensor; 0 <= p < 1; p = 0: a copy; may be NULL) and
   dbias[H] = column sums of dx_dropped = that dense layer's bias gradient.  Saves the stand-alone dropout and column-sum
   passes of transformers BertSelfOutput / BertOutput backward. */
hs_status hs_layernorm_bwd_pre(int32_t dtype, const void* dy, const void* x, const float* gamma, const float* mean,
                               const float* rstd, void* dx, float* dgamma, float* dbeta, void* dx_dropped, float* dbias,
                               float dropout_p, uint64_t seed, void* ws, int64_t ws_bytes, int64_t M, int32_t H, void* stream);
int64_t hs_layernorm_bwd_ws_bytes(int64_t M, int32_t H);

/* ------------------------------------------------------------------------------------------- */
/* pooling, packing, casts, reductions, softmax, embeddings, loss, optimizer (HBM-bound helpers) */
/* ------------------------------------------------------------------------------------------- */
#define HS_CAST_MAX 48
#define HS_ADAM_MAX 32

/* MaxPool2d(k, s, p) on NHWC; idx (uint8, same shape as y) keeps the arg-max tap r * k + s for the backward: the first
   maximum in (r, s) scan order, taps in the padding never win (they count as -inf).  The backward is a gather.
   Replaces torchvision ResNet.maxpool (reference encoder.py:67).
   Preconditions, refused before any arithmetic or launch: C % 4 == 0 (f32) / C % 8 == 0 (bf16) and ksize <= 15 (HS_ERR_ARG);
   N, H, W, C >= 1, ksize >= 1, stride >= 1, pad >= 0, H + 2 pad >= ksize and W + 2 pad >= ksize, so that P, Q >= 1
   (HS_ERR_UNSUPPORTED).  pad <= ksize / 2
   as torch demands is not checked: a window that lies in the padding altogether yields -inf and tap 0. */
hs_status hs_maxpool_fwd(int32_t dtype, const void* x, void* y, void* idx, int32_t N, int32_t H, int32_t W, int32_t C,
                         int32_t ksize, int32_t stride, int32_t pad, void* stream);
hs_status hs_maxpool_bwd(int32_t dtype, const void* dy, const void* idx, void* dx, int32_t N, int32_t H, int32_t W,
                         int32_t C, int32_t ksize, int32_t stride, int32_t pad, void* stream);
/* y[b][:] = mean_t x[b][t][:]  (AdaptiveAvgPool / tokens.mean(dim=1); reference
   modules/fusion_blocks.py:97-98,170-178, model.py:283-290, torchvision ResNet.avgpool).  The sum is multiplied by
   float(1 / Nt); the backward is dx[b][t][:] = dy[b][:] * float(1 / Nt), rounded once.  B, Nt >= 1 and H % 4 == 0 (f32) /
   H % 8 == 0 (bf16), refused otherwise.  out_f32 / dy_f32: y / dy is float32 whatever dtype says. */
hs_status hs_mean_tokens_fwd(int32_t dtype, const void* x, void* y, int32_t B, int32_t Nt, int32_t H, int32_t out_f32,
                             void* stream);
hs_status hs_mean_tokens_bwd(int32_t dtype, const void* dy, void* dx, int32_t B, int32_t Nt, int32_t H, int32_t dy_f32,
                             void* stream);
/* f32 NCHW image -> zero-bordered NHWC4 image of type dtype: [N][Hp][Wp][4], pixel (h,w) at (h+pad, w+pad). */
hs_status hs_pack_image(int32_t dtype, const float* x, void* y, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Hp,
                        int32_t Wp, int32_t pad, void* stream);
/* stem filter [K][R][S][Cin] f32 (channels_last storage of (K,Cin,R,S)) <-> packed [K][R][8][4]. */
hs_status hs_pack_stem_weight(int32_t dtype, const float* w, void* out, int32_t K, int32_t R, int32_t S, int32_t Cin,
                              void* stream);
hs_status hs_unpack_stem_wgrad(const float* g, float* dw, int32_t K, int32_t R, int32_t S, int32_t Cin, void* stream);
/* one launch per HS_CAST_MAX tensors: dst[i] (bf16) = src[i] (f32). */
hs_status hs_cast_f32_to_bf16_multi(int32_t count, const float* const* src, void* const* dst, const int64_t* n,
                                    void* stream);
/* dst[c][r] = src[r][c] for a bf16 matrix of R rows x C columns (leading dimensions in elements; R, C, ld % 8 == 0).
   Used by the BertLayer backward to turn its weight gradients (dY^T X, reduction over the row index of both operands)
   into K-contiguous GEMMs; replaces nothing in the reference (torch.nn.Linear's backward is one cuBLAS call there). */
hs_status hs_transpose_bf16(const void* src, void* dst, int32_t R, int32_t C, int64_t ld_src, int64_t ld_dst, void* stream);
/* the same for up to HS_TRANSPOSE_MAX matrices per launch (entries beyond that go to further launches) */
#define HS_TRANSPOSE_MAX 8
hs_status hs_transpose_bf16_multi(int32_t count, const void* const* src, void* const* dst, const int32_t* R, const int32_t* C,
                                  const int64_t* ld_src, const int64_t* ld_dst, void* stream);
/* The row map of the text tower on packed rows (hs_bert_desc.pack_rows), made on the device from attention_mask [B][L]
   (non-zero = valid) and never read by the host.  int32 words: map[0] = T valid tokens, map[1] = kc_n, map[2] = 32 * kc_n,
   map[3] = 0; cu = map + 4: [B + 1] first packed row of each sequence; row_of = cu + roundup(B + 1, 4): [B*L] padded position of
   a packed row; packed_of = row_of + B*L: [B*L] packed row of a padded position or -1; kc_pos = packed_of + B*L:
   [ceil(B*L / 32)], of which the first kc_n are set: the 32-position chunks of [0, B*L) that hold a valid token, ascending. */
int64_t hs_bert_row_map_bytes(int32_t B, int32_t L);
hs_status hs_bert_row_map(const int64_t* mask, int32_t B, int32_t L, int32_t* map, void* stream);
/* dst [C][ld_dst] = transpose of PACKED token rows src [..][ld_src] (bf16; R = B*L, R, C, ld % 8 == 0): column r is the token at
   padded position r, read from source row packed_of[r], zeros where that is -1.  With kc_n / kc_pos (both or neither; device
   pointers into a row map) the columns are chunk-compacted: column c < 32 * *kc_n is padded position kc_pos[c / 32] * 32 + c % 32,
   columns from there to max(64, roundup(32 * *kc_n, 64)) are zeros and nothing behind that is written.  The form the tower's
   weight gradients read; exported for tests. */
hs_status hs_transpose_bf16_tokens(const void* src, void* dst, int32_t R, int32_t C, int64_t ld_src, int64_t ld_dst,
                                   const int32_t* packed_of, const int32_t* kc_n, const int32_t* kc_pos, void* stream);
/* out = a*x + b*y (y may be NULL); dtypes are HS_F32/HS_BF16 for inputs (shared) and output. */
hs_status hs_axpby(int32_t in_dtype, int32_t out_dtype, const void* x, const void* y, void* out, int64_t n, float a,
                   float b, void* stream);
/* out[i] = x[i] * keep(seed, i) / (1-p): the same call is its own backward. */
hs_status hs_dropout(int32_t dtype, const void* x, void* out, int64_t n, float p, uint64_t seed, void* stream);
/* out = max(x, 0) by fmaxf: relu(NaN) = 0 (torch returns NaN), relu(-0.0) = +0.0; dx = y > 0 ? dy : 0. */
hs_status hs_relu_fwd(int32_t dtype, const void* x, void* out, int64_t n, void* stream);
hs_status hs_relu_bwd(int32_t dtype, const void* dy, const void* y, void* dx, int64_t n, void* stream);
/* dx = dy * gelu'(u)  (erf GELU). */
hs_status hs_gelu_bwd(int32_t dtype, const void* dy, const void* u, void* dx, int64_t n, void* stream);
/* out = x * scalar[0] with the scalar on the device (loss backward without a host sync). */
hs_status hs_mul_dev_scalar(const float* x, const float* scalar, float* out, int64_t n, void* stream);
/* out[n] (+)= sum_m x[m*ld + n]  (bias gradients).  M, N >= 1 (refused otherwise), ld >= N (not checked); ws holds
   hs_colsum_ws_bytes(M, N) bytes; out[N..] is never written. */
hs_status hs_colsum(int32_t dtype, const void* x, int64_t M, int32_t N, int32_t ld, float* out, void* ws,
                    int64_t ws_bytes, int32_t accumulate, void* stream);
int64_t hs_colsum_ws_bytes(int64_t M, int32_t N);
/* attention probabilities from materialised f32 scores; rows = (b,h,q); mask[b][k] == 0 masks key k.
   P gets the probabilities (padding columns Lk..ldP-1 zeroed), P_drop (optional) the dropped-out copy.
   Preconditions: 1 <= Lk <= ldP <= 1024 (Lk, ldP > 1024 and rows < 1 are refused; ldP >= Lk and ldS, ldG >= Lk are not
   checked).  The dropout element index of P[r][k] is r * Lk + k (not r * ldP + k): the mask of hs_dropout over a dense
   [rows][Lk] tensor, in the forward and the backward alike.  A row whose keys are all masked gets the uniform 1 / Lk. */
hs_status hs_softmax_fwd(int32_t dtype, const float* S, const int64_t* mask, void* P, void* P_drop, int64_t rows,
                         int32_t Lk, int32_t ldS, int32_t ldP, int32_t rows_per_batch, float dropout_p, uint64_t seed,
                         void* stream);
hs_status hs_softmax_bwd(int32_t dtype, const float* dP, const void* P, void* dS, int64_t rows, int32_t Lk, int32_t ldG,
                         int32_t ldP, float dropout_p, uint64_t seed, void* stream);
/* BertEmbeddings (token_type_ids == 0): sum_out = word[ids]+pos[l]+type0 ; y = dropout(LN(sum_out)).
   Token t of `tokens` sits at position l = t % L; sum_out is rounded to dtype first and the LayerNorm reads the rounded value;
   the dropout element index of y[t][h] is t * H + h (the mask of hs_dropout over the [tokens][H] tensor).
   An id outside [0, V) is clamped to 0 or V - 1, not refused (nn.Embedding raises there): intended, it keeps a bad id from
   reading outside the table, and hs_bert_embed_bwd clamps alike.
   Preconditions, refused before any launch: no NULL pointer; 4 <= H <= 1024, H % 4 == 0 (HS_ERR_ARG); tokens, L, V >= 1
   (HS_ERR_UNSUPPORTED). */
hs_status hs_bert_embed_fwd(int32_t dtype, const int64_t* ids, const float* word, const float* pos, const float* type0,
                            const float* gamma, const float* beta, void* sum_out, void* y, float* mean, float* rstd,
                            int64_t tokens, int32_t L, int32_t H, int32_t V, float eps, float dropout_p, uint64_t seed,
                            void* stream);
/* dword (zero-filled by the caller) += scatter(dsum by ids), skipping ids == pad_id (nn.Embedding
   padding_idx; -1 = none); dpos[l] = sum_b dsum[b][l].  dword or dpos may be NULL.  Up to 15360 tokens a table row is the
   sum of its tokens' rows in token order (the same bits on every run); beyond that float atomics add them in any order.
   Rows of ids that do not occur keep the caller's zeros.  ids are clamped as in the forward.
   Preconditions, refused before any launch: ids, dsum not NULL (HS_ERR_ARG); B, L, H, V >= 1 (HS_ERR_UNSUPPORTED). */
hs_status hs_bert_embed_bwd(int32_t dtype, const int64_t* ids, const void* dsum, float* dword, float* dpos, int32_t B,
                            int32_t L, int32_t H, int32_t V, int32_t pad_id, void* stream);
/* mean-reduced CrossEntropyLoss(weight, label_smoothing): writes the scalar loss, d loss / d logits
   (optional) and the per-row unreduced losses (optional). reference scripts/train.py:240,252-254.
   Precondition, here and in hs_mp_loss / hs_focal_loss: every label lies in [0, C).  Labels are not checked (there is no
   ignore_index); one outside the range reads logits and weight out of bounds. */
hs_status hs_cross_entropy(const float* logits, const int64_t* labels, const float* weight, float label_smoothing,
                           int32_t B, int32_t C, float* loss, float* dlogits, float* row_loss, void* stream);
/* fused multi-tensor Adam (decoupled=0) / AdamW (decoupled=1) step over f32 tensors. */
hs_status hs_adam_step_multi(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                             float* const* exp_avg_sq, const int64_t* n, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int32_t step, int32_t decoupled, float grad_scale, void* stream);
/* the same, additionally writing bf16 copies of the updated parameters (bf16_shadow[i] may be NULL; the whole array may be
   NULL): the copies the composites read as weights once registered with hs_weight_shadow_set */
hs_status hs_adam_step_multi_shadow(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                                    float* const* exp_avg_sq, void* const* bf16_shadow, const int64_t* n, float lr, float beta1,
                                    float beta2, float eps, float weight_decay, int32_t step, int32_t decoupled,
                                    float grad_scale, void* stream);
/* Caller-scoped grouping of weight-gradient GEMMs: between _begin and _end, the K-contiguous ("nt") weight-gradient GEMMs
   that hs_linear_bwd issues on `stream` are collected and then launched as ONE grid (an MLP's two Linear layers fill the chip
   together where each alone does not).  The workspaces passed to the collected hs_linear_bwd calls must stay alive and must
   not overlap until _end returns.  No reference counterpart (cuBLAS launches every GEMM on its own). */
hs_status hs_wgrad_group_begin(void* stream);
hs_status hs_wgrad_group_end(void* stream);
/* Deferred weight-gradient set.  While a set is open on `stream`, hs_linear_bwd launches only its data-gradient GEMM there and
   hands the row-major ("tn") weight gradient and the bias gradient to the set, copied by value (x, dy, leading dimensions, M,
   in_f, out_f, dtype, dw, db).  _flush launches them: the bf16 weight gradients as ONE grouped grid (per problem the tile, the
   split of hs_gemm_suggest_split and the reduction order of its own launch: the same bits), f32 ones one by one, and all bias
   gradients as ONE column-sum partial launch and ONE final launch (per problem the chunking and order of hs_colsum), then
   closes the set.  The caller keeps every x, dy, dw, db alive and unchanged until _flush has returned; ws holds
   hs_wgrad_defer_ws_bytes(stream) bytes (asked right before the flush).  A set holds up to 64 problems; a full set, the
   K-contiguous form (with its hs_wgrad_group_* scope) and the HAMSPINE_OVERLAP=1 mode take the immediate path.  _begin on an
   open set keeps it; _suspend leaves the set open but sends hs_linear_bwd down the immediate path until the next _begin (a
   caller brackets the calls whose operands it keeps alive with _begin / _suspend, so that other callers on the stream never feed
   the set); _abort drops a set without launching; _open / _pending: 1 / the number of problems held, 0 with no set.
   _counters: out[5] = problems deferred, problems flushed, grouped launches, column-sum launches, table uploads (process
   totals).  No reference counterpart (autograd runs every gradient where its node is). */
hs_status hs_wgrad_defer_begin(void* stream);
hs_status hs_wgrad_defer_suspend(void* stream);
int32_t hs_wgrad_defer_open(void* stream);
int32_t hs_wgrad_defer_pending(void* stream);
int64_t hs_wgrad_defer_ws_bytes(void* stream);
hs_status hs_wgrad_defer_flush(void* stream, void* ws, int64_t ws_bytes);
hs_status hs_wgrad_defer_abort(void* stream);
void hs_wgrad_defer_counters(int64_t* out);
/* bf16 shadow registry: while registered, every composite / tower reads `bf16` (n elements of the weight, same memory order)
   instead of casting `w` in its forward.  The caller keeps it equal to bf16(w).  bf16 = NULL forgets the entry.  No
   reference counterpart (torch autocast re-casts weights per call). */
hs_status hs_weight_shadow_set(const float* w, void* bf16);
void hs_weight_shadow_clear(void);

/* fused multi-tensor SGD, torch.optim.SGD semantics (the reference's fallback optimizer, scripts/train.py:309):
   g += wd*p; buf = first ? g : momentum*buf + g; g = nesterov ? g + momentum*buf : buf; p -= lr*g.  momentum_buf may be
   NULL when momentum == 0. */
hs_status hs_sgd_step_multi(int32_t count, float* const* params, const float* const* grads, float* const* momentum_buf,
                            const int64_t* n, float lr, float momentum, float weight_decay, int32_t nesterov, int32_t first,
                            float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------- */
/* Global gradient-norm clipping without a host sync (csrc/gradclip.hip).  Replaces               */
/* torch.nn.utils.clip_grad_norm_; no reference counterpart (the reference trains without it).    */
/* The norm and its clip coefficient stay on the device in a four-float record                    */
/*   rec[0] = the global 2-norm, rounded once to f32                                              */
/*   rec[1] = the coefficient fminf(max_norm / (rec[0] + 1e-6f), 1.0f) in f32, a NaN kept          */
/*   rec[2] = 1 if rec[0] is finite, else 0                                                       */
/*   rec[3] = 1 if the step is to be skipped (skip_nonfinite set and rec[2] == 0), else 0          */
/* that the step kernels below read.  Nothing here reads the device back.                         */
/* ------------------------------------------------------------------------------------------- */
#define HS_GRADCLIP_MAX 128
/* Sums of squares of `count` <= HS_GRADCLIP_MAX f32 tensors (n[i] >= 0 elements; grads[i] 4-byte aligned, any n[i] including
   0), in f64.  Every workgroup writes the sum over its fixed share of one tensor into its own slot: the call fills
   hs_grad_norm_partials(count, n) slots of `partials`, in tensor order, and further calls are laid end to end behind them.
   No atomics; the slot and the order of every sum depend on (count, n) alone, so a rerun repeats bitwise.
   Replaces the norm pass of torch.nn.utils.clip_grad_norm_; no reference counterpart.
   Refused before any launch (HS_ERR_ARG): count outside [0, HS_GRADCLIP_MAX], a NULL table, a NULL or misaligned entry,
   n[i] < 0, partials NULL. */
hs_status hs_grad_sumsq_multi(int32_t count, const float* const* grads, const int64_t* n, double* partials, void* stream);
/* slots the call above writes; -1 for arguments it refuses.  No reference counterpart. */
int64_t hs_grad_norm_partials(int32_t count, const int64_t* n);
/* One workgroup adds `n_partials` slots in a fixed order in f64 and writes rec[0..3] as stated above.  With
   skip_nonfinite == 0 a non-finite norm follows the arithmetic as torch does: a NaN norm gives a NaN coefficient, an infinite
   one the coefficient 0.  max_norm = +inf: coefficient 1 (monitor only).
   Replaces the norm reduction and clip_coef arithmetic of torch.nn.utils.clip_grad_norm_; no reference counterpart.
   Refused before any launch: partials or rec NULL, max_norm negative or NaN (HS_ERR_ARG); n_partials < 1
   (HS_ERR_UNSUPPORTED). */
hs_status hs_grad_norm_finish(const double* partials, int64_t n_partials, float max_norm, int32_t skip_nonfinite, float* rec,
                              void* stream);
/* g *= rec[1] in place over `count` <= HS_GRADCLIP_MAX tensors; every thread leaves at once (no write traffic) when
   rec[1] == 1.0f or rec[3] is set.  The stand-alone route for optimizers without a fused one.
   Replaces the scaling pass of torch.nn.utils.clip_grad_norm_; no reference counterpart.  Refusals as hs_grad_sumsq_multi,
   and rec NULL. */
hs_status hs_grad_scale_multi(int32_t count, float* const* grads, const int64_t* n, const float* rec, void* stream);
/* hs_adam_step_multi_shadow with the gradient multiplied by grad_scale, then by rec[1]; with rec[3] set the launch leaves
   p, exp_avg, exp_avg_sq and the bf16 shadow untouched.  With rec[1] == 1 the results are bitwise those of
   hs_adam_step_multi_shadow.  Replaces torch.nn.utils.clip_grad_norm_ in front of torch.optim.Adam/AdamW.step; no reference
   counterpart.  Refused (HS_ERR_ARG): count < 0, step < 1, rec NULL, a NULL table other than bf16_shadow. */
hs_status hs_adam_step_multi_clip(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                                  float* const* exp_avg_sq, void* const* bf16_shadow, const int64_t* n, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, int32_t step, int32_t decoupled, float grad_scale,
                                  const float* rec, void* stream);
/* hs_sgd_step_multi likewise: the gradient times grad_scale, then rec[1]; with rec[3] set p and the momentum buffer stay as
   they are.  Replaces torch.nn.utils.clip_grad_norm_ in front of torch.optim.SGD.step; no reference counterpart.
   Refused (HS_ERR_ARG): count < 0, momentum without buffers, rec NULL, a NULL table. */
hs_status hs_sgd_step_multi_clip(int32_t count, float* const* params, const float* const* grads, float* const* momentum_buf,
                                 const int64_t* n, float lr, float momentum, float weight_decay, int32_t nesterov, int32_t first,
                                 float grad_scale, const float* rec, void* stream);

/* ------------------------------------------------------------------------------------------- */
/* Muon (csrc/muon.hip): the Muon group of MuonWithAuxAdam, reference scripts/train.py:262-307     */
/* (`from muon import MuonWithAuxAdam`).  A parameter is the matrix (rows = shape[0], cols = numel  */
/* / rows) its dense f32 memory holds.  The matrices of one (rows, cols) group are packed into one  */
/* compute-dtype buffer [count][rows8][cols8], both extents rounded up to a multiple of 8 with zero */
/* fill, so that every Newton-Schulz product is one batched hs_gemm.  Momentum, norms and the        */
/* parameter update are f32; every sum is taken in a fixed order (results repeat bitwise).          */
/* ------------------------------------------------------------------------------------------- */
#define HS_MUON_MAX 32
#define HS_MUON_PARTIALS 256
/* Pre-pass over `count` tensors (reference scripts/train.py:262-307, the momentum / Nesterov / normalise steps of
   muon_update): m <- m + (1 - beta)(g - m) in place, u = g + beta (m - g), packed[i] = u / (||u||_F + 1e-7) as a
   [rows8][cols8] matrix of `dtype` with zero fill.  partials: f32 [count][HS_MUON_PARTIALS], the per-workgroup sums of
   squares, added in index order. */
hs_status hs_muon_prepare_multi(int32_t dtype, int32_t count, float* const* momentum, const float* const* grads,
                                void* const* packed, const int32_t* rows, const int32_t* cols, float beta, float* partials,
                                void* stream);
/* Five Newton-Schulz iterations X <- a X + (b A + c A A) X, A = X X^T (for rows > cols: on the transpose, read in place),
   (a, b, c) = (3.4445, -4.7750, 2.0315), on `count` packed matrices X [count][rows8][cols8] of `dtype`, in place (reference
   scripts/train.py:262-307: zeropower_via_newtonschulz5 of the muon package).  Every product is an hs_gemm launch (batched
   over the group; split-K for a single matrix): S = b X X^T, B = S + (c / b^2) S S, B += a I, X' = B X.
   ws: hs_muon_ws_bytes(dtype, count, rows, cols). */
hs_status hs_muon_orthogonalize(int32_t dtype, int32_t count, int32_t rows, int32_t cols, void* X, void* ws, int64_t ws_bytes,
                                void* stream);
/* workspace of hs_muon_orthogonalize (reference scripts/train.py:262-307): S and B [count][n8][n8], n8 = min(rows8, cols8),
   a second X and, for count == 1, the split-K slabs; -1 for bad arguments. */
int64_t hs_muon_ws_bytes(int32_t dtype, int32_t count, int32_t rows, int32_t cols);
/* Apply pass over `count` tensors (reference scripts/train.py:262-307, the update of the Muon group):
   p <- p (1 - lr weight_decay) - lr scale[i] O, O read from packed[i] ([rows8][cols8] of `dtype`, the pad skipped), and
   bf16_shadow[i] <- bf16(p) where given (the array or an entry may be NULL), as hs_adam_step_multi_shadow does. */
hs_status hs_muon_apply_multi(int32_t dtype, int32_t count, float* const* params, void* const* bf16_shadow,
                              const void* const* packed, const int32_t* rows, const int32_t* cols, const float* scale,
                              float lr, float weight_decay, void* stream);

/* ------------------------------------------------------------------------------------------- */
/* small f32 operators at the fusion / head / loss boundary                                       */
/* ------------------------------------------------------------------------------------------- */
/* out[b][:] = x[b][t][:] as f32 (CLS pooling, reference modules/fusion_blocks.py:170-173). */
hs_status hs_select_token_fwd(int32_t dtype, const void* x, float* out, int32_t B, int32_t Nt, int32_t H, int32_t t,
                              void* stream);
hs_status hs_select_token_bwd(int32_t dtype, const float* dy, void* dx, int32_t B, int32_t Nt, int32_t H, int32_t t,
                              void* stream);
/* out[r] = [a[r] | b[r]] and its inverse (torch.cat(dim=1): fusion_blocks.py:186, model_resnet.py:59). */
hs_status hs_concat2(const float* a, int32_t Ha, const float* b, int32_t Hb, float* out, int64_t rows, void* stream);
hs_status hs_split2(const float* g, float* da, int32_t Ha, float* db, int32_t Hb, int64_t rows, void* stream);
/* the same on token tensors of either element type (global/local token concat, reference model.py:311-313). */
hs_status hs_concat2_t(int32_t dtype, const void* a, int32_t Ha, const void* b, int32_t Hb, void* out, int64_t rows,
                       void* stream);
hs_status hs_split2_t(int32_t dtype, const void* g, void* da, int32_t Ha, void* db, int32_t Hb, int64_t rows, void* stream);
/* out = a*b; b_mode 0: same shape, 1: b is (rows,1), 2: b is a scalar. */
hs_status hs_mul(const float* a, const float* b, float* out, int64_t rows, int32_t cols, int32_t b_mode, void* stream);
hs_status hs_rowdot(const float* a, const float* b, float* out, int32_t rows, int32_t cols, void* stream);
/* out[r] = KL(p[r] || q[r]) on probabilities clamped to [eps, 1] (reference mibf_net/attention.py:25-28).  With w (the
   incoming gradient per row) dp / dq receive the gradients; out may then be NULL.  As with torch.clamp, an entry exactly on
   a bound (p == eps, p == 1) passes its gradient; one outside [eps, 1] gets 0. */
hs_status hs_kl_rows(const float* p, const float* q, float* out, const float* w, float* dp, float* dq, int32_t rows,
                     int32_t cols, float eps, void* stream);
/* out[0] = sum a[i]*b[i] (b NULL: sum a). */
hs_status hs_dot(const float* a, const float* b, float* out, int64_t n, void* stream);
hs_status hs_sigmoid_fwd(const float* x, float* out, int64_t n, void* stream);
hs_status hs_sigmoid_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);
/* ent[r] = -sum softmax(z)*log(softmax(z)+1e-8); with g/dlogits set it also writes the backward
   (reference model.py:276-278). */
hs_status hs_softmax_entropy(const float* logits, const float* g, float* ent, float* dlogits, int32_t rows, int32_t C,
                             void* stream);
/* MIBF MP-Loss: 0.3 CE(img) + 0.6 CE(txt) + 1.1 mean(exp(symKL)) CE(fused), loss + three logit gradients
   (reference mibf_net/model_resnet.py:76-94). scratch: B floats. */
hs_status hs_mp_loss(const float* image_logits, const float* text_logits, const float* fused_logits, const int64_t* labels,
                     int32_t B, int32_t C, float* loss, float* d_image, float* d_text, float* d_fused, float* scratch,
                     void* stream);
/* FocalLoss(gamma, weight), mean reduction (reference scripts/train.py:46-61).  gamma = 0 is plain CE with the plain mean
   over the batch.  On a saturated row (ce == 0 in float32: the label class leads by about 17 or more) the gradient is 0 for
   gamma = 0 and for gamma >= 1; for 0 < gamma < 1 it is NaN, as in the reference, whose (1 - pt)^(gamma - 1) is infinite
   there. */
hs_status hs_focal_loss(const float* logits, const int64_t* labels, const float* weight, float gamma, int32_t B, int32_t C,
                        float* loss, float* dlogits, void* stream);
/* out = bilinear_resize(x[:, :, y0:y0+ch, x0:x0+cw], (H, W)), align_corners=False, f32 NCHW
   (reference model.py:292-301). */
hs_status hs_center_crop_resize(const float* x, float* out, int32_t N, int32_t Cc, int32_t H, int32_t W, int32_t y0,
                                int32_t x0, int32_t ch, int32_t cw, void* stream);

/* LSTM / GRU cells of the slice-sequence encoder (reference modules/sequence_blocks.py:22-34,58-62 -> torch.nn.LSTM /
   nn.GRU), f32.  gx = x W_ih^T + b_ih and gh = h W_hh^T + b_hh come from hs_linear_fwd (row pitches ldx / ldh); gate order
   as torch (LSTM i,f,g,o; GRU r,z,n).  `act` [B][4H] keeps the activated gates for the backward. */
hs_status hs_lstm_cell_fwd(const float* gx, int32_t ldx, const float* gh, int32_t ldh, const float* c_prev, float* h, float* c,
                           float* act, int32_t B, int32_t H, void* stream);
/* dgates [B][4H] is the gradient of (gx + gh); dh / dc may be NULL (= zero). */
hs_status hs_lstm_cell_bwd(const float* dh, const float* dc, const float* act, const float* c_prev, const float* c,
                           float* dgates, float* dc_prev, int32_t B, int32_t H, void* stream);
hs_status hs_gru_cell_fwd(const float* gx, int32_t ldx, const float* gh, int32_t ldh, const float* h_prev, float* h,
                          float* act, int32_t B, int32_t H, void* stream);
/* dgx / dgh [B][3H]: gradients of gx and gh; dh_prev: the direct z*dh path only (the W_hh path comes from dgh). */
hs_status hs_gru_cell_bwd(const float* dh, const float* act, const float* h_prev, float* dgx, float* dgh, float* dh_prev,
                          int32_t B, int32_t H, void* stream);

/* ------------------------------------------------------------------------------------------- */
/* Mamba block of the SSM fusion (reference modules/fusion_blocks.py:264-292 -> mamba_ssm.Mamba    */
/* with d_state 16, d_conv 4).  Activations are HS_F32 / HS_BF16 matrices [B*L][d] with explicit   */
/* row pitches (elements; each a multiple of 16 bytes and >= d), so slices of the in_proj / x_proj */
/* outputs are read in place.  Parameters are f32.  State and every sum are f32; all reductions    */
/* run in a fixed order (results repeat bitwise).  Unsupported arguments (N != 16, k != 4,         */
/* misaligned pitches, empty shapes) return HS_ERR_UNSUPPORTED without a launch.                   */
/* ------------------------------------------------------------------------------------------- */
/* y[b][t][c] = silu(bias[c] + sum_j w[c][j] * x[b][t-3+j][c]), x = 0 before t = 0
   (reference modules/fusion_blocks.py:264-292: Mamba.conv1d, depthwise, k = 4, left pad 3). */
hs_status hs_causal_conv1d_fwd(int32_t dtype, const void* x, int32_t ldx, const float* weight, const float* bias, void* y,
                               int32_t ldy, int32_t B, int32_t L, int32_t d, int32_t k, void* stream);
/* dx, dweight [d][4], dbias [d] of the above (reference modules/fusion_blocks.py:264-292); the pre-activation is
   recomputed from x.  ws: hs_causal_conv1d_ws_bytes(B, d) (per-batch partials, summed over b in order). */
hs_status hs_causal_conv1d_bwd(int32_t dtype, const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* weight,
                               const float* bias, void* dx, int32_t lddx, float* dweight, float* dbias, void* ws,
                               int64_t ws_bytes, int32_t B, int32_t L, int32_t d, int32_t k, void* stream);
int64_t hs_causal_conv1d_ws_bytes(int32_t B, int32_t d);
/* Selective scan (reference modules/fusion_blocks.py:264-292: Mamba's selective_scan_fn with delta_softplus, D and z):
     delta = softplus(dt + dt_bias), A = -exp(A_log) [d][16]
     h_t = exp(delta_t A) h_{t-1} + delta_t Bm_t u_t,  y_t = <h_t, Cm_t> + D u_t,  out_t = y_t silu(z_t)
   Bm / Cm: [B*L][16] with the shared pitch ldbc.  hck (NULL in inference): f32 [B][(L-1)/chunk][d][16], the state after every
   full chunk of hs_selective_scan_chunk_len() steps that has a successor, kept for the backward. */
hs_status hs_selective_scan_fwd(int32_t dtype, const void* u, int32_t ldu, const void* dt, int32_t lddt, const float* dt_bias,
                                const float* A_log, const void* Bm, const void* Cm, int32_t ldbc, const float* D, const void* z,
                                int32_t ldz, void* out, int32_t ldo, float* hck, int32_t B, int32_t L, int32_t d, int32_t N,
                                void* stream);
/* Gradients of hs_selective_scan_fwd (reference modules/fusion_blocks.py:264-292): du, ddt (raw dt), dz [B*L][d], dBm / dCm
   [B*L][16] (pitch lddbc, summed over channels), dA_log [d][16], dD [d], ddt_bias [d] (summed over batch and time).  The
   states inside a chunk are recomputed from hck.  ws: hs_selective_scan_ws_bytes(B, L, d). */
hs_status hs_selective_scan_bwd(int32_t dtype, const void* dout, int32_t lddo, const void* u, int32_t ldu, const void* dt,
                                int32_t lddt, const float* dt_bias, const float* A_log, const void* Bm, const void* Cm,
                                int32_t ldbc, const float* D, const void* z, int32_t ldz, const float* hck, void* du, int32_t lddu,
                                void* ddt, int32_t ldddt, void* dBm, void* dCm, int32_t lddbc, void* dz, int32_t lddz,
                                float* dA_log, float* dD, float* ddt_bias, void* ws, int64_t ws_bytes, int32_t B, int32_t L,
                                int32_t d, int32_t N, void* stream);
int64_t hs_selective_scan_ws_bytes(int32_t B, int32_t L, int32_t d);
int32_t hs_selective_scan_chunk_len(void);
/* The scan above for N = d_state in {16, 32, 64, 128, 256} (reference ConNexT/models/block/len4mamba.py:74-79,138-143:
   Mamba(d_state=128)): every [16] above reads [N], hck is [B][(L-1)/chunk][d][N], and for N > 16 A_log, Bm, Cm and hck must
   be 16-byte aligned.  Steps between saved states for this N (16 at N <= 64, 8 at 128, 4 at 256); -1 for any other N. */
int32_t hs_selective_scan_chunk_len_n(int32_t N);
/* Workspace of hs_selective_scan_bwd at d_state N (reference ConNexT/models/block/len4mamba.py:74-79,138-143): per-block
   partials [ceil(d/16)][B*L][2N] and per-batch partials [B][d][N + 2], f32; -1 for an unsupported N. */
int64_t hs_selective_scan_ws_bytes_n(int32_t B, int32_t L, int32_t d, int32_t N);
/* The scan above without the gate, N = 8 (reference ConNexT/models/block/mamba_vision.py:1622-1631: selective_scan_fn with
   z=None, d_state 8 from 1719-1723): hs_selective_scan_fwd / _bwd with N = 8 take z = NULL (and dz = NULL; ldz, lddz are
   ignored), out_t = y_t, and there is no dz.  8 lanes per (batch, channel) pair, 32 channels per block.  N = 8 with a gate,
   and z = NULL at any other N, return HS_ERR_UNSUPPORTED before any launch.  out may be a column slice of a wider buffer
   (pitch ldo).  The gate is a compile-time property of a kernel, so its queries are apart: the two below answer for the
   gate-less instantiations (N = 8: 16 steps between saved states; per-block partials [ceil(d/32)][B*L][16] and per-batch
   partials [B][d][10], f32) and return -1 for any other N, as the _n queries above do for N = 8. */
int32_t hs_selective_scan_chunk_len_nogate(int32_t N);
int64_t hs_selective_scan_ws_bytes_nogate(int32_t B, int32_t L, int32_t d, int32_t N);
/* y[b][t][c] = silu(bias[c] + w[c][0] x[b][t-1][c] + w[c][1] x[b][t][c] + w[c][2] x[b][t+1][c]), x = 0 outside [0, L); bias
   may be NULL (reference ConNexT/models/block/mamba_vision.py:1615-1616: F.silu(F.conv1d(..., padding='same', groups=d)) with
   the bias-less (d, 1, 3) weights of 1588-1603).  x and y carry their own row pitch, so both halves of the in_proj output are
   read in place and y may be a column slice of the buffer out_proj reads (the torch.cat of 1633). */
hs_status hs_conv1d_same_silu_fwd(int32_t dtype, const void* x, int32_t ldx, const float* weight, const float* bias, void* y,
                                  int32_t ldy, int32_t B, int32_t L, int32_t d, int32_t k, void* stream);
/* dx, dweight [d][3] and, when bias is given, dbias [d] of the above (reference ConNexT/models/block/mamba_vision.py:1615-1616);
   bias and dbias are both NULL or both given; the pre-activation is recomputed from x.  ws: hs_conv1d_same_silu_ws_bytes(B, d)
   (per-batch partials, summed over b in order). */
hs_status hs_conv1d_same_silu_bwd(int32_t dtype, const void* dy, int32_t lddy, const void* x, int32_t ldx, const float* weight,
                                  const float* bias, void* dx, int32_t lddx, float* dweight, float* dbias, void* ws,
                                  int64_t ws_bytes, int32_t B, int32_t L, int32_t d, int32_t k, void* stream);
int64_t hs_conv1d_same_silu_ws_bytes(int32_t B, int32_t d);
/* map (B, C, H, W) f32 -> tokens (B nWh nWw, ws ws, C) of `dtype`, nWh = ceil(H / ws), nWw = ceil(W / ws): the zero padding to
   the right and bottom and window_partition of reference ConNexT/models/block/mamba_vision.py:1301-1314,1813-1820, with the
   cast to the compute dtype.  Also the backward of hs_window_reverse. */
hs_status hs_window_partition(int32_t dtype, const float* map, void* tokens, int32_t B, int32_t C, int32_t H, int32_t W, int32_t ws,
                              void* stream);
/* tokens (B nWh nWw, ws ws, C) of `dtype` -> map (B, C, H, W) f32, dropping the tokens of padded positions: window_reverse and
   the crop of reference ConNexT/models/block/mamba_vision.py:1317-1330,1825-1827.  Also the backward of hs_window_partition. */
hs_status hs_window_reverse(int32_t dtype, const void* tokens, float* map, int32_t B, int32_t C, int32_t H, int32_t W, int32_t ws,
                            void* stream);

/* ------------------------------------------------------------------------------------------- */
/* The convolutional half of MambaVision (csrc/mvconv.hip).  Activations are NHWC rows of `dtype` with a channel pitch that
   is a multiple of 8 (ld = ceil8(C)); lanes C .. ld-1 hold zeros and every entry below that writes an activation writes
   them as zeros.                                                                                                       */
/* ------------------------------------------------------------------------------------------- */
/* y[N][P][Q][ldy] = conv3x3(x[N][H][W][ldx], pad 1, stride 1 | 2) [+ bias[Kout]], P = (H - 1) / stride + 1: the nn.Conv2d(.., 3,
   stride, 1) of Downsample, PatchEmbed and ConvBlock (reference ConNexT/models/block/mamba_vision.py:1456,1479,1482,1501,1504)
   as an implicit GEMM on MFMA at channel counts hs_gemm's convolution refuses (any C, Kout with pitches % 8 == 0; bf16 operands
   with f32 accumulation, or f32).  wf: the compute copy [Kout][3][3][ldx] of hs_conv3x3_pack_filter.  No im2col buffer. */
hs_status hs_conv3x3_fwd(int32_t dtype, const void* x, const void* wf, const float* bias, void* y, int32_t N, int32_t H, int32_t W, int32_t C,
                         int32_t ldx, int32_t Kout, int32_t ldy, int32_t stride, void* stream);
/* dx[N][H][W][lddx] of the above from dy[N][P][Q][lddy], for odd and even H, W (the backward of the convolutions of reference
   ConNexT/models/block/mamba_vision.py:1456,1479,1482,1501,1504).  wt: the transposed compute copy [C][3][3][lddy]. */
hs_status hs_conv3x3_dgrad(int32_t dtype, const void* dy, const void* wt, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t lddx,
                           int32_t Kout, int32_t lddy, int32_t stride, void* stream);
/* compute copies of a filter parameter w (Kout, C, 3, 3) f32 (reference ConNexT/models/block/mamba_vision.py:1456,1479-1504 keeps
   nn.Conv2d's layout in the state dict): wf[Kout][3][3][ldc] and, unless NULL, wt[C][3][3][ldk], both of `dtype` with zero pad. */
hs_status hs_conv3x3_pack_filter(int32_t dtype, const float* w, void* wf, void* wt, int32_t Kout, int32_t C, int32_t ldc, int32_t ldk,
                                 void* stream);
/* dw (Kout, C, 3, 3) f32 from the [Kout][3][3][ldc] f32 result of hs_gemm's weight-gradient layout (HS_A_RC x HS_B_CONV over the
   padded input): the weight gradient in the parameter's shape (reference ConNexT/models/block/mamba_vision.py:1456,1479-1504). */
hs_status hs_conv3x3_unpack_wgrad(const float* g, float* dw, int32_t Kout, int32_t C, int32_t ldc, void* stream);
/* image (N, Cin, H, W) f32 -> NHWC rows [N][H][W][ld] of `dtype`, channels Cin .. ld-1 zero: how the image enters PatchEmbed
   (reference ConNexT/models/block/mamba_vision.py:1487-1490 takes it as NCHW). */
hs_status hs_pack_image_nhwc(int32_t dtype, const float* x, void* y, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t ld, void* stream);
/* the backward of hs_pack_image_nhwc: NHWC rows of `dtype` -> (N, Cin, H, W) f32, the input gradient of PatchEmbed (reference
   ConNexT/models/block/mamba_vision.py:1487-1490). */
hs_status hs_unpack_image_nhwc(int32_t dtype, const void* y, float* x, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t ld, void* stream);
/* y = gelu_tanh(fma(x, scale, shift)) over [M][ld] rows: norm1 + act1 of ConvBlock (reference
   ConNexT/models/block/mamba_vision.py:1517-1518); scale / shift from hs_batchnorm_fwd with y = NULL. */
hs_status hs_bn_gelu_tanh_fwd(int32_t dtype, const void* x, const float* scale, const float* shift, void* y, int64_t M, int32_t C, int32_t ld,
                              void* stream);
/* y = res + ls_gamma[c] * rowscale[row / rows_per_sample] * fma(x, scale, shift): norm2, layer scale, stochastic depth and the
   residual of ConvBlock (reference ConNexT/models/block/mamba_vision.py:1520-1523).  ls_gamma NULL: no layer scale; rowscale
   NULL: no stochastic depth. */
hs_status hs_bn_scale_residual_fwd(int32_t dtype, const void* x, const float* scale, const float* shift, const void* res, const float* ls_gamma,
                                   const float* rowscale, void* y, int64_t M, int32_t C, int32_t ld, int64_t rows_per_sample, void* stream);
/* backward of the two passes above (mode 0: tanh-GELU, mode 1: layer scale + residual; reference
   ConNexT/models/block/mamba_vision.py:1517-1523): dx, dgamma, dbeta of the BatchNorm and, mode 1 with ls_gamma, d ls_gamma[c] =
   bn_gamma[c] sum d' xhat + bn_beta[c] sum d', d' = dy rowscale (the residual's gradient is dy itself).  The pre-BatchNorm
   gradient is recomputed from x, scale and shift.  One partial-sum pass into ws, a fixed-order final pass, one apply pass.
   training 0: running statistics, dx = scale * dz. */
hs_status hs_bn_epilogue_bwd(int32_t dtype, int32_t mode, const void* dy, const void* x, const float* scale, const float* shift,
                             const float* save_mean, const float* save_invstd, const float* bn_gamma, const float* bn_beta, const float* ls_gamma,
                             const float* rowscale, void* dx, float* dgamma, float* dbeta, float* dls_gamma, int32_t training, int64_t M, int32_t C,
                             int32_t ld, int64_t rows_per_sample, void* ws, int64_t ws_bytes, void* stream);
/* workspace of hs_bn_epilogue_bwd: [row blocks][C][2] partial sums + [C][3] coefficients (reference
   ConNexT/models/block/mamba_vision.py:1517-1523). */
int64_t hs_bn_epilogue_ws_bytes(int64_t M, int32_t C);
/* NHWC map [B][H][W][ld] of `dtype` -> tokens (B nWh nWw, ws ws, C) of `dtype`, zeros for positions right of W / below H: the
   padding and window_partition of reference ConNexT/models/block/mamba_vision.py:1301-1314,1813-1820 on the Downsample output.
   Also the backward of hs_window_reverse_nhwc. */
hs_status hs_window_partition_nhwc(int32_t dtype, const void* map, void* tokens, int32_t B, int32_t C, int32_t ld, int32_t H, int32_t W, int32_t ws,
                                   void* stream);
/* tokens -> NHWC map [B][H][W][ld], dropping the tokens of padded positions: window_reverse and the crop of reference
   ConNexT/models/block/mamba_vision.py:1317-1330,1825-1827.  Also the backward of hs_window_partition_nhwc. */
hs_status hs_window_reverse_nhwc(int32_t dtype, const void* tokens, void* map, int32_t B, int32_t C, int32_t ld, int32_t H, int32_t W, int32_t ws,
                                 void* stream);
/* out[b][t][:] = x[b][t][:] + v[b][:] (v f32): the pooled text feature added to every image token
   (reference modules/fusion_blocks.py:264-292, `image_tokens + txt_feat`). */
hs_status hs_add_token_bias_fwd(int32_t dtype, const void* x, const float* v, void* out, int32_t B, int32_t L, int32_t H,
                                void* stream);
/* dv[b][:] = sum_t dy[b][t][:] in time order (reference modules/fusion_blocks.py:264-292); dx is dy itself. */
hs_status hs_add_token_bias_bwd(int32_t dtype, const void* dy, float* dv, int32_t B, int32_t L, int32_t H, void* stream);
/* Token sequence of the multimodal Mamba blocks (reference ConNexT/models/block/len4mamba.py:86-106,147-168), f32:
   seq[b] = [text[b]; img[b][0..P-1]; first[b]; last[b]] + pe[0..P+2], rows of H = proj_dim; replaces torch.cat and the
   broadcast add of the positional encoding. */
hs_status hs_token_seq_assemble_fwd(const float* text, const float* img, const float* first, const float* last, const float* pe,
                                    float* seq, int32_t B, int32_t P, int32_t H, void* stream);
/* The rows of dseq [B][P+3][H] handed back to the four projections (reference ConNexT/models/block/len4mamba.py:86-106);
   a NULL output is skipped. */
hs_status hs_token_seq_assemble_bwd(const float* dseq, float* dtext, float* dimg, float* dfirst, float* dlast, int32_t B,
                                    int32_t P, int32_t H, void* stream);
/* dst[b][c][r] = src[b][r][c], f32: `img.permute(0, 2, 1)` of reference ConNexT/models/block/len4mamba.py:93,155 as the
   (B P, C) rows the projection GEMM reads; the same call with R and C swapped is its backward. */
hs_status hs_transpose_batched_f32(const float* src, float* dst, int32_t B, int32_t R, int32_t C, void* stream);

/* KANLinear.regularization_loss (reference ConNexT/models/block/kan1.py:216-236) on spline_weight viewed as
   [rows = out*in][coeffs]: loss = ra * sum_j l_j + re * entropy(l / sum l), l_j = mean_c |w[j][c]|; dw (optional) is
   d loss / d w.  Single workgroup, deterministic. */
hs_status hs_kan_regularization(const float* w, int64_t rows, int32_t coeffs, float reg_activation, float reg_entropy,
                                float* loss, float* dw, void* stream);

/* SupConLoss(temperature) on (B, D) features, mean over anchors, loss + d/d features
   (reference scripts/train.py:23-44).  ws: hs_supcon_ws_bytes(B, D); its size is not checked.  Single workgroup:
   1 <= B <= 256 is required, a larger batch is refused before anything is written.  An anchor without positives adds
   exactly 0 to the loss and to the gradient.  A zero-norm row is normalised as F.normalize does, by max(norm, 1e-12): its
   feature stays 0, and its gradient is the gradient of the normalised feature times 1e12. */
hs_status hs_supcon_loss(const float* feat, const int64_t* labels, int32_t B, int32_t D, float temperature, float* loss,
                         float* dfeat, float* ws, void* stream);
int64_t hs_supcon_ws_bytes(int32_t B, int32_t D);

/* The same loss over any number of rows, tiled on the f32-input MFMA (csrc/supcon.hip), for one process or for W ranks that
   have gathered the step's N = W * B rows.  `loss` is SupConLoss(temperature) over ALL N rows with the reference's constants:
   rows normalised by max(norm, 1e-12); row maximum over all j, the diagonal included; E_i = 1e-8 + sum_{j != i} exp(s_ij - mx_i)
   (the 1e-8 joins after the last online-softmax rescale); denominators P_i + 1e-8; mean over the N anchors.  `dfeat` (optional,
   [M][D]) is grad_scale * d loss / d feat for the rows row0 .. row0 + M - 1 only, the rows the caller owns; it contains the
   terms of the anchors outside those rows.  One process passes row0 = 0, M = N, grad_scale = 1.  An anchor without positives
   adds exactly 0 to the loss and to the gradient; a zero-norm row is treated as by hs_supcon_loss.
   Range: 1 <= N <= HS_SUPCON_TILED_MAX_N, 1 <= D <= HS_SUPCON_TILED_MAX_D, 0 <= row0, 1 <= M, row0 + M <= N.  Anything else,
   a NULL feat / labels / loss / ws, or a ws that is not 16-byte aligned is refused (HS_ERR_ARG) before anything is written.
   ws: hs_supcon_tiled_ws_bytes(N, D) = 4 * (N * Dp + 6 * N + [KS > 1] KS * N * (Dp + 5)) bytes, Dp = D rounded up to a
   multiple of 4: the normalised copy, which is the only copy of the features; six floats per row (norm, maximum, E, P,
   weight, the row's loss); and, where the keys are cut into KS > 1 runs so that a pass fills the device, the runs' partial
   results per row.  NT = ceil(N / 64) key tiles, want = min(NT, 16, ceil(512 / NT)), tps = ceil(NT / want) tiles per run,
   KS = ceil(NT / tps) <= 16: 1 for N <= 64 and for N > 32768, so the workspace stays below 17 N Dp + 86 N floats and has no
   N^2 term.  -1 for (N, D) outside the range.  The size of ws is not checked.  No N x N array exists.  No atomics: every sum
   has one order that depends on (N, D) alone (KS never depends on row0 or M), so a rerun repeats bitwise, and the rows of a
   sliced call equal those rows of the full call bitwise (so do the losses).  f32 throughout: s_ij is one fma chain of Dp
   terms, d fn_i one fma chain of up to 64 * tps terms per run and KS - 1 additions.  Four to six launches, no host
   synchronisation.  No reference counterpart for N > its batch: it is the reference's loss on the concatenated batch. */
#define HS_SUPCON_TILED_MAX_N 65536
#define HS_SUPCON_TILED_MAX_D 4096
int64_t hs_supcon_tiled_ws_bytes(int32_t N, int32_t D);
hs_status hs_supcon_tiled(const float* feat, const int64_t* labels, int32_t N, int32_t D, int32_t row0, int32_t M,
                          float temperature, float grad_scale, float* loss, float* dfeat, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------- */
/* ConvNeXt operators on NHWC activations (reference ConNexT/models/ourmodel.py:43,78 ->          */
/* transformers ConvNextModel: ConvNextLayer.dwconv / layer_scale_parameter, ConvNextEmbeddings   */
/* .patch_embeddings, ConvNextStage.downsampling_layer).                                          */
/* ------------------------------------------------------------------------------------------- */
/* depthwise ksize x ksize convolution (ksize in {3,5,7}), stride 1, padding ksize/2, C % 4 == 0.
   w: f32 [C][ksize*ksize] (memory of a torch groups=C weight (C,1,k,k)); bias f32 [C] or NULL. */
int64_t hs_dwconv_ws_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t ksize);
hs_status hs_dwconv_fwd(int32_t dtype, const void* x, const float* w, const float* bias, void* y, int32_t N, int32_t H,
                        int32_t W, int32_t C, int32_t ksize, void* ws, int64_t ws_bytes, void* stream);
/* dx (optional) = correlation of dy with the flipped filter; dw [C][k*k] and db [C] (optional) are reduced
   deterministically through ws. */
hs_status hs_dwconv_bwd(int32_t dtype, const void* x, const float* w, const void* dy, void* dx, float* dw, float* db,
                        int32_t N, int32_t H, int32_t W, int32_t C, int32_t ksize, void* ws, int64_t ws_bytes, void* stream);
/* out[m][c] = res[m][c] + gamma[c] * rowscale[m / rows_per_sample] * u[m][c]; rowscale (f32, one value per sample:
   stochastic depth keep/(1-p)) may be NULL. */
hs_status hs_layerscale_fwd(int32_t dtype, const void* u, const float* gamma, const float* rowscale, int32_t rows_per_sample,
                            const void* res, void* out, int64_t M, int32_t C, void* stream);
/* du (optional) = gamma * rowscale * dy ; dgamma[c] = sum_m rowscale * dy * u.  C % 4 == 0 as in the forward (refused
   otherwise); ws holds at least hs_layerscale_ws_bytes(M, C) bytes. */
hs_status hs_layerscale_bwd(int32_t dtype, const void* dy, const void* u, const float* gamma, const float* rowscale,
                            int32_t rows_per_sample, void* du, float* dgamma, void* ws, int64_t ws_bytes, int64_t M, int32_t C,
                            void* stream);
int64_t hs_layerscale_ws_bytes(int64_t M, int32_t C);
/* space-to-depth for stride == kernel convolutions: out[(n,p,q)][(r*k+s)*C + c] = x[n][p*k+r][q*k+s][c], P = H/k,
   Q = W/k (floor), row pitch ldo >= k*k*C (extra columns zeroed); _bwd is the inverse scatter into dx (N,H,W,C). */
hs_status hs_patchify_fwd(int32_t dtype, const void* x, void* out, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k,
                          int32_t ldo, void* stream);
hs_status hs_patchify_bwd(int32_t dtype, const void* dpatch, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k,
                          int32_t ldp, void* stream);

/* ------------------------------------------------------------------------------------------- */
/* KAN layer / MoE gating pieces (reference ConNexT/models/block/kan1.py:77-165, moe.py:171-291).  */
/* KANLinear(x) = [act(x) | b_splines(x)] @ [base_weight | spline_weight*spline_scaler]^T: the      */
/* feature / weight packing below, the contraction on hs_gemm.                                     */
/* ------------------------------------------------------------------------------------------- */
/* feat[b] = [act(x[b,:]) | bases(x[b,0]) .. bases(x[b,in-1])], row length in*(1 + grid_size + order);
   grid: (in, grid_size + 2*order + 1) knots.  base_act = the layer's `base_activation` (kan1.py:17,35): 0 SiLU (the
   reference default), 1 GELU (erf), 2 ReLU, 3 identity -- the KAN classifier head (reference modules/heads.py:108-140,
   `act_mode`) selects it.  At most 32 knots per feature (grid_size + 2*order + 1 <= 32), more are refused.  The knots of a
   feature must increase strictly.  A basis is 1 on [g[j], g[j+1]): x on a knot belongs to the interval it opens, and x at or
   beyond the last knot, or below the first, has all bases (and their derivatives) 0. */
hs_status hs_kan_features_fwd(const float* x, const float* grid, float* feat, int64_t B, int32_t in_f, int32_t grid_size,
                              int32_t order, int32_t base_act, void* stream);
hs_status hs_kan_features_bwd(const float* x, const float* grid, const float* dfeat, float* dx, int64_t B, int32_t in_f,
                              int32_t grid_size, int32_t order, int32_t base_act, void* stream);
/* wcat[o] = [base_w[o,:] | spline_w[o,i,:]*scaler[o,i] ...]  (scaler may be NULL), nb = grid_size + order.
   hs_kan_unpack_wgrad: d_base = the base columns of dwcat, d_spline = dwcat * scaler, d_scaler = <dwcat, spline_w> over nb
   (each d_* optional).  Both refuse out_f, in_f or nb < 1. */
hs_status hs_kan_pack_weight(const float* base_w, const float* spline_w, const float* scaler, float* wcat, int32_t out_f,
                             int32_t in_f, int32_t nb, void* stream);
hs_status hs_kan_unpack_wgrad(const float* dwcat, const float* spline_w, const float* scaler, float* d_base, float* d_spline,
                              float* d_scaler, int32_t out_f, int32_t in_f, int32_t nb, void* stream);
/* KAN grid update on the device (csrc/kan_grid.hip): KANLinear.update_grid without a host round trip, a sort, the
   (batch, in, out) tensor of per-feature spline outputs or a vendor solver.  f32 in, f32 out; nk = grid_size + 2*order + 1
   knots and nb = grid_size + order coefficients per feature; every (grid_size >= 1, order >= 0) with nk <= 32 is supported.

   hs_kan_grid_knots: the knot rows grid (in_f, nk) of the batch x (B, in_f), replacing the sort and the knot arithmetic of
   reference ConNexT/models/block/kan1.py:167-214 (lines 182-211).  Per feature: the order statistics of its column at the
   0-based positions ranks[0..grid_size] (a HOST array: torch.linspace(0, B-1, grid_size+1, dtype=int64), so the truncation
   is torch's by construction), its minimum and maximum, then in f32 with every operation rounded on its own and in the
   reference's order
       step = (max - min + 2*margin) / grid_size
       knot[order + j] = grid_eps * (j*step + min - margin) + one_minus_eps * statistic[j]          j = 0..grid_size
       knot[order - m] = knot[order] - step*m,  knot[order + grid_size + m] = knot[order + grid_size] + step*m     m = 1..order
   The statistics are the values torch.sort gives: equal values and +-0.0 compare equal (a selected zero is written as
   +0.0), a NaN sorts last.  A column does not influence another column's knots.  The selection is a radix select with integer
   counts (no atomics): a rerun repeats bitwise.  ws: hs_kan_grid_knots_ws_bytes() bytes -- 0 today (the counters live in
   LDS; ws may then be NULL), -1 for arguments the entry refuses.
   Refused before any launch (HS_ERR_ARG): x, ranks or grid NULL; B < 1; in_f < 1; an unsupported knot count; ws_bytes below
   hs_kan_grid_knots_ws_bytes(); a rank outside [0, B). */
int64_t hs_kan_grid_knots_ws_bytes(int64_t B, int32_t in_f, int32_t grid_size, int32_t order);
hs_status hs_kan_grid_knots(const float* x, const int64_t* ranks, float* grid, int64_t B, int32_t in_f, int32_t grid_size,
                            int32_t order, float grid_eps, float one_minus_eps, float margin, void* ws, int64_t ws_bytes,
                            void* stream);
/* hs_kan_refit: per-feature least-squares fit of spline coefficients on the knots grid_new (in_f, nk), replacing the batched
   torch.linalg.lstsq of reference kan1.py:112-142 (curve2coeff) and, in S-mode, the spline-output tensor of
   kan1.py:167-214 (lines 172-179, 214) as well.  With A_i (B x nb) the bases of x[:, i] on grid_new:
     S-mode (grid_old and spline_w given, y NULL): S_i = the bases on grid_old (in_f, nk), C_i[q][o] = spline_w[o][i][q] *
       scaler[o][i] (scaler NULL = 1; the product is rounded to f32 as the reference's scaled_spline_weight is), and
       out[o][i][:] = (A_i^+ S_i) C_i[:, o] -- the minimiser of |A_i sol - S_i C_i|, i.e. update_grid's fit;
     y-mode (y (B, in_f, out_f) given, grid_old and spline_w NULL): out[o][i][:] = A_i^+ y[:, i, o], i.e. curve2coeff.
   The bases come from the evaluation hs_kan_features_fwd uses.  A_i^T A_i and A_i^T S_i (or A_i^T Y_i) are summed in f64,
   one workspace slot per chunk of 256 rows, and the slots are added in chunk order: no atomics, a rerun repeats bitwise.
   A_i^+ = V diag(1/lambda) V^T A_i^T from a cyclic Jacobi eigen-decomposition of the Gram matrix in f64 (at most 24 sweeps),
   with the eigenvalues <= rcond^2 * lambda_max dropped, rcond = 2^-23 * max(B, nb): the default cutoff of torch.linalg.lstsq,
   applied to the squared singular values.  A feature of full column rank gets the least-squares solution; a rank-deficient
   one (a constant column, B < nb, ...) gets the truncated pseudo-inverse solution, the least-norm one among the minimisers
   (the reference's drivers are undefined or unbounded there).  out is (out_f, in_f, nb) like spline_w and may alias it.  The
   result is NOT divided by the scaler (kan1.py:214).  A feature's result depends on its own column alone.
   ws: hs_kan_refit_ws_bytes() = ceil(B/256) * in_f * nb * (nb + (y_mode ? out_f : nb)) doubles, 8-byte aligned; -1 for
   arguments the entry refuses.
   Refused before any launch (HS_ERR_ARG): x, grid_new, out or ws NULL; B < 1; in_f or out_f < 1; an unsupported knot count;
   both or neither of S-mode (grid_old / spline_w) and y-mode (y); S-mode with only one of grid_old, spline_w; ws_bytes below
   hs_kan_refit_ws_bytes(); a misaligned ws. */
int64_t hs_kan_refit_ws_bytes(int64_t B, int32_t in_f, int32_t out_f, int32_t grid_size, int32_t order, int32_t y_mode);
hs_status hs_kan_refit(const float* x, const float* grid_new, const float* grid_old, const float* y, const float* spline_w,
                       const float* scaler, float* out, int64_t B, int32_t in_f, int32_t out_f, int32_t grid_size, int32_t order,
                       void* ws, int64_t ws_bytes, void* stream);
/* noisy top-k gating on clean = x@w_gate (and raw_noise = x@w_noise when noisy): gates (B,E), load-balancing loss
   coef*(cv^2(importance)+cv^2(load)), plus everything the backward needs (p, top: (B,17) int32, z, sigma,
   loadrow, d_imp[E], d_load[E]).  E <= 16.
   noise: optional (B,E) standard-normal draw to use instead of the counter RNG (NULL = draw from `seed`): the reference's
   torch.randn_like(clean_logits), moe.py:247, recorded by a caller that wants its gating reproduced exactly.
   hs_moe_gate_bwd: d_clean (and d_raw, optional) from dgates and g_loss (optional: NULL = no loss gradient).  Like the forward
   it refuses anything but 1 <= k <= E <= 16, and B < 1; noisy gating with d_raw wanted needs raw_noise. */
hs_status hs_moe_gate_fwd(const float* clean, const float* raw_noise, const float* noise, int32_t B, int32_t E, int32_t k, int32_t noisy,
                          float noise_eps, uint64_t seed, float coef, float* gates, float* p, int32_t* top, float* z,
                          float* sigma, float* loadrow, float* loss, float* d_imp, float* d_load, void* stream);
hs_status hs_moe_gate_bwd(const float* clean, const float* raw_noise, const float* p, const int32_t* top, const float* z,
                          const float* sigma, const float* dgates, const float* g_loss, const float* d_imp,
                          const float* d_load, int32_t B, int32_t E, int32_t k, int32_t noisy, float* d_clean, float* d_raw,
                          void* stream);
/* y[b,:] = sum_e gates[b,e]*outs[e][b,:] (dense form of SparseDispatcher.combine, moe.py:86-103) and its backward.
   1 <= E <= 16; B < 1 or O < 1 is refused. */
hs_status hs_moe_combine_fwd(const float* gates, const float* const* outs, float* y, int32_t B, int32_t E, int32_t O,
                             void* stream);
hs_status hs_moe_combine_bwd(const float* gates, const float* const* outs, const float* dy, float* const* douts,
                             float* dgates, int32_t B, int32_t E, int32_t O, void* stream);

/* Streaming 1x1 convolution of the image tower (csrc/pw_stream.hip; reference: torchvision Bottleneck conv1 / conv3 / downsample
   + train-mode BatchNorm, encoder.py:35-58, mibf_net/model_resnet.py:15): y[M][N] = x[M][K] . w[N][K]^T in bf16 with f32
   accumulation, persistent workgroups over 64-row blocks.  stats (optional): hs_pointwise_stat_rows(M, N, K) rows of
   (count, mean, M2) per output channel -- the partials hs_bn_params.partial_rows consumes.  Covered shapes: K % 64 == 0,
   64 <= K <= 256, N % 128 == 0 or N == 64.  A measured alternative to hs_gemm for these layers (not faster end to end: see
   the kernel's header); the composite executors use it only under HAMSPINE_PW_STREAM=1. */
int32_t hs_pointwise_stat_rows(int64_t M, int32_t N, int32_t K);
hs_status hs_pointwise_fwd(const void* x, int64_t M, int32_t K, int32_t ldx, const void* w, int32_t N, void* y, int32_t ldy,
                           float* stats, void* stream);

/* Sparse dispatch (SparseDispatcher, moe.py:48-112: expert e sees only the rows with gates[b][e] > 0, i.e. k/E of the work).
   hs_moe_dispatch_index: idx[e*B + 0 .. count[e]) = those rows, ascending.  hs_rows_gather: dst[i] = src[idx[i]] (rows of D
   floats).  hs_rows_scatter_add: dst[idx[i]] += scale[idx[i]*ld_scale + col] * src[i] (scale may be NULL; idx unique, so the
   update is a plain read-modify-write and deterministic).  hs_rows_scatter_add_bwd: the backward of the weighted scatter for
   one expert column: dsrc[i] = gates[idx[i]][col] * dy[idx[i]], dgates[idx[i]][col] = <dy[idx[i]], src[i]>. */
hs_status hs_moe_dispatch_index(const float* gates, int32_t B, int32_t E, int32_t* idx, int32_t* count, void* stream);
hs_status hs_rows_gather(const float* src, const int32_t* idx, float* dst, int32_t n, int32_t D, void* stream);
hs_status hs_rows_scatter_add(float* dst, const int32_t* idx, const float* scale, int32_t ld_scale, int32_t col, const float* src,
                              int32_t n, int32_t D, void* stream);
hs_status hs_rows_scatter_add_bwd(const float* dy, const int32_t* idx, const float* gates, int32_t E, int32_t col, const float* src,
                                  float* dsrc, float* dgates, int32_t n, int32_t D, void* stream);

/* ------------------------------------------------------------------------------------------- */
/* Composite executors: one call = one nn.Module forward (or backward) of the reference's module  */
/* tree, launched from C++ so the Python host issues O(10) calls per step instead of O(1000).     */
/* Every composite has a *_query that returns the bytes of `saved` (activations kept for the      */
/* backward, also used as forward temporaries) and `ws` (scratch) it needs for a given descriptor. */
/* The caller allocates both; `saved` must be passed unchanged to the matching backward.          */
/* ------------------------------------------------------------------------------------------- */

/* multi-head attention core on projected q/k/v (materialised scores):
     S = scale * Q K^T (+ key mask) ; P = softmax(S) ; O = dropout(P) V
   q/k/v/o element (b, t, h, j) lives at  base + b*bs + t*ld + h*hd + j.
   Replaces the attention inside torch.nn.MultiheadAttention (reference modules/fusion_blocks.py:
   18-31,107-112; modules/heads.py:86) and transformers BertSelfAttention (encoder.py:131). */
typedef struct hs_attn_desc {
    int32_t dtype;
    int32_t B, H, Lq, Lk, hd;      /* batch, heads, query len, key len, head dim                  */
    int64_t q_bs, k_bs, v_bs, o_bs;/* batch strides (elements)                                    */
    int32_t q_ld, k_ld, v_ld, o_ld;/* token strides (elements)                                    */
    float scale;
    float dropout_p;
    uint64_t seed;
    const int64_t* key_mask;       /* [B][Lk], 0 = masked key; NULL = no mask                     */
} hs_attn_desc;
hs_status hs_attention_query(const hs_attn_desc* d, int64_t* saved_bytes, int64_t* ws_bytes);
hs_status hs_attention_fwd(const hs_attn_desc* d, const void* q, const void* k, const void* v, void* o, void* saved,
                           int64_t saved_bytes, void* ws, int64_t ws_bytes, void* stream);
/* dq/dk/dv use the q/k/v strides of the descriptor; do uses the o strides. */
hs_status hs_attention_bwd(const hs_attn_desc* d, const void* q, const void* k, const void* v, const void* d_o, void* dq,
                           void* dk, void* dv, void* saved, int64_t saved_bytes, void* ws, int64_t ws_bytes,
                           void* stream);

/* weight-gradient side stream inside the composites below: 1 on (or env HAMSPINE_OVERLAP=1), 0 off (default) = every
   kernel of a composite runs on the caller's stream. */
void hs_set_overlap(int32_t on);
/* Gradient milestones for bucketed data-parallel exchange (reference mibf_net/train_resnet.py:134: DDP starts a bucket's
   all-reduce when its last gradient is ready).  The NEXT hs_resnet_bwd / hs_bert_bwd on the calling thread records
   events[i] (hipEvent_t) on its stream right after the kernels that finish the parameter gradient at grad_ptrs[i] (one of the
   dw / db / dgamma / dbeta pointers of its descriptor) have been enqueued; entries it does not recognise are recorded when
   it returns.  n <= 64; n = 0 clears the list. */
hs_status hs_grad_milestones(int32_t n, const void* const* grad_ptrs, void* const* events);
/* 1 when the library was built with -DHS_MEASURE (the HAMSPINE_KNOCKOUT work-skipping switch of tools/knockout.sh is compiled
   in; results may be garbage when that variable is set), 0 for the release build.  bench.py refuses a measurement build. */
int32_t hs_measure_build(void);
/* BertLayer backward (bf16): weight gradients as K-contiguous GEMMs on transposed copies of dY and X (1, default) or straight
   from the row-major operands (0); measurement / A-B testing switch. */
void hs_set_wgrad_nt(int32_t on);
/* Text tower on packed rows: the grouped weight gradients walk only the 32-token chunks that hold a valid token (1, default;
   HAMSPINE_BERT_WGRAD_CHUNKS) or every padded column (0).  Same results bit for bit; measurement / A-B testing switch. */
void hs_set_bert_wgrad_chunks(int32_t on);
/* GEMMs with a device-side row count (hs_gemm_params.m_rows): deal the workgroups over the tile rows that hold a row, so the
   live tiles run on all eight XCDs (1, default; HAMSPINE_PACK_XCD_SPREAD) or over all tile rows (0).  Same results bit for bit. */
void hs_set_pack_xcd_spread(int32_t on);
/* number of weight-gradient GEMMs queued so far with a chunk-compacted K walk (process-wide; tests read which path ran) */
int64_t hs_gemm_k_cols_queued(void);

/* conv + BatchNorm pair of a residual block. `w` is the f32 filter stored KRSC (channels_last). */
typedef struct hs_conv_bn {
    int32_t Cin, Cout, R, stride, pad;
    const float* w;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float* dw;        /* backward outputs (f32); NULL = frozen parameter, wgrad skipped            */
    float* dgamma;
    float* dbeta;
} hs_conv_bn;

/* torchvision BasicBlock (n_main = 2: 3x3,3x3) / Bottleneck (n_main = 3: 1x1,3x3[stride],1x1) with an
   optional 1x1 downsample branch: y = relu(main(x) + (ds ? bn(conv(x)) : x)).
   Replaces torchvision.models.resnet.{BasicBlock,Bottleneck}.forward under reference
   encoder.py:69-72 and mibf_net/model_resnet.py:15. */
typedef struct hs_resblock_desc {
    int32_t dtype;
    int32_t N, H, W;              /* input image; channels = main[0].Cin                           */
    int32_t training;             /* BatchNorm mode                                                */
    float eps, momentum;
    int32_t n_main;
    hs_conv_bn main[3];
    int32_t has_ds;
    hs_conv_bn ds;
    int32_t inference;            /* 1 (only with training = 0): no backward follows -- every BatchNorm is folded into
                                     its convolution's epilogue (scale, shift, ReLU, identity add) and only the weight
                                     casts use `saved`                                                 */
} hs_resblock_desc;
hs_status hs_resblock_query(const hs_resblock_desc* d, int64_t* saved_bytes, int64_t* ws_bytes);
hs_status hs_resblock_fwd(const hs_resblock_desc* d, const void* x, void* y, void* saved, int64_t saved_bytes, void* ws,
                          int64_t ws_bytes, void* stream);
/* dx may be NULL (no input gradient wanted). */
hs_status hs_resblock_bwd(const hs_resblock_desc* d, const void* x, const void* y, const void* dy, void* dx, void* saved,
                          int64_t saved_bytes, void* ws, int64_t ws_bytes, void* stream);

/* ResNet stem: conv7x7/2 (3->64) + BN + ReLU + maxpool3x3/2 on an f32 NCHW image.
   Replaces reference encoder.py:63-68 (self.stem) / torchvision ResNet conv1..maxpool. */
typedef struct hs_stem_desc {
    int32_t dtype;
    int32_t N, H, W;              /* input image (3 channels, f32 NCHW)                            */
    int32_t training;
    float eps, momentum;
    hs_conv_bn cb;                /* Cin = 3, Cout = 64, R = 7, stride = 2, pad = 3                */
    int32_t inference;            /* as hs_resblock_desc.inference                                 */
} hs_stem_desc;
hs_status hs_stem_query(const hs_stem_desc* d, int64_t* saved_bytes, int64_t* ws_bytes);
hs_status hs_stem_fwd(const hs_stem_desc* d, const float* image, void* y, void* saved, int64_t saved_bytes, void* ws,
                      int64_t ws_bytes, void* stream);
hs_status hs_stem_bwd(const hs_stem_desc* d, const void* y, const void* dy, void* saved, int64_t saved_bytes, void* ws,
                      int64_t ws_bytes, void* stream);

/* Linear layer parameters (f32) and their gradient outputs. */
typedef struct hs_linear {
    int32_t in_f, out_f;
    const float* w;               /* [out][in]                                                     */
    const float* b;               /* [out] or NULL                                                 */
    float* dw;                    /* NULL = frozen                                                 */
    float* db;
} hs_linear;
typedef struct hs_norm {
    const float* gamma;
    const float* beta;
    float* dgamma;
    float* dbeta;
} hs_norm;

/* transformers BertLayer (post-LN, erf-GELU): self-attention + output dense/LN + FFN + output LN.
   Replaces transformers.models.bert.modeling_bert.BertLayer.forward under reference
   encoder.py:131, mibf_net/bert.py:12. */
typedef struct hs_bert_layer_desc {
    int32_t dtype;
    int32_t B, L, hidden, heads, inter;
    float ln_eps;
    float hidden_dropout, attn_dropout;   /* 0 in eval mode                                         */
    uint64_t seed;
    const int64_t* attention_mask;        /* [B][L], 1 = attend                                     */
    hs_linear q, k, v, ao;                /* attention.self.{query,key,value}, attention.output.dense */
    hs_norm ln1;                          /* attention.output.LayerNorm                             */
    hs_linear inter_l, out_l;             /* intermediate.dense, output.dense                       */
    hs_norm ln2;                          /* output.LayerNorm                                       */
} hs_bert_layer_desc;
hs_status hs_bert_layer_query(const hs_bert_layer_desc* d, int64_t* saved_bytes, int64_t* ws_bytes);
hs_status hs_bert_layer_fwd(const hs_bert_layer_desc* d, const void* x, void* y, void* saved, int64_t saved_bytes,
                            void* ws, int64_t ws_bytes, void* stream);
hs_status hs_bert_layer_bwd(const hs_bert_layer_desc* d, const void* x, const void* dy, void* dx, void* saved,
                            int64_t saved_bytes, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------- */
/* Whole-tower executors: one call runs a complete tower forward or backward (the stem and every residual block /
   the embeddings and every BertLayer), with the same kernels and per-composite layout code as the per-block entry
   points above.  They exist for the host side: the unchanged reference loop calls `model(...)` once per step
   (scripts/train.py:373-385, mibf_net/train_resnet.py:30-32), so the product can hand a whole tower to ONE C call
   instead of ~70 (descriptors are built once per module and reused; nothing is re-planned or re-allocated per block).
   Replaces torchvision ResNet.forward up to layer4 (reference encoder.py:88-100, mibf_net/model_resnet.py:15) and
   transformers BertModel.forward (encoder.py:130-134, mibf_net/bert.py:11-13).                                       */
/* ------------------------------------------------------------------------------------------- */
/* sizeof of ABI struct number `which` as the library was compiled: 0 hs_conv_geom, 1 hs_gemm_params, 2 hs_bn_params,
   3 hs_bn_bwd_params, 4 hs_attn_desc, 5 hs_conv_bn, 6 hs_resblock_desc, 7 hs_stem_desc, 8 hs_linear, 9 hs_norm,
   10 hs_bert_layer_desc, 11 hs_resnet_desc, 12 hs_resnet_plan, 13 hs_bert_desc, 14 hs_jpeg_info; -1 for an unknown number.  A binding
   (the ctypes mirror in hamspine/_lib.py, a reference-side stub) checks its own declarations against it. */
int64_t hs_abi_sizeof(int32_t which);

#define HS_RESNET_MAX_BLOCKS 24
#define HS_RESNET_MAX_TAPS 4
typedef struct hs_resnet_desc {
    hs_stem_desc stem;
    int32_t n_blocks;
    hs_resblock_desc blocks[HS_RESNET_MAX_BLOCKS];   /* layer1..layer4 flattened; block i takes block i-1's output    */
    int32_t n_taps;                                  /* block outputs handed back (encoder.py:94-100: layer2/3/4)     */
    int32_t tap_block[HS_RESNET_MAX_TAPS];           /* ascending block indices; the last one is n_blocks - 1          */
} hs_resnet_desc;
typedef struct hs_resnet_plan {
    int64_t saved_bytes, ws_bytes;
    int64_t tap_offset[HS_RESNET_MAX_TAPS];          /* byte offset of tap t inside `saved` (NHWC, compute dtype)      */
    int32_t tap_C[HS_RESNET_MAX_TAPS], tap_H[HS_RESNET_MAX_TAPS], tap_W[HS_RESNET_MAX_TAPS];
} hs_resnet_plan;
hs_status hs_resnet_query(const hs_resnet_desc* d, hs_resnet_plan* plan);
/* image: f32 NCHW.  The tap activations are left inside `saved` at plan.tap_offset. */
hs_status hs_resnet_fwd(const hs_resnet_desc* d, const float* image, void* saved, int64_t saved_bytes, void* ws,
                        int64_t ws_bytes, void* stream);
/* dy_taps[t]: gradient of tap t (NHWC, compute dtype) or NULL; the last tap's gradient is required.  Parameter
   gradients go to the dw / dgamma / dbeta pointers of the descriptor (NULL = frozen). */
hs_status hs_resnet_bwd(const hs_resnet_desc* d, const void* const* dy_taps, void* saved, int64_t saved_bytes, void* ws,
                        int64_t ws_bytes, void* stream);

/* Test / analysis aid (tests/test_decisions_gpu.py): byte offsets, inside the `saved` arena of hs_resnet_fwd, of every
   ReLU output of the tower and of the stem's max-pool arg-max, in forward order: [0] stem BN+ReLU output ([N][P][Q][C],
   compute dtype), [1] max-pool arg-max taps (uint8 [N][P2][Q2][C], tap = 3*dh + dw inside the 3x3 window), then per block
   its inner stage outputs (n_main - 1 of them) and its output.  Returns the number of entries (-1: bad descriptor or
   max_entries too small).  In bf16 mode entry [0] may be UNWRITTEN: the training forward pools relu(bn(c)) straight from the
   convolution output and never stores it (HAMSPINE_IMG_LEAN bit 0); the buffer stays reserved.  f32 mode always writes it. */
int32_t hs_resnet_debug_offsets(const hs_resnet_desc* d, int64_t* out, int32_t max_entries);

#define HS_BERT_MAX_LAYERS 24
typedef struct hs_bert_desc {
    int32_t dtype;
    int32_t B, L, hidden, vocab, max_pos, n_types;
    int32_t pad_id;                       /* nn.Embedding padding_idx of the word table (-1: none)                    */
    float ln_eps, embed_dropout;          /* BertEmbeddings LayerNorm eps / dropout (0 in eval mode)                   */
    uint64_t seed;                        /* dropout seed of this call: embeddings use it, layer i uses seed+16(i+1)   */
    const float* word;                    /* [vocab][hidden]                                                           */
    const float* pos;                     /* [max_pos][hidden]                                                         */
    const float* type0;                   /* [n_types][hidden]; row 0 is used (token_type_ids = 0)                     */
    const float* gamma;
    const float* beta;
    float* dword;                         /* gradient outputs, NULL = frozen                                           */
    float* dpos;
    float* dtype0;
    float* dgamma;
    float* dbeta;
    int32_t n_layers;
    hs_bert_layer_desc layers[HS_BERT_MAX_LAYERS];   /* attention_mask / seed fields are overridden per call           */
    /* 1: compute only the tokens whose attention_mask is non-zero (bf16, head dim 64, L <= 128, a mask must be given; anything
       else is an error -- the caller decides).  A kernel makes the row map on the device (cu[B + 1] = exclusive prefix sum of
       the valid counts, row_of[t] = padded row b*L + l of packed row t, T = cu[B]) and the host never reads it back: every
       grid and every buffer stays sized for B*L rows, packed rows occupy the first T rows of the same buffers.  Valid tokens
       keep their order, so holes in a mask are handled like padding; a sequence without valid tokens contributes no rows.
       last_hidden_state is written in the padded [B][L][hidden] layout with ZEROS at masked positions, and the backward
       ignores the cotangent there.  Kernels that sum over tokens (weight / bias / LayerNorm gradients) walk the PADDED positions
       and leave the masked ones out, where the padded tower adds exact zeros (the grouped weight gradients leave out whole
       32-token chunks without a valid token -- one MFMA each, products of zeros -- and keep the others whole and in order,
       hs_set_bert_wgrad_chunks): for right-padded masks every valid hidden state
       and every gradient is bitwise what the padded tower computes, dropout draws included.  With holes in a mask the
       attention sums over keys round differently and the attention-probability draws differ (their flat index counts keys
       in packed order). */
    int32_t pack_rows;
} hs_bert_desc;
/* 1 when the switches the library has latched (HAMSPINE_WGRAD_NT / hs_set_wgrad_nt, HAMSPINE_FUSED_ATTENTION) leave pack_rows
   the kernels it needs, 0 when a caller must keep the padded tower. */
int32_t hs_bert_pack_rows_available(void);
/* out_offset: byte offset of last_hidden_state ([B][L][hidden], compute dtype) inside `saved`; with pack_rows it is the ONLY
   way to find the output (the row map and the padded output sit in front of the other buffers). */
hs_status hs_bert_query(const hs_bert_desc* d, int64_t* saved_bytes, int64_t* ws_bytes, int64_t* out_offset);
hs_status hs_bert_fwd(const hs_bert_desc* d, const int64_t* ids, const int64_t* mask, void* saved, int64_t saved_bytes,
                      void* ws, int64_t ws_bytes, void* stream);
hs_status hs_bert_bwd(const hs_bert_desc* d, const int64_t* ids, const int64_t* mask, const void* dy, void* saved,
                      int64_t saved_bytes, void* ws, int64_t ws_bytes, void* stream);

/* y = act(x W^T + b) with optional dropout / residual; generic Linear fwd + bwd on [M][in] rows.
   Replaces torch.nn.Linear call sites of the reference (encoder.py:80-86, modules/ *.py, model.py:195-200,
   mibf_net/attention.py:40-45, mibf_net/model_resnet.py:16,22-34). */
hs_status hs_linear_fwd(int32_t dtype, const void* x, int64_t M, int32_t ldx, const hs_linear* lin, const void* w_lp,
                        void* y, int32_t ldy, int32_t out_dtype, int32_t act, void* preact, const void* residual,
                        int32_t ldr, float dropout_p, uint64_t seed, void* stream);
/* dx = (dy W) [* act'(preact)] ; dw/db per `lin` (skipped when NULL). `dy` must already include the
   activation derivative when act != none (use mul_mode to fold it into this call's dx = ... of the
   PREVIOUS layer instead).  ws: hs_linear_bwd_ws_bytes. */
hs_status hs_linear_bwd(int32_t dtype, const void* x, int64_t M, int32_t ldx, const hs_linear* lin, const void* w_lp,
                        const void* dy, int32_t ldy, void* dx, int32_t lddx, int32_t dx_dtype, int32_t mul_mode,
                        const void* mul_src, int32_t ldm, const void* dx_residual, void* ws, int64_t ws_bytes,
                        void* stream);
int64_t hs_linear_bwd_ws_bytes(int64_t M, int32_t in_f, int32_t out_f, int32_t dtype);

/* ------------------------------------------------------------------------------------------- */
/* callers either side of the path: inference helpers and input staging     */
/* ------------------------------------------------------------------------------------------- */
/* Test-time augmentation as ONE batch (replaces the per-variant model calls of reference scripts/predict.py:33-42,
   63-70): out[v] = op_v(x) over `planes` = B*C (or B*T*C) image planes of H x W f32.  ops[v]: 0 identity, 1 flip(-1)
   ("hflip"), 2 flip(-2) ("vflip"), 3 torch.rot90(k=1, dims=(-2,-1)) (square planes only).  1 <= V <= 8. */
hs_status hs_tta_expand(const float* x, float* out, int64_t planes, int32_t H, int32_t W, const int32_t* ops, int32_t V,
                        void* stream);
/* out[i] = mean over v of x[v*n + i]: torch.stack(logits_list, 0).mean(0) of scripts/predict.py:70. */
hs_status hs_group_mean(const float* x, float* out, int32_t V, int64_t n, void* stream);
/* out[v*n + i] = x[i]: tiles text tokens / ids / masks over the TTA variants (elements of 2, 4 or 8 bytes). */
hs_status hs_repeat(int32_t elem_bytes, const void* x, void* out, int64_t n, int32_t V, void* stream);
/* Grad-CAM map per image from one stage's activation and gradient, both [B][HW][C] (NHWC memory):
   w = mean_hw(grad); cam = relu(sum_c w[c] * act[:, c]); cam /= max(cam) if max(cam) > 0.
   Replaces the numpy loop of reference analysis_tools.py:78-93 (before its cv2.resize). */
hs_status hs_gradcam(int32_t dtype, const void* act, const void* grad, float* cam, int32_t B, int32_t C, int32_t HW,
                     void* stream);
/* Input staging: decoded u8 images [B][H][W][3] -> f32 [B][3][H][W], (v/255 - mean[c]) / std[c] in IEEE f32
   (torchvision ToTensor + Normalize of the reference's data pipeline, data_loader.py transforms). */
hs_status hs_stage_images_u8(const uint8_t* src, float* out, int32_t B, int32_t H, int32_t W, const float* mean,
                             const float* std, void* stream);

/* Device-side augmentation: the loaders' PIL transforms (RandomResizedCrop, flips, RandomRotation, ColorJitter; Resize +
   CenterCrop for eval) from a pack of decoded u8 images to the f32 [N][3][S][S] batch, bit-equal to Pillow's arithmetic
   (tests/augment_ref.py restates it).  The pack: one device byte arena; source i is [h][w][3] u8, tightly packed, at byte
   src_off[i] (any alignment).  All tables are HOST arrays, checked before any launch; only `arena`, `ws` and `out` are device
   memory.  Per output n:
     iparams[n][16] = source index, crop box top, left, h, w, hflip, vflip, rotate (0: no rotation stage), the colour order as a
                      permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue (4 ints), enable[op] (4 ints, by op)
     fparams[n][5]  = angle in degrees (Image.rotate's sign), brightness, contrast, saturation factors, hue shift in [-0.5, 0.5]
   Passes, in stream order, all on one workspace of hs_augment_ws_bytes (16-byte aligned):
     plan    resampling windows + 22-bit coefficients per output and axis, rotation matrices in 16.16, the output records
     resize  crop box -> S x S u8: horizontal pass (rounded to u8, rows the vertical pass reads), then the vertical pass
     stats   per output, the integer sum of L of the image as its contrast op meets it (skippable when no output has contrast)
     finish  rotation / flip gather (fill 0), colour ops in order with the u8 store between them, (v/255 - mean[c]) / std[c]
   The eval plan is Resize(R) + CenterCrop(S) of whole sources: shorter side to R, longer to int(R * long / short), window at
   int(round((len - S) / 2.0)) (half to even); R >= S.  The ws queries return -1 on a bad argument. */
int64_t hs_augment_ws_bytes(const int32_t* iparams, int32_t N, int32_t S);
int64_t hs_augment_eval_ws_bytes(const int32_t* src_h, const int32_t* src_w, int32_t n_src, const int32_t* src_index, int32_t N,
                                 int32_t R, int32_t S);
/* byte offset inside the workspace of what == 0: the int64 L sums [N] (stats), what == 1: the resized u8 images [N][S][S][3] */
int64_t hs_augment_ws_offset(int32_t what, int32_t N, int32_t S);
hs_status hs_augment_plan(const int32_t* src_h, const int32_t* src_w, const int64_t* src_off, int32_t n_src, int64_t arena_bytes,
                          const int32_t* iparams, const double* fparams, int32_t N, int32_t S, void* ws, int64_t ws_bytes,
                          void* stream);
hs_status hs_augment_plan_eval(const int32_t* src_h, const int32_t* src_w, const int64_t* src_off, int32_t n_src,
                               int64_t arena_bytes, const int32_t* src_index, int32_t N, int32_t R, int32_t S, void* ws,
                               int64_t ws_bytes, void* stream);
hs_status hs_augment_resize(const uint8_t* arena, void* ws, int32_t N, int32_t S, void* stream);
hs_status hs_augment_stats(void* ws, int32_t N, int32_t S, void* stream);
hs_status hs_augment_finish(const void* ws, float* out, int32_t N, int32_t S, const float* mean, const float* std, void* stream);

/* Device-side validation metrics (csrc/metrics.hip): the multiclass confusion matrix, precision / recall / F1 / accuracy and
   one-vs-rest AUROC without a host round trip per batch.  State lives in caller-owned device tensors:
     cm       [C][C] int64, row = label, column = prediction        invalid  one int64: rows whose label is outside [0, C)
     scores   [C][capacity] f32, class-major                        labels   [capacity] int32, -1 for an invalid row
   The number of stored rows n is a host integer.  2 <= C <= HS_METRICS_MAX_CLASSES; capacity < 2^31. */
#define HS_METRICS_MAX_CLASSES 64
/* the f64 vector of hs_metrics_finalize: HS_METRICS_SCALARS averages -- accuracy, macro precision / recall / F1, support-weighted
   precision / recall / F1, macro AUROC -- then HS_METRICS_PER_CLASS arrays of C: precision, recall, F1, AUROC, support */
#define HS_METRICS_SCALARS 8
#define HS_METRICS_PER_CLASS 5
/* One validation batch: logits [B][C] f32 or bf16, labels [B] int64, stored as rows n .. n + B - 1.  Per row: arg-max (lowest
   index on ties; NaN counts as the largest value, as in torch.argmax), softmax in f32 with the maximum subtracted (from_logits
   == 0 stores the values as given), the C scores written to column n + row, the label stored, cm[label][argmax] += 1.  A label
   outside [0, C) adds one to `invalid` instead; its score column is NaN and its stored label -1.  scores == labels == NULL
   keeps the matrix alone.  Replaces torch.argmax + MetricCollection.update + AUROC.update of reference
   ConNexT/models/pl_model_MOE2.py:159-163 and the per-batch .cpu() of scripts/train.py:113-119, mibf_net/train_resnet.py:52-57,
   ConNexT/models/test.py:97-104. */
hs_status hs_metrics_update(int32_t dtype, const void* logits, const int64_t* labels, int32_t B, int32_t C, int64_t n,
                            int64_t capacity, int64_t* cm, int64_t* invalid, float* scores, int32_t* stored_labels,
                            int32_t from_logits, void* stream);
/* cm[labels[i]][preds[i]] += 1 for i < B; a label or prediction outside [0, C) adds one to `invalid` instead.
   Replaces MetricCollection.update(pred_labels, labels) (pl_model_MOE2.py:161,163). */
hs_status hs_metrics_update_preds(const int64_t* preds, const int64_t* labels, int64_t B, int32_t C, int64_t* cm,
                                  int64_t* invalid, void* stream);
/* counts [C][4] int64, overwritten: per class c over the n stored rows, with positives = rows labelled c and negatives = rows
   with any other valid label: the number of (positive i, negative j) pairs with s_j < s_i, the number with s_j == s_i, the number
   of positives, the number of negatives.  Replaces torchmetrics AUROC.compute (pl_model_MOE2.py:170) and
   sklearn.metrics.roc_auc_score on host copies (mibf_net/predict_resnet_ham_image.py:103-110). */
hs_status hs_metrics_auroc(const float* scores, const int32_t* labels, int64_t n, int64_t capacity, int32_t C, int64_t* counts,
                           void* stream);
/* The counts of hs_metrics_auroc, integer for integer, in O(C n log n) instead of O(C n^2): per class the negatives' scores
   are radix-sorted as order-preserving 32-bit keys (-0.0 == +0.0, denormals by value, NaN set aside: such a row counts in P or
   Nn and takes part in no pair) and every positive finds its lower and upper bound among them.  Same arguments and limits as
   hs_metrics_auroc; n == 0 zeroes counts and needs no workspace.  `workspace` is caller-owned device memory, 16-byte aligned;
   hs_metrics_auroc_ranked_ws_bytes(n, C) (-1 outside the limits) holds all classes at once.  With less, but at least
   ws_bytes(n, C) / C, the classes are taken in as many rounds as fit; with less than one class's share the call is refused
   and nothing is written.  No read-back, no synchronisation.  Replaces, like hs_metrics_auroc, torchmetrics AUROC.compute
   (pl_model_MOE2.py:170) and sklearn.metrics.roc_auc_score (mibf_net/predict_resnet_ham_image.py:103-110), which sort too. */
int64_t hs_metrics_auroc_ranked_ws_bytes(int64_t n, int32_t C);
hs_status hs_metrics_auroc_ranked(const float* scores, const int32_t* labels, int64_t n, int64_t capacity, int32_t C,
                                  void* workspace, int64_t ws_bytes, int64_t* counts, void* stream);
/* out: HS_METRICS_SCALARS + HS_METRICS_PER_CLASS * C doubles, laid out as above; every division in f64 from the integer counts,
   0 where a denominator is 0.  Macro averages run over the classes with tp + fp + fn > 0, the weighted ones use the supports.
   AUROC of a class is (2 less + eq) / (2 P Nn), NaN without a positive or without a negative; its macro average runs over the
   defined classes.  counts == NULL: every AUROC is NaN.  Replaces the torchmetrics .compute() calls of pl_model_MOE2.py:169-171
   and the sklearn calls of ConNexT/models/test.py:112-130, scripts/train.py:121-129. */
hs_status hs_metrics_finalize(const int64_t* cm, const int64_t* counts, int32_t C, double* out, void* stream);

/* JPEG decode, split where it stops being serial (csrc/jpeg_host.h, csrc/jpeg.hip): DataLoader workers run the Huffman stage on
   the host and hand over quantised coefficients; dequantisation, the inverse DCT, chroma upsampling, YCbCr -> RGB and the copy
   into the pack are two kernels per batch.  The arithmetic is libjpeg's default path (the "islow" integer IDCT, "fancy" h2v1 /
   h2v2 upsampling, 16-bit colour tables; tests/jpeg_ref.py restates it), so the pixels equal Pillow's
   Image.open(path).convert("RGB") bit for bit.  Replaces the PIL decode of reference data_loader.py:258,274,285,
   mibf_net/dataset_spine.py:78-80 and ConNexT/dataset/pl_datset.py:136.

   Accepted: SOF0 and 8-bit SOF1 Huffman files with one interleaved scan, 1 component, or 3 components with luma 1x1, 2x1 or 2x2
   over 1x1 chroma (with a JFIF marker, or without an Adobe marker and with component ids other than 'R','G','B'), of fewer than
   2^31 output bytes (3 * h * w; HS_JPEG_ERR_TOO_LARGE otherwise: the device stage indexes bytes in 32 bits).  Everything else is
   refused with its own status and nothing is written; a damaged stream is HS_JPEG_ERR_CORRUPT. */
enum { HS_JPEG_ERR_CORRUPT = 16, HS_JPEG_ERR_PROGRESSIVE = 17, HS_JPEG_ERR_ARITHMETIC = 18, HS_JPEG_ERR_PROCESS = 19,
       HS_JPEG_ERR_PRECISION = 20, HS_JPEG_ERR_QTAB16 = 21, HS_JPEG_ERR_COMPONENTS = 22, HS_JPEG_ERR_SAMPLING = 23,
       HS_JPEG_ERR_MULTISCAN = 24, HS_JPEG_ERR_COLORSPACE = 25, HS_JPEG_ERR_NARROW = 26, HS_JPEG_ERR_TOO_LARGE = 27 };
#define HS_JPEG_MAX_COMPONENTS 3
typedef struct hs_jpeg_info {
    int32_t width, height, components;               /* components: 1 (gray) or 3 (YCbCr)                               */
    int32_t h_samp[HS_JPEG_MAX_COMPONENTS], v_samp[HS_JPEG_MAX_COMPONENTS];          /* 1 x 1 for a 1-component file     */
    int32_t block_rows[HS_JPEG_MAX_COMPONENTS], block_cols[HS_JPEG_MAX_COMPONENTS];  /* 8x8 blocks, padded to whole MCUs */
    int32_t restart_interval;
    int64_t coef_bytes;                              /* sum over components of block_rows * block_cols * 64 * 2          */
} hs_jpeg_info;
/* the text of a status of the two host entries below (a static string; "" for HS_OK) */
const char* hs_jpeg_status_text(hs_status status);
/* Host only, no HIP call, no global state, re-entrant: safe in a worker process that must never open the GPU.
   probe: reads the markers up to the first scan and fills `info`; HS_OK, a refusal or HS_JPEG_ERR_CORRUPT.
   entropy_decode: as probe, then zeroes `coef` and writes, per component one after another, int16 [block_rows][block_cols][64]
   quantised coefficients in natural (row-major) order, and qtab[c][64], component c's 8-bit quantisation table in natural
   order.  coef_bytes below info->coef_bytes is HS_ERR_ARG.  Never reads or writes out of bounds and always consumes input:
   a truncated file, a bad marker length, a Huffman code outside its table, a run past index 63, a DC category above 11 or an
   AC category above 10, a DC predictor that leaves int16, a missing or wrong RSTn and a missing table are all
   HS_JPEG_ERR_CORRUPT (the buffers may then be partly written).  Bytes after the last MCU are not looked at.
   A coded block takes at least 2 bits (a DC and an AC symbol), so a frame whose blocks cannot fit in the bytes behind SOS is
   corrupt already for probe, before anyone sizes a buffer from its header: a short file cannot ask for gigabytes. */
hs_status hs_jpeg_probe(const uint8_t* data, int64_t nbytes, hs_jpeg_info* info);
hs_status hs_jpeg_entropy_decode(const uint8_t* data, int64_t nbytes, int16_t* coef, int64_t coef_bytes, uint16_t* qtab,
                                 hs_jpeg_info* info);
/* Device stage.  HOST tables, checked before any launch, one row per image:
     geom[i][HS_JPEG_GEOM]  height, width (3 * h * w < 2^31), components, luma h_samp, luma v_samp, 0, 0, 0 (chroma is 1 x 1)
     coef_off / coef_len    byte offset (16-byte aligned) and length of image i inside the DEVICE arena `coef`; the length must be
                            what the geometry implies
     out_off                byte offset of image i's [h][w][3] u8 pixels inside the DEVICE arena `out` (pack_images' layout: any
                            alignment); ascending, not overlapping.  Bytes of `out` that belong to no image are not written.
   qtab: DEVICE uint16 [n][3][64].  ws: hs_jpeg_ws_bytes (-1 on a bad table), 16-byte aligned: the padded u8 planes.
   Two launches per HS_JPEG_CHUNK images (the checked image records travel in the kernels' arguments, as hs_augment_plan's do, so
   there is no table copy to order on the stream; a batch above HS_JPEG_CHUNK images takes a launch pair per chunk): dequantise + IDCT (one thread per block), then upsample + colour + pack (one thread
   per aligned 4 output bytes).  No atomics; bitwise repeatable. */
#define HS_JPEG_GEOM 8
#define HS_JPEG_CHUNK 32
int64_t hs_jpeg_ws_bytes(const int32_t* geom, int32_t n);
hs_status hs_jpeg_decode(const int16_t* coef, int64_t coef_bytes, const uint16_t* qtab, const int32_t* geom,
                         const int64_t* coef_off, const int64_t* coef_len, const int64_t* out_off, int32_t n, uint8_t* out,
                         int64_t out_bytes, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HAMSPINE_H */
