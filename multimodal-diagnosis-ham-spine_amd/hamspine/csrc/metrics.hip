// Device-side multiclass validation metrics (DESIGN.md "Device-side validation metrics").
//
//   update    per row: arg-max (lowest index on ties), softmax in f32, the probabilities stored class-major, the label
//             stored, one count added to the confusion matrix
//   preds     the confusion-matrix half alone, from predicted labels
//   auroc     per class, the pair counts of the Mann-Whitney statistic over the stored rows: an exact integer form of the area
//             under the ROC curve
//   ranked    the same counts from a radix sort of each class's negatives and a binary search per positive
//   finalize  every ratio in f64 from the integer counts, in one block
//
// All state is integer counts (or stored f32 values that no later launch re-rounds), and the counts are added with integer
// atomics after a per-block reduction: the result depends neither on the order of the batches nor on the order of the blocks.
#include <math.h>

#include "hs_common.h"

namespace hs {

static constexpr int kMetMaxC = HS_METRICS_MAX_CLASSES;
static constexpr int kMetRows = 16;          // rows of one update block: 4 waves x 4 rows
static constexpr int kMetThreads = 256;
static constexpr int kAucPerThread = 2;      // s_i a thread of the pair count keeps in registers
static constexpr int kAucTileI = kMetThreads * kAucPerThread;
static constexpr int kAucTileJ = 256;

__device__ __forceinline__ void add_i64(long long* p, unsigned long long v) {
    if (v) atomicAdd((unsigned long long*)p, v);
}

// sum over the block of a value below 2^32 per thread; every thread gets the sum.  red: kMetThreads / 64 words of LDS
__device__ __forceinline__ unsigned long long block_sum(unsigned v, unsigned long long* red) {
    unsigned long long s = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __syncthreads();                          // red may still be read from the call before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    s = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w];
    return s;
}

// order-preserving key of a logit for the arg-max: NaN above everything (numpy / torch: the first NaN wins), -0 == +0
__device__ __forceinline__ unsigned argmax_key(float v) {
    if (v != v) return 0xffffffffu;
    const unsigned b = __float_as_uint(v + 0.f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// ------------------------------------------------------------------------------------------------------------- update
// Replaces, per validation batch, torch.argmax(pred, 1) + the three torchmetrics updates of reference
// ConNexT/models/pl_model_MOE2.py:159-163 (and the .cpu() / softmax of scripts/train.py:113-119, ConNexT/models/test.py:97-104).
// One wave per row, lane c holds class c.  A block takes kMetRows consecutive rows, counts them in an LDS copy of the matrix
// and stages their probabilities in LDS, so that the class-major store writes runs of kMetRows floats.
template <typename T>
__global__ __launch_bounds__(kMetThreads) void metrics_update_kernel(const T* __restrict__ logits,
                                                                    const long long* __restrict__ labels, int B, int C,
                                                                    long long n, long long capacity, long long* __restrict__ cm,
                                                                    long long* __restrict__ invalid, float* __restrict__ scores,
                                                                    int* __restrict__ stored, int from_logits) {
    __shared__ unsigned s_cm[kMetMaxC * kMetMaxC];
    __shared__ float s_p[kMetMaxC][kMetRows + 1];
    __shared__ unsigned s_bad;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < C * C; i += kMetThreads) s_cm[i] = 0;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const long long row0 = (long long)blockIdx.x * kMetRows;
    for (int k = 0; k < kMetRows / 4; ++k) {
        const int lr = wv * (kMetRows / 4) + k;
        const long long r = row0 + lr;
        if (r >= B) break;                                    // wave-uniform
        const float x = lane < C ? to_f32(logits[r * C + lane]) : -INFINITY;
        // arg-max: the largest key, the lowest class among equals; lanes past C stay below every class
        unsigned long long best = lane < C ? ((unsigned long long)argmax_key(x) << 32) | (unsigned)(0xffffffffu - lane) : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other > best ? other : best;
        }
        int pred = (int)(0xffffffffu - (unsigned)best);
        pred = pred < 0 ? 0 : (pred >= C ? C - 1 : pred);
        float p = x;
        if (from_logits) {
            const float mx = wave_max(x);
            const float e = lane < C ? expf(x - mx) : 0.f;
            p = e / wave_sum(e);
        }
        const long long y = labels[r];
        const bool ok = y >= 0 && y < C;
        if (lane < C) s_p[lane][lr] = ok ? p : NAN;
        if (lane == 0) {
            if (ok) atomicAdd(&s_cm[(int)y * C + pred], 1u);
            else atomicAdd(&s_bad, 1u);
            if (stored) stored[n + r] = ok ? (int)y : -1;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += kMetThreads) add_i64(cm + i, s_cm[i]);
    if (threadIdx.x == 0) add_i64(invalid, s_bad);
    if (scores) {
        for (int i = threadIdx.x; i < C * kMetRows; i += kMetThreads) {
            const int c = i / kMetRows, lr = i % kMetRows;
            if (row0 + lr < B) scores[(long long)c * capacity + n + row0 + lr] = s_p[c][lr];
        }
    }
}

// MetricCollection.update(pred_labels, labels) of pl_model_MOE2.py:161,163: the confusion matrix alone
__global__ __launch_bounds__(kMetThreads) void metrics_preds_kernel(const long long* __restrict__ preds,
                                                                   const long long* __restrict__ labels, long long B, int C,
                                                                   long long* __restrict__ cm, long long* __restrict__ invalid) {
    __shared__ unsigned s_cm[kMetMaxC * kMetMaxC];
    __shared__ unsigned s_bad;
    for (int i = threadIdx.x; i < C * C; i += kMetThreads) s_cm[i] = 0;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    for (long long r = (long long)blockIdx.x * kMetThreads + threadIdx.x; r < B; r += (long long)gridDim.x * kMetThreads) {
        const long long y = labels[r], q = preds[r];
        if (y >= 0 && y < C && q >= 0 && q < C) atomicAdd(&s_cm[(int)y * C + (int)q], 1u);
        else atomicAdd(&s_bad, 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += kMetThreads) add_i64(cm + i, s_cm[i]);
    if (threadIdx.x == 0) add_i64(invalid, s_bad);
}

// -------------------------------------------------------------------------------------------------------------- auroc
// Replaces torchmetrics AUROC.compute (pl_model_MOE2.py:170) and sklearn roc_auc_score on host copies
// (mibf_net/predict_resnet_ham_image.py:103-110).  Grid (tile of i, class, span of j).  A thread keeps kAucPerThread scores
// s_i of POSITIVES (anything else is NaN, for which both comparisons are false); the tiles of j go through LDS with every score
// that is not a NEGATIVE's replaced by NaN, and are read as broadcasts.  The j range is cut into gridDim.z spans of `jspan`
// rows (a multiple of the tile) so that a few thousand rows still fill the machine; the counts are integers, so the cut
// changes nothing.  P and Nn are counted over i by the blocks of the first span.
__global__ __launch_bounds__(kMetThreads) void metrics_auroc_kernel(const float* __restrict__ scores,
                                                                   const int* __restrict__ labels, long long n,
                                                                   long long capacity, long long jspan,
                                                                   long long* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float s_j[kAucTileJ];
    __shared__ unsigned long long s_red[kMetThreads / 64];
    const int c = blockIdx.y;
    const float* sc = scores + (long long)c * capacity;
    float si[kAucPerThread];
    unsigned pos = 0, neg = 0;
#pragma unroll
    for (int u = 0; u < kAucPerThread; ++u) {
        const long long i = (long long)blockIdx.x * kAucTileI + u * kMetThreads + threadIdx.x;
        const int y = i < n ? labels[i] : -1;
        si[u] = y == c ? sc[i] : NAN;
        pos += y == c;
        neg += y >= 0 && y != c;
    }
    const unsigned long long P = block_sum(pos, s_red), Nn = block_sum(neg, s_red);
    unsigned less[kAucPerThread] = {}, eq[kAucPerThread] = {};
    if (P) {                                                   // block-uniform: a tile without positives has no pairs
        const long long jbeg = (long long)blockIdx.z * jspan, jend = jbeg + jspan < n ? jbeg + jspan : n;
        for (long long j0 = jbeg; j0 < jend; j0 += kAucTileJ) {
            __syncthreads();
            {
                const long long j = j0 + threadIdx.x;
                const int y = j < n ? labels[j] : -1;
                s_j[threadIdx.x] = (y >= 0 && y != c) ? sc[j] : NAN;
            }
            __syncthreads();
#pragma unroll 4
            for (int k = 0; k < kAucTileJ; k += 4) {
                const f32x4 v = *(const f32x4*)&s_j[k];
#pragma unroll
                for (int u = 0; u < kAucPerThread; ++u) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        less[u] += v[q] < si[u];
                        eq[u] += v[q] == si[u];
                    }
                }
            }
        }
    }
    unsigned long long l = 0, e = 0;                           // a thread's counts stay below 2^32 each (n < 2^31), their sums may not
#pragma unroll
    for (int u = 0; u < kAucPerThread; ++u) {
        l += block_sum(less[u], s_red);
        e += block_sum(eq[u], s_red);
    }
    if (threadIdx.x == 0) {
        add_i64(counts + c * 4 + 0, l);
        add_i64(counts + c * 4 + 1, e);
        if (blockIdx.z == 0) {
            add_i64(counts + c * 4 + 2, P);
            add_i64(counts + c * 4 + 3, Nn);
        }
    }
}

// ------------------------------------------------------------------------------------------------------ auroc, ranked
// The same counts in O(C n log n) (DESIGN.md "Rank-based AUROC and metrics over all ranks").  Per class c every row gets a
// 32-bit key: the order-preserving image of its score if the row is a NEGATIVE of c with a score that is not NaN, kRkNoKey
// otherwise.  No score maps to kRkNoKey (+inf is 0xff800000), so after a sort of all n keys the negatives stand in front in
// ascending order and whatever takes part in no pair stands behind them: the number of negatives need not be known, and a
// positive's lower and upper bound among the n keys are its `less` and `less + eq`.  The sort is a least-significant-digit
// radix sort, four passes of 8 bits, keys only: per pass a histogram per block of kRkTile keys, one exclusive scan per class
// over (digit, block), and a stable scatter.  A workspace slot holds one class: two key buffers and the table of the scan;
// the classes of one round are the grid's y.
static constexpr int kRkItems = 8;                            // keys of one thread per tile
static constexpr int kRkTile = kMetThreads * kRkItems;        // keys of one block: 2048
static constexpr int kRkDigits = 256;                         // 8 bits per pass; one thread of a block per digit
static constexpr int kRkSearch = 4;                           // rows of one thread of the search
static constexpr unsigned kRkNoKey = 0xffffffffu;
static_assert(kRkDigits == kMetThreads, "thread d of a block owns digit d");

// order-preserving image of a score: -0.0 is +0.0, denormals keep their value, NaN is kRkNoKey (csrc/kan_grid.hip: key_of)
__device__ __forceinline__ unsigned rank_key(float v) {
    unsigned b = __float_as_uint(v);
    if ((b & 0x7fffffffu) > 0x7f800000u) return kRkNoKey;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct RankSlots {
    unsigned* ws;                    // slot s: keys A [npad] | keys B [npad] | table [nblk][kRkDigits]
    long long slot_words, npad;
    int nblk, c0;                    // blocks per class; the class of slot 0
};

// key i of the pass's input: made from the stored row in the first pass, read from the other buffer afterwards
__device__ __forceinline__ unsigned rank_load(const float* __restrict__ sc, const int* __restrict__ labels,
                                              const unsigned* __restrict__ src, long long i, int c) {
    if (src) return src[i];
    const int y = labels[i];
    return (y >= 0 && y != c) ? rank_key(sc[i]) : kRkNoKey;
}

// pass p reads A for odd p > 0 and B for even p > 0, and writes the other: 0 -> A, A -> B, B -> A, A -> B
__device__ __forceinline__ const unsigned* rank_src(const unsigned* slot, long long npad, int pass) {
    return pass == 0 ? nullptr : slot + ((pass & 1) ? 0 : npad);
}

__global__ __launch_bounds__(kMetThreads) void metrics_rank_hist_kernel(const float* __restrict__ scores,
                                                                       const int* __restrict__ labels, long long n,
                                                                       long long capacity, RankSlots rs, int pass) {
    __shared__ unsigned s_h[kRkDigits];
    const int c = rs.c0 + blockIdx.y;
    unsigned* slot = rs.ws + (long long)blockIdx.y * rs.slot_words;
    const unsigned* src = rank_src(slot, rs.npad, pass);
    const float* sc = scores + (long long)c * capacity;
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kRkTile + threadIdx.x;
#pragma unroll
    for (int it = 0; it < kRkItems; ++it) {
        const long long i = base + it * kMetThreads;
        if (i < n) atomicAdd(&s_h[(rank_load(sc, labels, src, i, c) >> (8 * pass)) & 255u], 1u);
    }
    __syncthreads();
    slot[2 * rs.npad + (long long)blockIdx.x * kRkDigits + threadIdx.x] = s_h[threadIdx.x];
}

// table[b][d] <- the number of keys with a smaller digit, or with digit d in a block before b: where block b puts its first
// key of digit d.  One block per class; thread d walks column d.
__global__ __launch_bounds__(kMetThreads) void metrics_rank_scan_kernel(RankSlots rs) {
    __shared__ unsigned s_t[kRkDigits];
    unsigned* col = rs.ws + (long long)blockIdx.x * rs.slot_words + 2 * rs.npad + threadIdx.x;
    unsigned tot = 0;
#pragma unroll 8
    for (int b = 0; b < rs.nblk; ++b) tot += col[(long long)b * kRkDigits];
    s_t[threadIdx.x] = tot;
    __syncthreads();
    unsigned run = 0;
    for (int d = 0; d < (int)threadIdx.x; ++d) run += s_t[d];
    for (int b = 0; b < rs.nblk; ++b) {
        const unsigned v = col[(long long)b * kRkDigits];
        col[(long long)b * kRkDigits] = run;
        run += v;
    }
}

// Stable: a block takes its tile in kRkItems rounds of one key per thread, in row order; within a round a key goes behind the
// keys of its digit in the waves before its own (s_w) and in the lanes before its own (the ballots).
__global__ __launch_bounds__(kMetThreads) void metrics_rank_scatter_kernel(const float* __restrict__ scores,
                                                                          const int* __restrict__ labels, long long n,
                                                                          long long capacity, RankSlots rs, int pass) {
    __shared__ unsigned s_base[kRkDigits];
    __shared__ unsigned s_w[kMetThreads / 64][kRkDigits];
    const int c = rs.c0 + blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned* slot = rs.ws + (long long)blockIdx.y * rs.slot_words;
    const unsigned* src = rank_src(slot, rs.npad, pass);
    unsigned* dst = slot + ((pass & 1) ? rs.npad : 0);
    const float* sc = scores + (long long)c * capacity;
    s_base[threadIdx.x] = slot[2 * rs.npad + (long long)blockIdx.x * kRkDigits + threadIdx.x];
#pragma unroll
    for (int w = 0; w < kMetThreads / 64; ++w) s_w[w][threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kRkTile + threadIdx.x;
    for (int it = 0; it < kRkItems; ++it) {
        const long long i = base + it * kMetThreads;
        const bool live = i < n;
        const unsigned key = live ? rank_load(sc, labels, src, i, c) : 0u;
        const unsigned digit = (key >> (8 * pass)) & 255u;
        unsigned long long peers = __ballot(live);             // the live lanes of this wave with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long m = __ballot(live && bit);
            peers &= bit ? m : ~m;
        }
        const unsigned long long before = peers & ((1ull << lane) - 1ull);
        if (live && before == 0) s_w[wv][digit] = (unsigned)__popcll(peers);
        __syncthreads();
        if (live) {
            unsigned at = s_base[digit] + (unsigned)__popcll(before);
            for (int w = 0; w < wv; ++w) at += s_w[w][digit];
            if (at < n) dst[at] = key;                         // always, if the table is this pass's; a bound all the same
        }
        __syncthreads();
        unsigned add = 0;
#pragma unroll
        for (int w = 0; w < kMetThreads / 64; ++w) {
            add += s_w[w][threadIdx.x];
            s_w[w][threadIdx.x] = 0;
        }
        s_base[threadIdx.x] += add;
        __syncthreads();
    }
}

// every positive with a score looks its key up among the sorted keys (buffer B after four passes); P and Nn count NaN rows too
__global__ __launch_bounds__(kMetThreads) void metrics_rank_search_kernel(const float* __restrict__ scores,
                                                                         const int* __restrict__ labels, long long n,
                                                                         long long capacity, RankSlots rs,
                                                                         long long* __restrict__ counts) {
    __shared__ unsigned long long s_red[kMetThreads / 64];
    const int c = rs.c0 + blockIdx.y;
    const unsigned* sorted = rs.ws + (long long)blockIdx.y * rs.slot_words + rs.npad;
    const float* sc = scores + (long long)c * capacity;
    unsigned pos = 0, neg = 0;
    unsigned long long less = 0, eq = 0;                       // kRkSearch counts below 2^31 each
#pragma unroll
    for (int u = 0; u < kRkSearch; ++u) {
        const long long i = ((long long)blockIdx.x * kRkSearch + u) * kMetThreads + threadIdx.x;
        const int y = i < n ? labels[i] : -1;
        pos += y == c;
        neg += y >= 0 && y != c;
        const unsigned k = y == c ? rank_key(sc[i]) : kRkNoKey;
        if (k == kRkNoKey) continue;
        unsigned lo = 0, hi = (unsigned)n;
        while (lo < hi) {
            const unsigned mid = lo + ((hi - lo) >> 1);
            if (sorted[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        const unsigned lower = lo;
        hi = (unsigned)n;
        while (lo < hi) {
            const unsigned mid = lo + ((hi - lo) >> 1);
            if (sorted[mid] <= k) lo = mid + 1;
            else hi = mid;
        }
        less += lower;
        eq += lo - lower;
    }
    const unsigned long long P = block_sum(pos, s_red), Nn = block_sum(neg, s_red);
    const unsigned long long l = block_sum((unsigned)less, s_red) + (block_sum((unsigned)(less >> 32), s_red) << 32);
    const unsigned long long e = block_sum((unsigned)eq, s_red) + (block_sum((unsigned)(eq >> 32), s_red) << 32);
    if (threadIdx.x == 0) {
        add_i64(counts + c * 4 + 0, l);
        add_i64(counts + c * 4 + 1, e);
        add_i64(counts + c * 4 + 2, P);
        add_i64(counts + c * 4 + 3, Nn);
    }
}

static long long rank_npad(long long n) { return (n + 3) & ~3ll; }
static long long rank_slot_words(long long n) { return n ? 2 * rank_npad(n) + (long long)ceil_div(n, kRkTile) * kRkDigits : 0; }

// ----------------------------------------------------------------------------------------------------------- finalize
// Replaces the torchmetrics .compute() calls of pl_model_MOE2.py:169-171 and the sklearn calls of ConNexT/models/test.py:
// 112-130, scripts/train.py:121-129.  One wave; lane c owns class c, lane 0 adds the averages up in class order.
__device__ __forceinline__ double ratio(double num, double den) { return den != 0.0 ? num / den : 0.0; }

__global__ __launch_bounds__(64) void metrics_finalize_kernel(const long long* __restrict__ cm,
                                                             const long long* __restrict__ counts, int C,
                                                             double* __restrict__ out) {
    __shared__ double s_prec[kMetMaxC], s_rec[kMetMaxC], s_f1[kMetMaxC], s_auc[kMetMaxC], s_sup[kMetMaxC], s_tp[kMetMaxC];
    __shared__ int s_seen[kMetMaxC];
    const int c = threadIdx.x;
    if (c < C) {
        long long tp = cm[c * C + c], row = 0, col = 0;
        for (int k = 0; k < C; ++k) {
            row += cm[c * C + k];
            col += cm[k * C + c];
        }
        const long long fp = col - tp, fn = row - tp;
        s_tp[c] = (double)tp;
        s_sup[c] = (double)row;
        s_seen[c] = tp + fp + fn > 0;
        s_prec[c] = ratio((double)tp, (double)(tp + fp));
        s_rec[c] = ratio((double)tp, (double)(tp + fn));
        s_f1[c] = ratio((double)(2 * tp), (double)(2 * tp + fp + fn));
        double auc = NAN;
        if (counts) {
            const long long less = counts[c * 4], eq = counts[c * 4 + 1], P = counts[c * 4 + 2], Nn = counts[c * 4 + 3];
            if (P > 0 && Nn > 0) auc = (double)(2 * less + eq) / (2.0 * (double)P * (double)Nn);
        }
        s_auc[c] = auc;
        double* pc = out + HS_METRICS_SCALARS;
        pc[0 * C + c] = s_prec[c];
        pc[1 * C + c] = s_rec[c];
        pc[2 * C + c] = s_f1[c];
        pc[3 * C + c] = auc;
        pc[4 * C + c] = s_sup[c];
    }
    __syncthreads();
    if (c == 0) {
        double trace = 0, total = 0, mp = 0, mr = 0, mf = 0, wp = 0, wr = 0, wf = 0, ma = 0;
        int seen = 0, defined = 0;
        for (int k = 0; k < C; ++k) {
            trace += s_tp[k];
            total += s_sup[k];
            if (s_seen[k]) {
                mp += s_prec[k];
                mr += s_rec[k];
                mf += s_f1[k];
                ++seen;
            }
            wp += s_sup[k] * s_prec[k];
            wr += s_sup[k] * s_rec[k];
            wf += s_sup[k] * s_f1[k];
            if (s_auc[k] == s_auc[k]) {
                ma += s_auc[k];
                ++defined;
            }
        }
        out[0] = ratio(trace, total);
        out[1] = ratio(mp, (double)seen);
        out[2] = ratio(mr, (double)seen);
        out[3] = ratio(mf, (double)seen);
        out[4] = ratio(wp, total);
        out[5] = ratio(wr, total);
        out[6] = ratio(wf, total);
        out[7] = defined ? ma / (double)defined : NAN;
    }
}

static int metrics_classes_ok(int C) { return C >= 2 && C <= kMetMaxC; }

}  // namespace hs

using namespace hs;

extern "C" {

hs_status hs_metrics_update(int32_t dtype, const void* logits, const int64_t* labels, int32_t B, int32_t C, int64_t n,
                            int64_t capacity, int64_t* cm, int64_t* invalid, float* scores, int32_t* stored_labels,
                            int32_t from_logits, void* stream) {
    HS_REQUIRE(metrics_classes_ok(C), "hs_metrics_update: %d classes, supported 2..%d", C, kMetMaxC);
    HS_REQUIRE(dtype == HS_F32 || dtype == HS_BF16, "hs_metrics_update: dtype %d", dtype);
    HS_REQUIRE(B >= 0 && logits && labels && cm && invalid, "hs_metrics_update: null pointer or negative batch");
    HS_REQUIRE((scores == nullptr) == (stored_labels == nullptr), "hs_metrics_update: scores and labels are kept together");
    if (scores)
        HS_REQUIRE(n >= 0 && capacity >= 0 && n <= capacity && (int64_t)B <= capacity - n && capacity < (1ll << 31),
                   "hs_metrics_update: rows %lld + %d do not fit the capacity %lld", (long long)n, B, (long long)capacity);
    if (B == 0) return HS_OK;
    const int grid = ceil_div(B, kMetRows);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == HS_F32)
        metrics_update_kernel<float><<<grid, kMetThreads, 0, st>>>((const float*)logits, (const long long*)labels, B, C, n,
                                                                    capacity, (long long*)cm, (long long*)invalid, scores,
                                                                    stored_labels, from_logits);
    else
        metrics_update_kernel<bf16_t><<<grid, kMetThreads, 0, st>>>((const bf16_t*)logits, (const long long*)labels, B, C, n,
                                                                     capacity, (long long*)cm, (long long*)invalid, scores,
                                                                     stored_labels, from_logits);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_metrics_update_preds(const int64_t* preds, const int64_t* labels, int64_t B, int32_t C, int64_t* cm,
                                  int64_t* invalid, void* stream) {
    HS_REQUIRE(metrics_classes_ok(C), "hs_metrics_update_preds: %d classes, supported 2..%d", C, kMetMaxC);
    HS_REQUIRE(B >= 0 && preds && labels && cm && invalid, "hs_metrics_update_preds: null pointer or negative batch");
    if (B == 0) return HS_OK;
    const long long blocks = (B + kMetThreads - 1) / kMetThreads;
    metrics_preds_kernel<<<(int)(blocks > 1024 ? 1024 : blocks), kMetThreads, 0, (hipStream_t)stream>>>(
        (const long long*)preds, (const long long*)labels, B, C, (long long*)cm, (long long*)invalid);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

hs_status hs_metrics_auroc(const float* scores, const int32_t* labels, int64_t n, int64_t capacity, int32_t C, int64_t* counts,
                           void* stream) {
    HS_REQUIRE(metrics_classes_ok(C), "hs_metrics_auroc: %d classes, supported 2..%d", C, kMetMaxC);
    HS_REQUIRE(scores && labels && counts, "hs_metrics_auroc: null pointer");
    HS_REQUIRE(n >= 0 && n <= capacity && capacity < (1ll << 31), "hs_metrics_auroc: %lld rows, capacity %lld", (long long)n,
               (long long)capacity);
    hipStream_t st = (hipStream_t)stream;
    HS_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)C * 4 * sizeof(int64_t), st));
    if (n == 0) return HS_OK;
    // spans of j: as many as bring the grid to about four blocks per CU, at least one tile each
    const int itiles = ceil_div(n, kAucTileI), jtiles = ceil_div(n, kAucTileJ);
    int spans = 1024 / (itiles * C);
    spans = spans < 1 ? 1 : (spans > jtiles ? jtiles : spans);
    const long long jspan = (long long)ceil_div(jtiles, spans) * kAucTileJ;
    spans = ceil_div(n, jspan);
    metrics_auroc_kernel<<<dim3(itiles, C, spans), kMetThreads, 0, st>>>(scores, labels, n, capacity, jspan, (long long*)counts);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

int64_t hs_metrics_auroc_ranked_ws_bytes(int64_t n, int32_t C) {
    if (!metrics_classes_ok(C) || n < 0 || n >= (1ll << 31)) return -1;
    return (int64_t)C * rank_slot_words(n) * 4;
}

hs_status hs_metrics_auroc_ranked(const float* scores, const int32_t* labels, int64_t n, int64_t capacity, int32_t C,
                                  void* workspace, int64_t ws_bytes, int64_t* counts, void* stream) {
    HS_REQUIRE(metrics_classes_ok(C), "hs_metrics_auroc_ranked: %d classes, supported 2..%d", C, kMetMaxC);
    HS_REQUIRE(scores && labels && counts, "hs_metrics_auroc_ranked: null pointer");
    HS_REQUIRE(n >= 0 && n <= capacity && capacity < (1ll << 31), "hs_metrics_auroc_ranked: %lld rows, capacity %lld",
               (long long)n, (long long)capacity);
    const long long slot_words = rank_slot_words(n);
    if (n > 0) {
        HS_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "hs_metrics_auroc_ranked: workspace is null or not 16-byte aligned");
        HS_REQUIRE(ws_bytes >= slot_words * 4, "hs_metrics_auroc_ranked: workspace of %lld bytes, one class of %lld rows takes %lld",
                   (long long)ws_bytes, (long long)n, slot_words * 4);
    }
    hipStream_t st = (hipStream_t)stream;
    HS_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)C * 4 * sizeof(int64_t), st));
    if (n == 0) return HS_OK;
    const long long fit = ws_bytes / (slot_words * 4);
    const int per_round = fit < C ? (int)fit : C;              // classes sorted side by side
    RankSlots rs;
    rs.ws = (unsigned*)workspace;
    rs.slot_words = slot_words;
    rs.npad = rank_npad(n);
    rs.nblk = ceil_div(n, kRkTile);
    for (int c0 = 0; c0 < C; c0 += per_round) {
        const int cls = C - c0 < per_round ? C - c0 : per_round;
        rs.c0 = c0;
        for (int pass = 0; pass < 4; ++pass) {
            metrics_rank_hist_kernel<<<dim3(rs.nblk, cls), kMetThreads, 0, st>>>(scores, labels, n, capacity, rs, pass);
            HS_LAUNCH_CHECK();
            metrics_rank_scan_kernel<<<cls, kMetThreads, 0, st>>>(rs);
            HS_LAUNCH_CHECK();
            metrics_rank_scatter_kernel<<<dim3(rs.nblk, cls), kMetThreads, 0, st>>>(scores, labels, n, capacity, rs, pass);
            HS_LAUNCH_CHECK();
        }
        metrics_rank_search_kernel<<<dim3(ceil_div(n, kRkSearch * kMetThreads), cls), kMetThreads, 0, st>>>(
            scores, labels, n, capacity, rs, (long long*)counts);
        HS_LAUNCH_CHECK();
    }
    return HS_OK;
}

hs_status hs_metrics_finalize(const int64_t* cm, const int64_t* counts, int32_t C, double* out, void* stream) {
    HS_REQUIRE(metrics_classes_ok(C), "hs_metrics_finalize: %d classes, supported 2..%d", C, kMetMaxC);
    HS_REQUIRE(cm && out, "hs_metrics_finalize: null pointer");
    metrics_finalize_kernel<<<1, 64, 0, (hipStream_t)stream>>>((const long long*)cm, (const long long*)counts, C, out);
    HS_LAUNCH_CHECK();
    return HS_OK;
}

}  // extern "C"
