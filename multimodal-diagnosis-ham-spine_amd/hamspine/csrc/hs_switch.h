// Every environment switch of the library, once: the only place in csrc/ that reads the environment.  Host only (no HIP
// include), so a plain C++ program can compile it.  hs::sw::<id>() returns the switch's value.
//
// rule     how the variable's text becomes the value (d = the default, taken when the variable is unset):
//            off_if_0      0 only if the text starts with '0', else d        (d = 1)
//            on_if_1       1 only if the text starts with '1', else d        (d = 0)
//            int_any       atoi
//            int_mask15    atoi & 15
//            int_1to8      atoi if in 1..8, else d
//            int_positive  atoll if > 0 (unset counts as 0), else d
// latch    once      read at the switch's first use, which is never library load: callers set variables after loading it
//          per_call  read at every use: tests and A/B runs compare both settings in one process
//          settable  as once, and sw::set_<id>(on) -- behind the C-ABI setter named in the next column -- overrides the
//                    environment, before or after the first use
#pragma once
#include <atomic>
#include <stdlib.h>

namespace hs {
namespace sw {

inline long long off_if_0(const char* e, long long d) { return (e && e[0] == '0') ? 0 : d; }
inline long long on_if_1(const char* e, long long d) { return (e && e[0] == '1') ? 1 : d; }
inline long long int_any(const char* e, long long d) { return e ? atoi(e) : d; }
inline long long int_mask15(const char* e, long long d) { return e ? (atoi(e) & 15) : d; }
inline long long int_1to8(const char* e, long long d) { const long long v = e ? atoi(e) : d; return v >= 1 && v <= 8 ? v : d; }
inline long long int_positive(const char* e, long long d) { const long long v = e ? atoll(e) : 0; return v > 0 ? v : d; }

// clang-format off
//  id                  variable                        rule          d    latch     setter / the non-default setting
#define HS_SWITCHES(X) \
  /* ---- GEMM core (gemm.hip) ---- */ \
  X(p8,                 "HAMSPINE_P8",                  off_if_0,     1,   once,     -, "every GEMM on the generic body, none on the phase-pipelined one") \
  X(p8_wgrad,           "HAMSPINE_P8_WGRAD",            off_if_0,     1,   once,     -, "grouped deep-K weight gradients keep the generic 256x128 tiles") \
  X(conv3,              "HAMSPINE_CONV3",               off_if_0,     1,   once,     -, "3x3 stride-1 convolutions on the generic implicit GEMM, not the halo-patch kernel") \
  X(parity_dgrad,       "HAMSPINE_PARITY_DGRAD",        off_if_0,     1,   once,     -, "stride-2 data gradients keep the natural row order") \
  X(pack_xcd_spread,    "HAMSPINE_PACK_XCD_SPREAD",     off_if_0,     1,   settable, hs_set_pack_xcd_spread, "packed-row launches do not deal their live tiles over all XCDs") \
  X(persistent,         "HAMSPINE_PERSISTENT",          on_if_1,      0,   once,     -, "persistent GEMM launches (measured: no gain)") \
  X(epi_hist,           "HAMSPINE_EPI_HIST",            on_if_1,      0,   once,     -, "measurement: count the epilogue feature sets of the launches, print at exit") \
  X(group_debug,        "HAMSPINE_GROUP_DEBUG",         on_if_1,      0,   once,     -, "measurement: report every upload of a grouped launch's problem table") \
  X(split_units,        "HAMSPINE_SPLIT_UNITS",         int_positive, 512, once,     -, "measurement: the number of workgroups split-K aims at") \
  X(split_max,          "HAMSPINE_SPLIT_MAX",           int_positive, 64,  once,     -, "measurement: the largest split-K factor") \
  /* ---- attention (attn_fused.hip, blocks.hip) ---- */ \
  X(fused_attention,    "HAMSPINE_FUSED_ATTENTION",     off_if_0,     1,   once,     -, "the unfused attention path") \
  /* ---- composites and towers (blocks.hip) ---- */ \
  X(overlap,            "HAMSPINE_OVERLAP",             on_if_1,      0,   settable, hs_set_overlap, "a composite's weight gradients run on a side stream beside its data-gradient chain") \
  X(wgrad_nt,           "HAMSPINE_WGRAD_NT",            off_if_0,     1,   settable, hs_set_wgrad_nt, "BertLayer weight gradients from the row-major operands (tn); no packed rows then") \
  X(bert_wgrad_chunks,  "HAMSPINE_BERT_WGRAD_CHUNKS",   off_if_0,     1,   settable, hs_set_bert_wgrad_chunks, "packed text tower: weight gradients walk every padded column") \
  X(grouped_bert_wgrad, "HAMSPINE_GROUPED_BERT_WGRAD",  off_if_0,     1,   once,     -, "every weight-gradient GEMM of a BertLayer on its own") \
  X(wgrad_layers,       "HAMSPINE_WGRAD_LAYERS",        int_1to8,     2,   once,     -, "BERT layers whose weight gradients share one grouped grid (1: flush per layer)") \
  X(dgrad_nt,           "HAMSPINE_DGRAD_NT",            off_if_0,     1,   once,     -, "BERT data gradients read the row-contiguous weights") \
  X(defer_transposes,   "HAMSPINE_DEFER_TRANSPOSES",    off_if_0,     1,   once,     -, "one launch per dY^T where the gradient appears") \
  X(fused_bias_grad,    "HAMSPINE_FUSED_BIAS_GRAD",     off_if_0,     1,   once,     -, "bias gradients by separate column-sum passes") \
  X(fused_ln_bwd,       "HAMSPINE_FUSED_LN_BWD",        off_if_0,     1,   once,     -, "separate LayerNorm-backward / dropout / column-sum passes") \
  X(grouped_wgrad,      "HAMSPINE_GROUPED_WGRAD",       off_if_0,     1,   once,     -, "the image tower backward launches every weight gradient on its own") \
  X(staged_wgrad,       "HAMSPINE_STAGED_WGRAD",        off_if_0,     1,   once,     -, "with gradient milestones, the grouped weight gradients still run only at the end") \
  X(fused_bn_stats,     "HAMSPINE_FUSED_BN_STATS",      off_if_0,     1,   once,     -, "BatchNorm makes its own statistics pass") \
  X(bn_finish,          "HAMSPINE_BN_FINISH",           off_if_0,     1,   once,     -, "BatchNorm finishes its statistics in its own launch") \
  X(fused_bn_bwd,       "HAMSPINE_FUSED_BN_BWD",        off_if_0,     1,   once,     -, "BatchNorm backward makes its own partial-sum pass") \
  X(bnb_finish,         "HAMSPINE_BNB_FINISH",          on_if_1,      0,   once,     -, "the data-gradient GEMM also finishes the BatchNorm-backward sums (measured: no gain)") \
  X(bn_mask_from_x,     "HAMSPINE_BN_MASK_FROM_X",      on_if_1,      0,   once,     -, "inner-stage BatchNorm backward recomputes the ReLU mask from the convolution output (measured neutral)") \
  X(pw_stream,          "HAMSPINE_PW_STREAM",           on_if_1,      0,   once,     -, "1x1 convolutions of a training step through the streaming kernel (measured: a wash)") \
  X(xblock_bn,          "HAMSPINE_XBLOCK_BN",           int_any,      1,   per_call, -, "0: no BatchNorm sums across the block boundary; 2: on every eligible block, whatever its size") \
  X(ds_compact,         "HAMSPINE_DS_COMPACT",          off_if_0,     1,   per_call, -, "bf16 downsample data gradients keep the full-size parity-ordered route") \
  X(img_lean,           "HAMSPINE_IMG_LEAN",            int_mask15,   13,  per_call, -, "bit mask of the bf16 image tower's four lean passes (0: the separate launches)")
// Measurement builds only (make EXTRA=-DHS_MEASURE): a release library ignores the variable, sw::knockout() is constexpr 0.
#define HS_SWITCHES_MEASURE(X) \
  X(knockout,           "HAMSPINE_KNOCKOUT",            int_any,      0,   once,     -, "bit mask of launch classes left OUT of the step (results are then garbage)")
// clang-format on

#define HS_SW_once(id, name, rule, d) \
    inline long long id() { static const long long v = rule(getenv(name), d); return v; }
#define HS_SW_per_call(id, name, rule, d) \
    inline long long id() { return rule(getenv(name), d); }
// -1: not read yet.  A setter that runs between a first reader's load and its exchange keeps its value.
#define HS_SW_settable(id, name, rule, d)                                                                   \
    inline std::atomic<int>& id##_cell() { static std::atomic<int> v{-1}; return v; }                        \
    inline void set_##id(int on) { id##_cell().store(on ? 1 : 0, std::memory_order_relaxed); }               \
    inline long long id() {                                                                                  \
        int v = id##_cell().load(std::memory_order_relaxed);                                                 \
        if (v < 0) {                                                                                         \
            const int env = (int)rule(getenv(name), d);                                                      \
            if (id##_cell().compare_exchange_strong(v, env, std::memory_order_relaxed)) v = env;             \
        }                                                                                                    \
        return v;                                                                                            \
    }
#define HS_SW_DEFINE(id, name, rule, d, latch, setter, doc) HS_SW_##latch(id, name, rule, d)

HS_SWITCHES(HS_SW_DEFINE)
#ifdef HS_MEASURE
HS_SWITCHES_MEASURE(HS_SW_DEFINE)
#else
constexpr long long knockout() { return 0; }
#endif

}  // namespace sw
}  // namespace hs
