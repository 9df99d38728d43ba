"""The ctypes binding is derived from include/hamspine.h: completeness, literal spot checks against the hand table it replaced,
the generated struct mirrors, and the parser's strictness on fabricated header text.  Needs the built library, no GPU."""
import ctypes as C
import re

import pytest

import hamspine._lib as L

i32, i64, u64, f32, vp = C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_void_p


def _header_parameter_counts():
    """{entry point: number of parameters}, counted from the header text by commas, without the parser"""
    text = re.sub(r"/\*.*?\*/", "", open(L.HEADER_PATH).read(), flags=re.S)
    return {name: 0 if args.strip() == "void" else args.count(",") + 1
            for name, args in re.findall(r"\b(hs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}


def test_every_declared_entry_point_is_typed_with_the_headers_parameter_count():
    lib = L.lib()
    names, counts = L.exported_symbols(), _header_parameter_counts()
    assert len(names) == len(L.parse_header(open(L.HEADER_PATH).read()).prototypes) == len(counts) >= 174
    for n in names:
        assert getattr(lib, n).argtypes is not None, n
        assert len(getattr(lib, n).argtypes) == counts[n], (n, counts[n])


def test_spot_checks_against_the_hand_written_table():
    lib, P = L.lib(), C.POINTER
    expected = {
        "hs_selective_scan_bwd": [i32, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, i32,
                                  vp, vp, i32, vp, i32, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp],
        "hs_adam_step_multi": [i32, vp, vp, vp, vp, vp, f32, f32, f32, f32, f32, i32, i32, f32, vp],
        "hs_bert_embed_fwd": [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, f32, f32, u64, vp],
        "hs_gemm": [P(L.GemmParams), vp],
        "hs_resnet_query": [P(L.ResnetDesc), P(L.ResnetPlan)],
        "hs_linear_fwd": [i32, vp, i64, i32, P(L.Linear), vp, vp, i32, i32, i32, vp, vp, i32, f32, u64, vp],
        "hs_prof_collect": [vp, vp, vp],
        "hs_stage_images_u8": [vp, vp, i32, i32, i32, vp, vp, vp],
        "hs_prof_dump": [C.c_char_p],
        "hs_batchnorm_ws_bytes": [i64, i32, i32],
        "hs_version": [],
    }
    assert len(expected["hs_selective_scan_bwd"]) == 35
    for n, types in expected.items():
        assert list(getattr(lib, n).argtypes) == types, n
    assert lib.hs_last_error.restype is C.c_char_p
    assert lib.hs_gemm_splitk_ws_bytes.restype is i64
    assert lib.hs_gemm_tile_rows.restype is i32 and lib.hs_gemm.restype is i32 and lib.hs_version.restype is i32
    assert lib.hs_set_overlap.restype is None
    # what the callers hand a pointer parameter is still accepted, and a float is still refused
    for ok in (None, 4096, vp(4096), (i64 * 2)(), C.byref(i64()), C.pointer(i64()), (vp * 2)()):
        vp.from_param(ok)
    with pytest.raises(TypeError):
        vp.from_param(1.5)
    for ok in (None, L.GemmParams(), C.byref(L.GemmParams())):
        P(L.GemmParams).from_param(ok)


def test_struct_mirrors_follow_the_header():
    names = lambda s: [f for f, _ in s._fields_]
    types = lambda s: dict(s._fields_)
    assert names(L.ConvGeom) == ["N", "H", "W", "C", "P", "Q", "K", "R", "S", "stride", "pad", "row_pitch", "img_pitch", "qstep",
                                 "no_bounds"]
    assert set(types(L.ConvGeom).values()) == {i32}
    assert names(L.ResnetPlan) == ["saved_bytes", "ws_bytes", "tap_offset", "tap_C", "tap_H", "tap_W"]
    assert [t for _, t in L.ResnetPlan._fields_] == [i64, i64, i64 * 4, i32 * 4, i32 * 4, i32 * 4]
    assert names(L.GemmParams)[-8:] == ["bnb_mean", "bnb_invstd", "bnb_partials", "bn_finish", "bnb_y", "bnb_finish", "m_rows",
                                        "drop_rows"]
    assert len(L.GemmParams._fields_) == 56 and {types(L.GemmParams)[f] for f in names(L.GemmParams)[-8:]} == {vp}
    g = types(L.GemmParams)
    assert (g["g"], g["a_elems"], g["alpha"], g["dropout_seed"], g["D_seg"], g["rowsum_seg"]) == (L.ConvGeom, i64, f32, u64, vp * 2, vp * 2)
    assert types(L.ResnetDesc)["blocks"] is L.ResblockDesc * 24 and L.RESNET_MAX_BLOCKS == 24
    assert types(L.ResnetDesc)["tap_block"] is i32 * 4 and L.RESNET_MAX_TAPS == 4
    assert types(L.ResblockDesc)["main"] is L.ConvBn * 3 and types(L.ResblockDesc)["ds"] is L.ConvBn
    assert types(L.BertDesc)["layers"] is L.BertLayerDesc * 24 and L.BERT_MAX_LAYERS == 24
    assert [c.__name__ for _, c in L.abi_structs()] == [
        "ConvGeom", "GemmParams", "BnParams", "BnBwdParams", "AttnDesc", "ConvBn", "ResblockDesc", "StemDesc", "Linear", "Norm",
        "BertLayerDesc", "ResnetDesc", "ResnetPlan", "BertDesc"]
    assert [w for w, _ in L.abi_structs()] == list(range(14))
    assert (L.HS_OK, L.HS_F32, L.HS_BF16, L.A_KC, L.A_RC, L.A_CONV, L.A_DGRAD, L.B_KC, L.B_RC, L.B_WDGRAD, L.B_CONV) == \
        (0, 0, 1, 0, 1, 2, 3, 0, 1, 2, 3)
    assert (L.ACT_NONE, L.ACT_RELU, L.ACT_GELU, L.MUL_NONE, L.MUL_GELU_GRAD, L.MUL_RELU_MASK) == (0, 1, 2, 0, 1, 2)
    assert (L.CAST_MAX, L.ADAM_MAX, L.MUON_MAX, L.MUON_PARTIALS) == (48, 32, 32, 256)


GOOD = """
/* hs_status hs_in_a_comment(int32_t a); */
#define HS_LEN 3
enum { HS_X = 0, HS_Y = 5 };
struct hs_later;
typedef struct hs_pair {
    int32_t a, b[HS_LEN];       // two declarators
    const struct hs_later* next;
    void* seg[2];
} hs_pair;
typedef struct hs_outer { hs_pair p[2]; const float* const* rows; } hs_outer;
hs_status hs_run(const hs_outer* o, hs_pair* p, const float* const* rows, float x, uint64_t seed, void* stream);
void hs_reset(void);
"""


def test_parser_reads_fabricated_text_and_refuses_what_it_cannot_classify():
    h = L.parse_header(GOOD)
    assert h.constants == {"HS_LEN": 3, "HS_X": 0, "HS_Y": 5}
    assert h.structs == {"hs_pair": [("a", "int32_t", None), ("b", "int32_t", 3), ("next", "const struct hs_later*", None),
                                     ("seg", "void*", 2)],
                         "hs_outer": [("p", "hs_pair", 2), ("rows", "const float*const*", None)]}
    assert h.prototypes == {"hs_run": ("hs_status", ["const hs_outer*", "hs_pair*", "const float*const*", "float", "uint64_t", "void*"]),
                            "hs_reset": ("void", [])}
    assert "hs_in_a_comment" not in h.prototypes
    for bad in ("hs_status hs_f(size_t n, void* stream);",             # unknown by-value parameter type
                "hs_status hs_f(hs_unknown* p);",                      # pointer to a type that is declared nowhere
                "hs_status hs_f(hs_pair p);",                          # struct by value
                "typedef struct hs_t { int32_t v[HS_NOT_DEFINED]; } hs_t;",
                "typedef struct hs_t { float *a, *b; } hs_t;",         # a declarator it does not understand
                "typedef struct hs_t { int32_t a; } hs_other;",
                "hs_status hs_f(int32_t a, void* stream;",             # a prototype it cannot split
                "hs_status hs_f(int32_t, void* stream);",              # unnamed parameter
                "hs_status hs_f(int32_t a) { return 0; }",
                "enum { HS_Z };",
                "#define HS_RATE 1.5\n",
                "#define HS_MAX(a, b) ((a) > (b) ? (a) : (b))\n",
                "size_t hs_f(void);",
                "typedef long hs_word;"):
        with pytest.raises(L.HamspineError):
            L.parse_header(GOOD + bad)
