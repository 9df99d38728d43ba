"""ctypes binding of libhamspine_hip.so, derived from the C ABI declared in include/hamspine.h.

The header is the single source of truth: parse_header() reads its constants, structs and prototypes, and this module
builds the ctypes.Structure classes, the module constants and every entry point's argtypes / restype from that parse.
A new entry point is declared in the header and nowhere else.

The product path has no CPU fallback: if the shared library is missing, or a tensor that reaches a
kernel wrapper is not on the HIP device, we raise.  (The CPU oracle lives under /oracle and is only
used by tests/, bench.py's cpu_baseline leg and __graft_entry__.smoke().)
"""
import collections
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhamspine_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "hamspine.h"))

HS_OK = 0


class HamspineError(RuntimeError):
    pass


# ------------------------------------------------------------------------------------------ the header, parsed
_SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "hs_status": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "float": C.c_float}
_POINTEES = {"void", "char", "double", "uint8_t", "int16_t", "uint16_t", *_SCALARS}

Header = collections.namedtuple("Header", "constants structs prototypes")


def _symbols(text):
    return sorted(set(re.findall(r"\b(hs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))


def _classify(ctype, structs, what):
    """(kind, base type name) of a C type spelled without blanks around '*'; kind is one of 'scalar', 'struct', 'struct*',
    'char*', 'void*' (every other pointer).  Anything else raises."""
    m = re.fullmatch(r"(const )?(struct )?(\w+)((?:\*(?:const)?)*)", ctype)
    if m:
        base, depth = m.group(3), m.group(4).count("*")
        if depth == 0 and not m.group(2):
            if base in _SCALARS:
                return "scalar", base
            if base in structs:
                return "struct", base
        elif depth == 1 and base in structs:
            return "struct*", base
        elif ctype == "const char*":
            return "char*", base
        elif depth and (m.group(2) or base in _POINTEES or base in structs):
            return "void*", base
    raise HamspineError(f"{what}: cannot classify the C type {ctype!r}")


def _declarator(text, what, typed):
    """(C type, name, array length as written or None) of `type name[len]`, or of a further `name[len]` after a comma"""
    m = re.fullmatch((r"(.+?)\b" if typed else "()") + r"(\w+)(?:\[(\w+)\])?", text)
    if not m:
        raise HamspineError(f"{what}: cannot read the declarator {text!r}")
    return m[1].strip(), m[2], m[3]


def parse_header(text):
    """Header(constants, structs, prototypes) of the C ABI declared in `text`:
         constants   {name: int} of every enumerator and every `#define HS_NAME <int>`
         structs     {name: [(field, C type, array length or None), ...]} in declaration order
         prototypes  {name: (return C type, [parameter C types])}
    Strict: a declaration that is not understood raises HamspineError and nothing is skipped."""
    names = _symbols(text)
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(HS_\w+)(.*)$", text, flags=re.M):
        if not re.fullmatch(r"\s+-?\d+\s*", value):
            raise HamspineError(f"#define {name}{value}: not an integer constant")
        constants[name] = int(value)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    text = re.sub(r" ?\* ?", "*", " ".join(text.split()))
    structs, prototypes = {}, {}
    decl = re.compile(r"([^;{}]*)(?:\{([^{}]*)\}([^;{}]*))?;")
    if decl.sub("", text).strip():
        raise HamspineError(f"header: no declaration in {decl.sub('', text).strip()[:80]!r}")
    for m in decl.finditer(text):
        head, body, tail = (s if s is None else s.strip() for s in m.groups())
        what = m[0].strip()[:100]
        proto = re.fullmatch(r"(.+?)\b(hs_\w+) ?\((.*)\)", head)
        alias = re.fullmatch(r"typedef (\w+) (\w+)", head)
        if body is None and proto:
            ret, params = proto[1].strip(), [] if proto[3] == "void" else proto[3].split(",")
            if ret != "void" and _classify(ret, {}, what)[0] not in ("scalar", "char*"):
                raise HamspineError(f"{what}: unsupported return type {ret!r}")
            types = [_declarator(a.strip(), what, True) for a in params]
            if any(n is not None or _classify(t, structs, what)[0] == "struct" for t, _, n in types):
                raise HamspineError(f"{what}: array or by-value struct parameter")
            prototypes[proto[2]] = (ret, [t for t, _, _ in types])
        elif body is None and alias:                         # a scalar alias the type table already knows
            if alias[1] not in _SCALARS or _SCALARS.get(alias[2]) is not _SCALARS[alias[1]]:
                raise HamspineError(f"{what}: typedef the type table does not know")
        elif body is None and re.fullmatch(r"struct \w+", head):
            pass                                             # forward declaration: declares no layout
        elif body is not None and head == "enum" and not tail:
            for e in body.split(","):
                e = re.fullmatch(r"(HS_\w+) = (-?\d+)", e.strip())
                if not e:
                    raise HamspineError(f"{what}: enumerator without an integer value")
                constants[e[1]] = int(e[2])
        elif body is not None and head == "typedef struct " + tail:
            fields = []
            for line in filter(None, (s.strip() for s in body.split(";"))):
                first, *more = (d.strip() for d in line.split(","))
                ctype = _declarator(first, what, True)[0]
                _classify(ctype, structs, what)
                for _, name, length in [_declarator(first, what, True)] + [_declarator(d, what, False) for d in more]:
                    n = None if length is None else int(length) if length.isdigit() else constants.get(length)
                    if length is not None and n is None:
                        raise HamspineError(f"{what}: array length {length!r} is neither a number nor a known #define")
                    fields.append((name, ctype, n))
            structs[tail] = fields
        else:
            raise HamspineError(f"{what}: not a prototype, enum, scalar typedef or `typedef struct hs_x {{ ... }} hs_x`")
    if sorted(prototypes) != names:
        raise HamspineError(f"header: the parsed prototypes and the hs_*( names differ in {set(prototypes) ^ set(names)}")
    return Header(constants, structs, prototypes)


def _ctype(ctype, classes, param):
    kind, base = _classify(ctype, classes, ctype)
    if kind == "scalar":
        return _SCALARS[base]
    if kind == "struct":
        return classes[base]
    if kind == "struct*" and param:
        return C.POINTER(classes[base])
    return C.c_char_p if kind == "char*" else C.c_void_p


def exported_symbols():
    """Names declared in include/hamspine.h (used by the CPU-side ABI test)."""
    return _symbols(open(HEADER_PATH).read())


_header = parse_header(open(HEADER_PATH).read())

# ------------------------------------------------------------------------------------------ structs and constants
# C struct -> Python name, in the numbering of hs_abi_sizeof
_STRUCT_NAMES = {
    "hs_conv_geom": "ConvGeom",
    "hs_gemm_params": "GemmParams",
    "hs_bn_params": "BnParams",
    "hs_bn_bwd_params": "BnBwdParams",
    "hs_attn_desc": "AttnDesc",
    "hs_conv_bn": "ConvBn",
    "hs_resblock_desc": "ResblockDesc",
    "hs_stem_desc": "StemDesc",
    "hs_linear": "Linear",
    "hs_norm": "Norm",
    "hs_bert_layer_desc": "BertLayerDesc",
    "hs_resnet_desc": "ResnetDesc",
    "hs_resnet_plan": "ResnetPlan",
    "hs_bert_desc": "BertDesc",
}
# structs numbered after those (hs_abi_sizeof knows them; abi_structs() keeps listing the descriptor structs above)
_LATER_STRUCT_NAMES = {
    "hs_jpeg_info": "JpegInfo",
}
_ALL_STRUCT_NAMES = {**_STRUCT_NAMES, **_LATER_STRUCT_NAMES}
if set(_header.structs) != set(_ALL_STRUCT_NAMES):
    raise HamspineError(f"{HEADER_PATH}: structs without a Python name, or the reverse: {set(_header.structs) ^ set(_ALL_STRUCT_NAMES)}")
_classes = {}
for _c, _fields in _header.structs.items():
    _classes[_c] = type(_ALL_STRUCT_NAMES[_c], (C.Structure,), {"_fields_": [
        (f, _ctype(t, _classes, False) * n if n else _ctype(t, _classes, False)) for f, t, n in _fields]})
globals().update({_ALL_STRUCT_NAMES[_c]: _cls for _c, _cls in _classes.items()})


def abi_structs():
    """(number for hs_abi_sizeof, ctypes mirror) of every struct of the C ABI"""
    return list(enumerate(_classes[c] for c in _STRUCT_NAMES))


def later_abi_structs():
    """the same for the structs numbered after the descriptor structs (hs_abi_sizeof 14 and up)"""
    return list(enumerate((_classes[c] for c in _LATER_STRUCT_NAMES), start=len(_STRUCT_NAMES)))


def _const(*names):
    return [_header.constants["HS_" + n] for n in names]


if _const("OK") != [HS_OK]:
    raise HamspineError("HS_OK of the header is not 0")
HS_ERR_ARG, HS_ERR_HIP, HS_ERR_UNSUPPORTED = _const("ERR_ARG", "ERR_HIP", "ERR_UNSUPPORTED")
HS_F32, HS_BF16 = _const("F32", "BF16")
A_KC, A_RC, A_CONV, A_DGRAD = _const("A_KC", "A_RC", "A_CONV", "A_DGRAD")
B_KC, B_RC, B_WDGRAD, B_CONV = _const("B_KC", "B_RC", "B_WDGRAD", "B_CONV")
ACT_NONE, ACT_RELU, ACT_GELU = _const("ACT_NONE", "ACT_RELU", "ACT_GELU")
MUL_NONE, MUL_GELU_GRAD, MUL_RELU_MASK = _const("MUL_NONE", "MUL_GELU_GRAD", "MUL_RELU_MASK")
CAST_MAX, ADAM_MAX, MUON_MAX, MUON_PARTIALS = _const("CAST_MAX", "ADAM_MAX", "MUON_MAX", "MUON_PARTIALS")
GRADCLIP_MAX, = _const("GRADCLIP_MAX")
RESNET_MAX_BLOCKS, RESNET_MAX_TAPS, BERT_MAX_LAYERS = _const("RESNET_MAX_BLOCKS", "RESNET_MAX_TAPS", "BERT_MAX_LAYERS")
JPEG_GEOM, JPEG_CHUNK, JPEG_MAX_COMPONENTS = _const("JPEG_GEOM", "JPEG_CHUNK", "JPEG_MAX_COMPONENTS")
# {status: name without HS_JPEG_ERR_} of the JPEG host stage's refusals and of "corrupt"
JPEG_STATUS = {v: k[len("HS_JPEG_ERR_"):] for k, v in _header.constants.items() if k.startswith("HS_JPEG_ERR_")}

# ------------------------------------------------------------------------------------------ the library
_lib = None


def lib():
    """Load the shared library once and type every entry point of the header; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HamspineError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        missing = [n for n in _header.prototypes if not hasattr(l, n)]
        if missing:
            raise HamspineError(f"{LIB_PATH} lacks declared symbols: {missing}")
        for n, (ret, params) in _header.prototypes.items():
            getattr(l, n).restype = None if ret == "void" else _ctype(ret, _classes, True)
            getattr(l, n).argtypes = [_ctype(t, _classes, True) for t in params]
        _lib = l
    return _lib


def check(status, what=""):
    if status != HS_OK:
        msg = lib().hs_last_error().decode("utf-8", "replace")
        raise HamspineError(f"{what} failed (status {status}): {msg}")
