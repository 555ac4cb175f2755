"""ctypes binding of libdcap_hip.so (the C-ABI in include/dcap.h).

The header is the only description of the ABI: at import this module reads it and derives the DC_* constants, one ctypes.Structure
per descriptor struct and the SYMBOLS table from it.  Adding an entry point means editing the header and writing its wrapper in ops.py.

There is NO CPU fallback: if the library is missing, load() raises.  build it with
`python __graft_entry__.py` (hipcc --offload-arch=gfx950).
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libdcap_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dcap.h")


class DcapError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "uint32_t": C.c_uint32}
_POINTEES = set(_SCALARS) | {"void", "uint8_t", "uint16_t", "int32_t"}       # data pointers: all c_void_p
_DECLARATOR = r"\w+(?:\s*\[\s*\w+\s*\])?"
_FIELD = re.compile(r"(?:const\s+)?(\w+)(?:\s*(\*)\s*|\s+)(%s(?:\s*,\s*%s)*)" % (_DECLARATOR, _DECLARATOR))
_ARG = re.compile(r"(const\s+)?(\w+)(?:\s*(\*(?:\s*const\s*\*)?)\s*|\s+)\w+")
_STRUCT = re.compile(r"\s*typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"\s*(const\s+char\s*\*|int|size_t)\s*(dc_\w+)\s*\(([^()]*)\)\s*;")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(DC_\w+)[ \t]+(.*?)[ \t]*$", re.M)


def _ctype(base, stars, structures, where, int_out=False):
    """The ctypes type of `base` behind `stars` pointer levels.  int_out: a prototype's non-const `int*` argument."""
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base in structures:
        return C.POINTER(structures[base])
    if stars == 1 and base == "int" and int_out:         # an int the callee writes: passed with byref(c_int)
        return C.POINTER(C.c_int)
    if stars == 1 and base == "char":
        return C.c_char_p
    if stars == 1 and base in _POINTEES:
        return C.c_void_p
    if stars == 2 and base in _POINTEES:                 # a host array of device pointers
        return C.POINTER(C.c_void_p)
    raise DcapError("dcap.h: unknown type '%s%s' in '%s'" % (base, "*" * stars, where))


def _class_name(c_name):
    """dc_vocab_top1_bf16_desc -> VocabTop1Bf16Desc, dc_reg_segments -> RegSegments."""
    return "".join(w.capitalize() for w in c_name[3:].split("_"))


def parse_header(text):
    """include/dcap.h -> (constants {DC_NAME: int}, structures {C struct name: ctypes.Structure}, symbols {name: (restype, argtypes)}).
    Strict: a define, declaration or prototype it cannot match in full, a type or an array bound it does not know is a DcapError that
    names it -- nothing is skipped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {}
    for name, value in _DEFINE.findall(text):
        if not re.fullmatch(r"-?\d+", value):
            raise DcapError("dcap.h: #define %s: '%s' is not an integer" % (name, value))
        constants[name] = int(value)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)      # the extern "C" braces
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)                      # include guard, includes, the defines read above
    structures, symbols, pos = {}, {}, 0
    while text[pos:].strip():
        m = _STRUCT.match(text, pos)
        if m:
            fields = []
            for decl in filter(None, (s.strip() for s in m.group(1).split(";"))):
                f = _FIELD.fullmatch(decl)
                if not f or (f.group(2) and "," in f.group(3)):
                    raise DcapError("dcap.h: %s: cannot read the declaration '%s'" % (m.group(2), decl))
                ctype = _ctype(f.group(1), len(f.group(2) or ""), structures, "%s: %s" % (m.group(2), decl))
                for declarator in re.split(r"\s*,\s*", f.group(3)):
                    name, _, bound = declarator.rstrip("] ").partition("[")
                    n = bound.strip()
                    if n and not n.isdigit() and n not in constants:
                        raise DcapError("dcap.h: %s: unknown array bound '%s' in '%s'" % (m.group(2), n, decl))
                    fields.append((name.strip(), ctype * int(constants.get(n, n)) if n else ctype))
            structures[m.group(2)] = type(_class_name(m.group(2)), (C.Structure,), {"_fields_": fields})
        else:
            m = _PROTO.match(text, pos)
            if not m:
                raise DcapError("dcap.h: cannot read the declaration that starts '%s'" % " ".join(text[pos:].split())[:80])
            res = {"int": C.c_int, "size_t": C.c_size_t}.get(m.group(1), C.c_char_p)
            args = []
            for arg in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
                a = _ARG.fullmatch(arg.strip())
                if not a:
                    raise DcapError("dcap.h: %s: cannot read the argument '%s'" % (m.group(2), arg.strip()))
                args.append(_ctype(a.group(2), (a.group(3) or "").count("*"), structures, "%s(%s)" % (m.group(2), arg.strip()),
                                   int_out=not a.group(1)))
            symbols[m.group(2)] = (res, args)
        pos = m.end()
    return constants, structures, symbols


# SYMBOLS: name -> (restype, argtypes) of every prototype; STRUCTURES: C name -> Structure, each also a module attribute under its class
# name (dc_gemm_desc -> GemmDesc); every `#define DC_<NAME> <integer>` a module constant <NAME> (DC_ABI_VERSION -> ABI_VERSION)
if not os.path.exists(HEADER_PATH):
    raise DcapError("%s is missing: the bindings are read from it (keep include/ beside the package directory)" % HEADER_PATH)
with open(HEADER_PATH) as _f:
    CONSTANTS, STRUCTURES, SYMBOLS = parse_header(_f.read())
_derived = dict([(name[3:], value) for name, value in CONSTANTS.items()] + [(cls.__name__, cls) for cls in STRUCTURES.values()])
assert len(_derived) == len(CONSTANTS) + len(STRUCTURES) and not set(_derived) & set(globals()), sorted(set(_derived) & set(globals()))
globals().update(_derived)

RPN_TARGETS_MAX_GT = 512     # include/dcap.h, dc_rpn_targets_desc: the box capacity's limit
_lib = None


def load():
    """Load the HIP library (once).  Raises if it has not been built -- no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("DCAP_LIB", LIB_PATH)          # DCAP_LIB: an experiment build of the same library (tools/build_variant.sh)
    if not os.path.exists(path):
        raise DcapError("%s is missing: build it with `python __graft_entry__.py` "
                        "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    # torch first: its wheel bundles the HIP / HSA runtime it was built with, and the library must bind to THAT copy (same soname as the
    # system's /opt/rocm one).  Loaded before torch, the library maps the system runtime, torch then brings its own, and the process
    # holds two HSA runtimes -- the library's launches fail with "no ROCm-capable device is detected" (build() followed by smoke() in one
    # process did exactly that).
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    got = lib.dc_version()
    if got // 100 != ABI_VERSION // 100:                 # descriptor layouts are per major version (include/dcap.h: DC_ABI_VERSION)
        raise DcapError("%s is ABI version %d, these bindings are for %d: rebuild it (python __graft_entry__.py)" % (path, got, ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().dc_last_error()
        raise DcapError("%s failed (code %d): %s" % (what, rc, msg.decode() if msg else ""))
