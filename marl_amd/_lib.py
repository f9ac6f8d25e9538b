"""ctypes binding of libmarl_hip.so.  The C ABI is declared ONCE, in include/marl_hip.h: the struct classes and the
SIGNATURES table are read from that header at import, by a reader that knows the header's grammar and raises on anything else.

The product path has NO fallback: if the shared library is missing or a kernel returns an
error, this module raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C marl_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MARL_HIP_LIB") or os.path.join(_HERE, "libmarl_hip.so")   # override: diagnostic builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "marl_hip.h")           # csrc/Makefile compiles against the same file


class MarlHipError(RuntimeError):
    pass


P, I, L, F, U, SZ, D = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_uint, C.c_size_t, C.c_double   # device pointers travel as integers
_SCALARS = {"int": I, "long": L, "unsigned": U, "float": F, "double": D, "size_t": SZ}
_POINTEES = set(_SCALARS) | {"void", "long long"}
_STRUCT = re.compile(r"typedef\s+struct\s*\{([^{}]*)\}\s*(marl_\w+_t)\s*;")
_PROTO = re.compile(r"([\w\s*]+?)\(([^(){};]*)\)\s*;")
_BLANK = lambda m: " " + "\n" * m.group().count("\n")       # line numbers survive the stripping


def parse_header(text):
    """(structs, signatures) of a header in the grammar of include/marl_hip.h.  structs: typedef name -> ctypes.Structure named
    CamelCase of it without _t (marl_src_t -> MarlSrc), for every ``typedef struct { .. } marl_x_t;``.  signatures: name ->
    (restype, argtypes) for every ``marl_*`` prototype.  Scalars by value; pointers as c_void_p, ``const char*`` as c_char_p, to a
    struct of the header as POINTER(struct); returns int, size_t or const char*.  Anything else raises and names its line."""
    text = re.sub(r"/\*.*?\*/", _BLANK, text, flags=re.S)
    text = re.sub(r"^[ \t]*#ifdef __cplusplus\n.*?\n[ \t]*#endif", _BLANK, text, flags=re.S | re.M)      # extern "C" { .. }
    structs, signatures = {}, {}

    def fail(pos, what):
        pos += len(what) - len(what.lstrip())
        raise MarlHipError("marl_hip.h line %d: cannot read %r" % (text.count("\n", 0, pos) + 1, " ".join(what.split())))

    def pieces(pos, body, sep):
        return [(pos + m.start(), m.group()) for m in re.finditer("[^%s]+" % sep, body) if m.group().strip()]

    def declarations(pos, body, sep):
        """every declaration of `body` as (ctypes type, name): 'const float *a, *b' gives two, 'long long* n' one"""
        out = []
        for p, d in pieces(pos, body, sep):
            parts = [re.findall(r"\w+|\*", part) for part in d.split(",")]
            cut = parts[0].index("*") if "*" in parts[0] else len(parts[0]) - 1
            base, parts[0] = " ".join(parts[0][:cut]), parts[0][cut:]
            if re.search(r"[^\w\s*,]", d) or not base or any(not q or q[-1] == "*" or set(q[:-1]) - {"*"} for q in parts):
                fail(p, d)
            const, base = base.startswith("const "), re.sub(r"^const ", "", base)
            for q in parts:
                if len(q) == 1 and not const and base in _SCALARS:
                    out.append((_SCALARS[base], q[0]))
                elif len(q) == 2 and base in structs:
                    out.append((C.POINTER(structs[base]), q[1]))
                elif len(q) == 2 and const and base == "char":
                    out.append((C.c_char_p, q[1]))
                elif len(q) == 2 and base in _POINTEES:
                    out.append((P, q[1]))
                else:
                    fail(p, d)
        return out

    for p, line in pieces(0, text, "\n"):
        if line.lstrip().startswith("#"):
            if line.rstrip().endswith("\\"):
                fail(p, line)
            text = text[:p] + " " * len(line) + text[p + len(line):]
    pos = 0
    while text[pos:].strip():
        pos += len(text[pos:]) - len(text[pos:].lstrip())
        st, fn = _STRUCT.match(text, pos), _PROTO.match(text, pos)
        if st and st.group(2) not in structs:
            name = "".join(w.capitalize() for w in st.group(2)[:-2].split("_"))
            structs[st.group(2)] = type(name, (C.Structure,), {"_fields_": [(n, t) for t, n in declarations(st.start(1), st.group(1), ";")]})
        elif fn:
            head = declarations(pos, fn.group(1), ";")
            if len(head) != 1 or not re.fullmatch(r"marl_[a-z0-9_]+", head[0][1]) or head[0][1] in signatures or head[0][0] not in (I, SZ, C.c_char_p):
                fail(pos, fn.group(1))
            args = [] if fn.group(2).strip() == "void" else pieces(fn.start(2), fn.group(2), ",")
            signatures[head[0][1]] = (head[0][0], [declarations(p, d, ",")[0][0] for p, d in args])
        else:
            fail(pos, text[pos:].split("\n", 1)[0])
        pos = (fn or st).end()
    return structs, signatures


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise MarlHipError("include/marl_hip.h not found at %s: the ctypes tables are read from it, so marl_amd runs from its "
                           "source tree, beside include/" % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# STRUCTS: typedef name -> ctypes.Structure, also module attributes under their class names (MarlSrc, MarlAgentWeights, ..);
# SIGNATURES: name -> (restype, argtypes) of every function of the header
STRUCTS, SIGNATURES = _read_header()
globals().update({cls.__name__: cls for cls in STRUCTS.values()})

_lib = None


def load():
    """Load the shared library (once).  Raises if it has not been built - never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MarlHipError(
            "libmarl_hip.so not found at %s - the HIP hot path is mandatory (no CPU fallback). "
            "Build it with `python -c \"import __graft_entry__ as g; g.build()\"`." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    from . import experiments
    experiments.apply(lib)          # the MARL_* environment, read ONCE at import of marl_amd.experiments, goes into the library's table
    return lib


def check(code, what):
    if code != 0:
        raise MarlHipError("%s failed with hipError_t %d" % (what, code))
