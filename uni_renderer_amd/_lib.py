"""ctypes binding of ``liburhip.so``, derived at import from the C ABI declared in ``include/ur_kernels.h``.

The header is the one description of the ABI: its prototypes become ``SYMBOLS``, its structs the ``ctypes.Structure``
mirrors (``STRUCTS``, by header name) and its integer ``#define UR_*`` the constants namespace ``ABI``.  A new entry point,
struct or constant is declared in the header and nowhere else; nothing here, and no version number, is edited with it.

There is deliberately no fallback: if the HIP library or the header is missing or the library's ABI does not match the
header, importing the compute path raises.  ``import torch`` must happen before the library is loaded so that the
library's ``libamdhip64.so.7`` dependency resolves to the HIP runtime PyTorch already loaded (same streams, same device
context, same graph capture).
"""
from __future__ import annotations

import ctypes as C
import keyword
import os
import re
from types import SimpleNamespace

import torch  # noqa: F401  (must be imported first, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UR_LIB_PATH", os.path.join(_HERE, "liburhip.so"))  # override = kernel experiments only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ur_kernels.h")


class UrLibraryError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------
# the header reader: not a C parser -- it accepts exactly the shapes ur_kernels.h uses and raises on anything else
# ---------------------------------------------------------------------------------------------
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
_TYPED_POINTEES = ("int32_t", "int64_t")                   # T* parameters that become POINTER(T): host-side out values / tables
_OPAQUE_POINTEES = ("void", "float", "double", "int", "uint32_t", "uint8_t")  # device memory (or a stream handle): c_void_p
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "char*": C.c_char_p}
_DECL = re.compile(r"(\w+)\s*((?:\*\s*)*)(\w*)")           # base type, stars, name -- `const` already removed
_FIELD = re.compile(r"(\*?)\s*(\w+)(?:\s*\[\s*(\d+)\s*\])?")


def _field_type(struct: str, base: str, decl: str):
    m = _FIELD.fullmatch(decl.strip())
    if not m:
        raise UrLibraryError(f"ur_kernels.h: cannot read field `{base} {decl.strip()}` of {struct}")
    star, name, dim = m.groups()
    if keyword.iskeyword(name):
        raise UrLibraryError(f"ur_kernels.h: field `{name}` of {struct} is a Python keyword; rename it")
    if star and not dim and base in _TYPED_POINTEES + _OPAQUE_POINTEES:
        return name, C.c_void_p
    if base == "char" and dim and not star:
        return name, C.c_char * int(dim)
    if base in _SCALARS and not star and not dim:
        return name, _SCALARS[base]
    raise UrLibraryError(f"ur_kernels.h: unsupported type of field `{name}` of {struct}: `{base}{star}{'[' + dim + ']' if dim else ''}`")


def _param_type(fn: str, text: str, structs: dict):
    m = _DECL.fullmatch(text.strip())
    if not m:
        raise UrLibraryError(f"ur_kernels.h: cannot read parameter `{text.strip()}` of {fn}")
    base, stars = m.group(1), m.group(2).count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base in structs:
        return C.POINTER(structs[base])
    if stars == 1 and base in _TYPED_POINTEES:
        return C.POINTER(_SCALARS[base])
    if (stars == 1 and base in _OPAQUE_POINTEES) or (stars == 2 and base == "void"):
        return C.c_void_p
    raise UrLibraryError(f"ur_kernels.h: unsupported type of parameter `{text.strip()}` of {fn}")


def parse_header(text: str):
    """``(constants, structs, symbols)`` of the header ``text``: ``{UR_NAME: int}``, ``{struct name: ctypes.Structure class}``
    and ``{function name: (restype, argtypes)}``.  Raises ``UrLibraryError``, naming the declaration, on whatever is not one
    of the shapes INTEGRATION.md lists (integer ``#define UR_*``; structs of pointers, int32_t / int64_t / int / float and
    ``char[N]``; functions of scalars and pointers returning int, int64_t or ``const char*``) -- it never guesses."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)  # comments first: some run over `\`-continued #define lines
    text = re.sub(r"//[^\n]*", " ", text)
    consts = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$", text, flags=re.M):
        value = value.strip()
        m = re.fullmatch(r"(-?\d+)|\(\s*(-?\d+)\s*\)", value)
        if value and not (name.startswith("UR_") and m):
            raise UrLibraryError(f"ur_kernels.h: `#define {name} {value}` is not an integer UR_* constant")
        if value:  # (no value: the include guard)
            consts[name] = int(m.group(1) or m.group(2))
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r"\bconst\b", " ", text)

    structs = {}

    def struct(m):
        name, body = m.group(1), m.group(2)
        if m.group(3) != name:
            raise UrLibraryError(f"ur_kernels.h: typedef struct {name} is named {m.group(3)}")
        fields = []
        for line in filter(None, (" ".join(ln.replace("*", " *").split()) for ln in body.split(";"))):
            base, _, decls = line.partition(" ")  # `float *p` / `void *q, *k` / `int32_t M, N` / `char label[16]`
            fields += [_field_type(name, base, d) for d in decls.split(",")]
        structs[name] = type(name, (C.Structure,), {"_fields_": fields, "__doc__": f"Mirror of ``{name}`` (include/ur_kernels.h)."})
        return " "

    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r'\bextern\s+"C"\s*\{', " ", text).replace("}", " ")  # what is left: the prototypes, `;`-separated
    symbols = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(int|int64_t|char ?\*) ?(ur_\w+) ?\((.*)\)", decl)
        if not m:
            raise UrLibraryError(f"ur_kernels.h: cannot read the declaration `{decl}`")
        ret, fn, args = m.group(1).replace(" ", ""), m.group(2), m.group(3).strip()
        symbols[fn] = (_RETURNS[ret], [] if args in ("", "void") else [_param_type(fn, a, structs) for a in args.split(",")])
    return consts, structs, symbols


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise UrLibraryError(f"cannot read {HEADER_PATH}: {e}.  The binding is derived from the header; there is no second copy.") from e


_consts, STRUCTS, SYMBOLS = _read_header()  # SYMBOLS: name -> (restype, argtypes) of every function the header declares
ABI = SimpleNamespace(**_consts)           # every integer `#define UR_*`, by its header name
ABI_VERSION = ABI.UR_ABI_VERSION
IGemmDesc, AttnDesc = STRUCTS["ur_igemm_desc"], STRUCTS["ur_attn_desc"]
AttnBwdDesc, TChainDesc = STRUCTS["ur_attn_bwd_desc"], STRUCTS["ur_tchain_desc"]

_lib = None


def load() -> C.CDLL:
    """Load (once) and type the library; raise ``UrLibraryError`` loudly if it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UrLibraryError(
            f"{LIB_PATH} not found: the HIP kernels are not built. Run `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback for the compute path."
        )
    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover - depends on the host
        raise UrLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise UrLibraryError(f"{LIB_PATH} does not export {name}; rebuild it") from e
        fn.restype = res
        fn.argtypes = args
    if lib.ur_abi_version() != ABI_VERSION:
        raise UrLibraryError(f"ABI version mismatch: library {lib.ur_abi_version()} vs include/ur_kernels.h {ABI_VERSION}; rebuild it")
    for name in SYMBOLS:  # every ur_sizeof_X() the header declares, against the struct ur_X it names
        if name.startswith("ur_sizeof_"):
            ctype = STRUCTS.get("ur_" + name[len("ur_sizeof_"):])
            if ctype is None:
                raise UrLibraryError(f"include/ur_kernels.h declares {name}() but no struct ur_{name[len('ur_sizeof_'):]}")
            if getattr(lib, name)() != C.sizeof(ctype):
                raise UrLibraryError(f"descriptor layout mismatch: {name}() = {getattr(lib, name)()} in the library vs "
                                     f"sizeof({ctype.__name__}) = {C.sizeof(ctype)} from include/ur_kernels.h; rebuild it")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        if rc == ABI.UR_E_BADARG:
            msg = "UR_E_BADARG (inconsistent descriptor)"
        elif rc == ABI.UR_E_UNSUPPORTED:
            msg = "UR_E_UNSUPPORTED (shape not instantiated)"
        else:
            msg = f"hipError {-rc}"
        raise RuntimeError(f"{what} failed: {msg}")


def desc_arrays(struct, rows, nmax: int, fill) -> list:
    """The descriptor arrays of a multi-tensor entry point over ``rows``: one ctypes array of ``struct`` per ``nmax`` rows,
    after ``fill(desc, row, i)`` has set descriptor ``desc`` from ``rows[i]`` (``i`` counts over all of ``rows``)."""
    arrays = []
    for i in range(0, len(rows), nmax):
        part = rows[i:i + nmax]
        arr = (struct * len(part))()
        for k, row in enumerate(part):
            fill(arr[k], row, i + k)
        arrays.append(arr)
    return arrays


def launch_chunked(fn_name: str, struct, rows, nmax: int, fill, *tail) -> None:
    """``lib.fn_name(descs, n, *tail)`` once per ``nmax`` rows (``desc_arrays``), each call checked."""
    fn = getattr(load(), fn_name)
    for arr in desc_arrays(struct, rows, nmax, fill):
        check(fn(arr, len(arr), *tail), fn_name)
