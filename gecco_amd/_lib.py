"""ctypes binding of libgecco_hip.so, read from include/gecco_hip.h: the header is the one statement of the C ABI.

`parse_header()` turns the header's `typedef struct`s, prototypes and integer `#define`s into ctypes classes, `SIGNATURES`
and `CONSTANTS` at import (the library need not exist yet).  It accepts the style the header is written in and nothing else:
`typedef struct Name { fields } Name;` with flat fields, and `type gecco_name(named parameters);`.  `load()` fails loudly
when the library is absent — the product path never falls back to a CPU or eager-PyTorch implementation.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GECCO_HIP_LIB") or os.path.join(_HERE, "libgecco_hip.so")   # override: A/B builds only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gecco_hip.h")

c_f = C.c_void_p  # device pointers travel as void*
PP = C.POINTER(C.c_void_p)  # T* const*: a host array of device pointers


class GeccoHipError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double,
            "uint64_t": C.c_uint64, "long long": C.c_longlong, "uint8_t": C.c_uint8, "int32_t": C.c_int32, "int64_t": C.c_int64}
_BLANK = lambda m: "\n" * m.group().count("\n")  # noqa: E731  (erase, keeping the line numbers)
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(GECCO_\w+)[ \t]+\(?[ \t]*(\d+)[ \t]*(?:<<[ \t]*(\d+))?[ \t]*\)?[ \t]*$", re.M)   # n, (n), (n << s)
_STATEMENT = re.compile(r"\s*(?:typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)|([^;{}()]+?)\b(gecco_\w+)\s*\(([^;{}()]*)\))\s*;")
_DECL = re.compile(r"(.*?)\s*(\**)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?", re.S)   # [type] [*]name[[n]]


def parse_header(text: str):
    """-> (structs, signatures, constants) of a header in gecco_hip.h's style; GeccoHipError names the line of anything else."""
    structs, signatures = {}, {}

    def fail(pos, what):
        pos += len(text[pos:]) - len(text[pos:].lstrip())
        raise GeccoHipError(f"gecco_hip.h line {text.count(chr(10), 0, pos) + 1}: cannot bind {what}")

    def ctype(spec, pos):
        words = spec.replace("*", " * ").split()
        stars, base = words.count("*"), " ".join(w for w in words if w not in ("const", "*"))
        pointee = base in _SCALARS or base == "void"
        if stars == 0 and (base in _SCALARS or base in structs):
            return _SCALARS.get(base) or structs[base]
        if stars == 1 and base == "char":
            return C.c_char_p
        if stars == 1 and base in structs:
            return C.POINTER(structs[base])
        if stars == 1 and pointee and words[-1] == "*":
            return C.c_void_p
        if stars == 2 and pointee and words[-3:] == ["*", "const", "*"]:
            return PP
        fail(pos, f"type `{' '.join(words)}`")

    def declarations(body, pos, sep):
        """(name, ctype) of every declarator in `body`: `type declarator` pieces split by `sep`, comma declarators if sep is `;`."""
        out = []
        for piece in body.split(sep):
            base = None
            for d in piece.split(",") if sep == ";" else [piece]:
                m = _DECL.fullmatch(d.strip())
                if not m or bool(m.group(1)) == (base is not None):
                    fail(pos, f"declaration `{' '.join(piece.split())}`")
                base = base or m.group(1)
                t = ctype(base + m.group(2), pos)
                out.append((m.group(3), t * int(m.group(4)) if m.group(4) else t))
            pos += len(piece) + 1
        return out

    text = re.sub(r"/\*.*?\*/|//[^\n]*", _BLANK, text, flags=re.S)
    constants = {name: int(n) << int(shift or 0) for name, n, shift in _DEFINE.findall(text)}
    text = re.sub(r"^[ \t]*#[ \t]*ifdef __cplusplus.*?#[ \t]*endif|^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", _BLANK, text, flags=re.S | re.M).rstrip()
    pos = 0
    while pos < len(text):
        m = _STATEMENT.match(text, pos)
        if not m:
            fail(pos, "this statement")
        tag, body, name, restype, fn, params = m.groups()
        if tag:
            if tag != name:
                fail(m.start(1), f"struct {tag} under the name {name}")
            structs[name] = type(name, (C.Structure,), {"_fields_": declarations(body.rstrip().removesuffix(";"), m.start(2), ";")})
        else:
            args = [] if params.strip() == "void" else [t for _, t in declarations(params, m.start(6), ",")]
            signatures[fn] = (ctype(restype, m.start(4)), args)
        pos = m.end()
    return structs, signatures, constants


if not os.path.exists(HEADER_PATH):
    raise GeccoHipError(f"{HEADER_PATH} not found: the binding is read from the C header that ships beside the package.")
with open(HEADER_PATH) as _f:
    _structs, SIGNATURES, CONSTANTS = parse_header(_f.read())   # name -> (restype, argtypes); name -> int
globals().update(_structs)   # GeccoAdaGN ... GeccoAdamEma, one class per typedef struct
ABI_VERSION = CONSTANTS["GECCO_ABI_VERSION"]

_lib = None


def load() -> C.CDLL:
    """dlopen the library (after torch, so its libamdhip64.so.7 dependency resolves to the HIP
    runtime torch already loaded) and bind every declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GeccoHipError(
            f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
            "gecco_amd has no CPU fallback.")
    import torch  # noqa: F401  (loads the HIP runtime first)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.gecco_abi_version() != ABI_VERSION:
        raise GeccoHipError(f"ABI mismatch: library {lib.gecco_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().gecco_last_error().decode()
        raise GeccoHipError(f"{what} failed with code {rc}: {msg}")
