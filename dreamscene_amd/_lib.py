"""ctypes binding of libgsrast.so, derived from the C ABI in include/gsrast.h: the structures, the constants and the
signatures below are read from the header at import, nothing of it is restated here. Fails loudly when the HIP library
is missing or does not export the declared symbols: there is NO CPU / PyTorch fallback in the product path."""
from __future__ import annotations

import ctypes as C
import os
import re
from types import SimpleNamespace

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSR_LIB: an experimental build of the same library (dreamscene_amd/build.py, A/B measurements); default: the product
LIB_PATH = os.environ.get("GSR_LIB") or os.path.join(_HERE, "libgsrast.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gsrast.h")


class GsrError(RuntimeError):
    pass


# ---- the header's grammar, and nothing else: whatever parse_header() does not recognise is an error ------------------------------
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "uint8_t": C.c_uint8, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_ITEM = re.compile(r"""
    ^[ \t]*\#define[ \t]+(?P<define>GSR_\w+)[ \t]+(?P<value>\S+)[ \t]*$
  | \benum\s*\{(?P<enum>[^{};]*)\}\s*;
  | \btypedef\s+struct\s+(?P<opaque>\w+)\s+(?P=opaque)\s*;
  | \btypedef\s+struct\s+(?P<struct>\w+)\s*\{(?P<fields>[^{}]*)\}\s*(?P=struct)\s*;
  | \b(?P<ret>(?:const\s+)?\w+\s*\*?)\s*\b(?P<fn>gsr_\w+)\s*\((?P<params>[^(){};]*)\)\s*;
""", re.M | re.X)
_DECL = re.compile(r"(?:const\s+)?(\w+)\b(.*)", re.S)                        # base type, declarators
_DECLARATOR = re.compile(r"\s*(\*?)\s*(\w+)?\s*(?:\[\s*(\w+)\s*\])?\s*")     # [*] [name] [[size]]
_PREAMBLE = re.compile(r'#ifndef (\w+) #define \1 (?:#include <[\w./]+> )*#ifdef __cplusplus extern "C" \{ #endif '
                       r'#ifdef __cplusplus \} #endif #endif')


def parse_header(text: str, host_pointers: dict | None = None) -> SimpleNamespace:
    """The ABI a header in gsrast.h's grammar declares, as ctypes: .constants {name: int} (#defines and enumerators), .enums
    [{name: int}] (one per enum), .structs {name: Structure subclass}, .symbols [(name, restype, argtypes)]. A pointer to a Gsr
    struct becomes POINTER(struct), any other pointer c_void_p (device pointers travel as integers) -- except the parameters
    host_pointers {(function, parameter): ctypes type} names. A pure function of its arguments."""
    abi = SimpleNamespace(constants={}, enums=[], structs={}, symbols=[], opaque=set())
    pending = dict(host_pointers or {})

    def const(name, value):
        if name in abi.constants:
            raise GsrError(f"gsrast.h: {name} is defined twice")
        abi.constants[name] = value

    def ctype(decl, base, star, size):
        if base in abi.structs:
            t, pointer = abi.structs[base], C.POINTER(abi.structs[base])
        elif base in _SCALARS:
            t, pointer = _SCALARS[base], C.c_void_p
        elif base in ("void", "char") or base in abi.opaque:
            t, pointer = None, C.c_void_p
        else:
            raise GsrError(f"gsrast.h: unknown type {base!r} in {decl!r}")
        t = pointer if star else t
        if t is None:
            raise GsrError(f"gsrast.h: {base!r} by value in {decl!r}")
        if size is not None:
            n = int(size) if size.isdigit() else abi.constants.get(size)
            if n is None:
                raise GsrError(f"gsrast.h: unknown array size {size!r} in {decl!r}")
            t = t * n
        return t

    def declarations(decl, named):
        """(name, ctypes type) of every declarator of `float *a, *b`, `float m1[9], m2[25]`, `const GsrView* views`, `GsrProfile*`.
        named: a struct's fields (a name each, arrays allowed); else a parameter or a return type (no arrays)."""
        decl = " ".join(decl.split())
        head = _DECL.fullmatch(decl)
        for d in head.group(2).split(",") if head else [""]:
            m = _DECLARATOR.fullmatch(d)
            if not head or not m or (not m.group(2) if named else m.group(3)):
                raise GsrError(f"gsrast.h: cannot read the declaration {decl!r}")
            yield m.group(2), ctype(decl, head.group(1), m.group(1), m.group(3))

    def item(m):
        if m["define"]:
            lit = re.fullmatch(r"(\d+)u?", m["value"])
            if not lit and m["value"] != "UINT64_MAX":
                raise GsrError(f"gsrast.h: cannot read the value of {m[0].strip()!r}")
            const(m["define"], int(lit.group(1)) if lit else 2 ** 64 - 1)
        elif m["enum"] is not None:
            block, value = {}, -1
            for e in m["enum"].split(","):
                em = re.fullmatch(r"\s*(\w+)\s*(?:=\s*(-?\d+)\s*)?", e)
                if not em:
                    raise GsrError(f"gsrast.h: cannot read the enumerator {e.strip()!r}")
                value = int(em.group(2)) if em.group(2) else value + 1
                const(em.group(1), value)
                block[em.group(1)] = value
            abi.enums.append(block)
        elif m["opaque"]:
            abi.opaque.add(m["opaque"])
        elif m["struct"]:
            fields = [f for d in m["fields"].split(";") if d.strip() for f in declarations(d, named=True)]
            abi.structs[m["struct"]] = type(m["struct"], (C.Structure,), {"_fields_": fields})
        else:
            ret, params = " ".join(m["ret"].split()), m["params"].strip()
            restype = None if ret == "void" else C.c_char_p if ret == "const char*" else next(declarations(ret, named=False))[1]
            args = [a for p in params.split(",") for a in declarations(p, named=False)] if params not in ("", "void") else []
            abi.symbols.append((m["fn"], restype, [pending.pop((m["fn"], name), t) for name, t in args]))
        return ""

    rest = [ln.strip() for ln in _ITEM.sub(item, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)).splitlines() if ln.strip()]
    if not _PREAMBLE.fullmatch(" ".join(" ".join(rest).split())):
        stray = [ln for ln in rest if not re.fullmatch(r'#(ifndef|define|ifdef|endif|include)\b[^;]*|extern "C" \{|\}', ln)]
        raise GsrError("gsrast.h: not understood: " + " | ".join(stray or rest))
    if pending:
        raise GsrError(f"gsrast.h declares no such function / parameter: {sorted(pending)}")
    return abi


# The one thing the header cannot say: these parameters point to HOST memory. They keep their element type, and ctypes
# then refuses anything but a pointer to, or an array of, that type.
_HOST_POINTERS = {
    ("gsr_profile_collect", "ms"): C.POINTER(C.c_double),
    ("gsr_profile_collect", "counts"): C.POINTER(C.c_int64),
    ("gsr_forward_project", "n_pairs_host"): C.POINTER(C.c_uint64),
    ("gsr_pack_views_streams", "streams"): C.POINTER(C.c_uint32),
    ("gsr_photo_window", "taps"): C.POINTER(C.c_float),
    ("gsr_extract_fields", "center"): C.POINTER(C.c_float),
}

with open(HEADER_PATH) as _fh:
    _abi = parse_header(_fh.read(), _HOST_POINTERS)

globals().update(_abi.constants)     # every GSR_* #define and enumerator: GSR_OK .. GSR_ESCRATCH, GSR_MAX_*, GSR_STAGE_*, ...
SYMBOLS = _abi.symbols               # every function the header declares: (name, restype, argtypes)
_S = _abi.structs
GsrView, GsrModel, GsrScene = _S["GsrView"], _S["GsrModel"], _S["GsrScene"]
GsrModelGrads, GsrSceneGrads, GsrGaussians = _S["GsrModelGrads"], _S["GsrSceneGrads"], _S["GsrGaussians"]
GsrGeom, GsrBinning, GsrImages, GsrImageGrads = _S["GsrGeom"], _S["GsrBinning"], _S["GsrImages"], _S["GsrImageGrads"]
GsrGrads, GsrAdamGroup, GsrRowRegion, GsrRowSet = _S["GsrGrads"], _S["GsrAdamGroup"], _S["GsrRowRegion"], _S["GsrRowSet"]
GsrDispViews, GsrPlacement, GsrFrameViews = _S["GsrDispViews"], _S["GsrPlacement"], _S["GsrFrameViews"]
GsrDensifyPlan, GsrDensifyTensor, GsrDensifyTable = _S["GsrDensifyPlan"], _S["GsrDensifyTensor"], _S["GsrDensifyTable"]
GsrPhotoViews, GsrPhotoWeights = _S["GsrPhotoViews"], _S["GsrPhotoWeights"]
if set(_S) - set(globals()):
    raise GsrError(f"{__file__} binds no name to {sorted(set(_S) - set(globals()))} of gsrast.h")


def _enum_names(prefix: str) -> list:
    """The lower-cased suffixes of the enum whose enumerators start with `prefix`, in value order, without COUNT."""
    block, = (e for e in _abi.enums if all(k.startswith(prefix) for k in e))
    return [k[len(prefix):].lower() for k in sorted(block, key=block.get) if k != prefix + "COUNT"]


STAGES = _enum_names("GSR_STAGE_")                    # "preprocess" .. "preprocess_bwd"
GSR_DENSIFY_NAMES = tuple(_enum_names("GSR_DENSIFY_"))  # "xyz" .. "rotation": the order of GsrDensifyTable.t

_lib = None


def load() -> C.CDLL:
    """dlopen the in-tree library and bind every declared entry point. Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: libgsrast.so must share the HIP runtime torch has loaded (its device pointers and streams are
    # only meaningful inside that runtime instance); dlopen resolves libamdhip64 to the already-loaded copy.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise GsrError(f"{LIB_PATH} is missing: build it with `python -m dreamscene_amd.build` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise GsrError(f"{LIB_PATH} does not export {name} (declared in include/gsrast.h)") from e
        fn.restype = res
        fn.argtypes = args
    if lib.gsr_version() != GSR_VERSION:  # noqa: F821 (from the header)
        raise GsrError(f"libgsrast ABI version {lib.gsr_version()} != {GSR_VERSION} of include/gsrast.h")  # noqa: F821
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        lib = load()
        raise GsrError(f"{what} failed: {lib.gsr_strerror(rc).decode()} (code {rc})")


class Profile:
    """Per-stage HIP-event timing (GsrProfile). Use: p = Profile(); ...pass p.handle...; p.collect()."""

    def __init__(self):
        self.lib = load()
        self.handle = self.lib.gsr_profile_create()
        self.ms = (C.c_double * len(STAGES))()
        self.counts = (C.c_int64 * len(STAGES))()

    def set_stages(self, names=None):
        """Record only the named stages (None = all)."""
        mask = 0xFFFFFFFF if names is None else sum(1 << STAGES.index(n) for n in names)
        self.lib.gsr_profile_set_stage_mask(self.handle, mask)

    def set_sampling(self, every: int = 1):
        """Record one of every `every` occurrences of each stage."""
        self.lib.gsr_profile_set_sampling(self.handle, int(every))

    def collect(self) -> dict:
        check(self.lib.gsr_profile_collect(self.handle, self.ms, self.counts), "gsr_profile_collect")
        return {s: (self.ms[i], self.counts[i]) for i, s in enumerate(STAGES)}

    def reset(self):
        self.collect()
        for i in range(len(STAGES)):
            self.ms[i] = 0.0
            self.counts[i] = 0

    def __del__(self):
        try:
            if self.handle:
                self.lib.gsr_profile_destroy(self.handle)
                self.handle = None
        except Exception:
            pass
