"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/gsrast.h declares (no compute
calls: there is no GPU here). Also the host-side error behaviour of the drop-in Python interface."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z_0-9]+)\s*\(", src)))


def test_library_builds_and_exports_header_symbols(built_lib):
    from dreamscene_amd import _lib
    names = _declared_functions()
    assert "gsr_forward_project" in names and "gsr_backward" in names and len(names) >= 14
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in gsrast.h but not exported by libgsrast.so"
    bound = {n for n, _, _ in _lib.SYMBOLS}
    assert set(names) == bound, f"ctypes binding and header disagree: {set(names) ^ bound}"


def test_ctypes_signatures_have_the_header_s_parameter_counts():
    """A binding with one argument too few still calls -- with the stream in the wrong slot (it happened: gsr_rowmsg_apply_slices
    gained `touched` in the header and not in _lib.SYMBOLS, and the first call crashed the process)."""
    from dreamscene_amd import _lib
    src = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = {}
    for name, args in re.findall(r"\b(gsr_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        args = " ".join(args.split())
        decl[name] = 0 if args in ("", "void") else args.count(",") + 1
    for name, _, argtypes in _lib.SYMBOLS:
        assert name in decl, name
        assert len(argtypes) == decl[name], f"{name}: {decl[name]} parameters in gsrast.h, {len(argtypes)} in _lib.SYMBOLS"


def test_library_contains_gfx950_code_object(built_lib):
    from dreamscene_amd import _lib
    out = subprocess.run(["strings", "-n", "6", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out
    for k in ("k_preprocess", "k_render_fwd", "k_render_bwd", "k_radix_scatter", "k_emit_pairs", "k_preprocess_bwd"):
        assert k in out, f"kernel {k} missing from the fat binary"


def test_pure_helpers_without_gpu(built_lib):
    lib = built_lib
    assert lib.gsr_version() == 1
    assert lib.gsr_num_tiles(1024, 1024) == 4096 and lib.gsr_num_tiles(70, 90) == 5 * 6
    assert lib.gsr_num_blocks(1) == 1 and lib.gsr_num_blocks(257) == 2
    assert lib.gsr_sort_scratch_bytes(0, 16) > 0
    assert lib.gsr_sort_scratch_bytes(3_000_000, 4096) >= 3 * 4 * 3_000_000
    assert lib.gsr_project_scratch_bytes(500_000) >= 4 * 4 * 500_000
    assert b"invalid argument" in lib.gsr_strerror(-1)
    # argument validation happens before any HIP call: NULL view -> EINVAL
    assert lib.gsr_forward_project(None, None, None, None, None, None) == -1
    assert lib.gsr_backward(None, None, None, None, None, None, None, None, None) == -1


def test_project_batch_rejects_several_views_beyond_256_tiles_before_touching_anything(built_lib):
    """gsr_forward_project_batch, n_views = 2, a 40 x 4100 view (257 tile columns: the general binning path, which shares no
    launches between views): GSR_EINVAL from the argument checks -- the caller's count words are as it left them and nothing
    was enqueued. Every OTHER argument is valid (aligned, non-NULL, equally spaced scratch buffers of the size the library
    asks for), so only the grid can be what it objects to; the buffers are host memory and the stream is a made-up handle,
    which a library that went on to K1 could not survive quietly: before the check moved in front of K1 this call zeroed the
    words, armed them with GSR_N_PENDING and launched."""
    import numpy as np
    from dreamscene_amd import _lib
    lib = built_lib
    P, K, V = 300, 4, 2
    sb = int(lib.gsr_project_scratch_bytes(P))
    stride = (sb + 255) // 256 * 256
    sizes = dict(means3D=P * 12, opacities=P * 4, shs=P * K * 12, scales=P * 12, rotations=P * 16, cam=64 * 4,
                 splat=V * P * 48, radii=V * P * 4, tiles=V * P * 4, offs=V * (int(lib.gsr_num_blocks(P)) + 8) * 4,
                 scratch=V * stride)
    arena = np.zeros(sum((n + 255) // 256 * 256 for n in sizes.values()) + 256, np.uint8)
    at, ptr = (arena.ctypes.data + 255) // 256 * 256, {}
    for name, n in sizes.items():
        ptr[name] = at
        at += (n + 255) // 256 * 256
    views = (_lib.GsrView * V)()
    gauss = (_lib.GsrGaussians * V)()
    geoms = (_lib.GsrGeom * V)()
    for k in range(V):
        v = views[k]
        v.P, v.sh_stride, v.sh_degree, v.image_height, v.image_width = P, K, 1, 40, 4100
        v.tanfovx, v.tanfovy, v.scale_modifier = 2.3, 0.022, 1.0
        v.bg, v.viewmatrix, v.projmatrix, v.campos = ptr["cam"], ptr["cam"] + 16, ptr["cam"] + 80, ptr["cam"] + 144
        g = gauss[k]
        g.means3D, g.opacities, g.shs, g.scales, g.rotations = (ptr[n] for n in ("means3D", "opacities", "shs", "scales",
                                                                                 "rotations"))
        ge = geoms[k]
        ge.splat, ge.radii, ge.tiles_touched = ptr["splat"] + k * P * 48, ptr["radii"] + k * P * 4, ptr["tiles"] + k * P * 4
        ge.block_offsets = ptr["offs"] + k * (int(lib.gsr_num_blocks(P)) + 8) * 4
        ge.scratch, ge.scratch_bytes = ptr["scratch"] + k * stride, sb
    words = (ctypes.c_uint64 * V)(0x1234, 0x5678)
    made_up_stream = ctypes.c_void_p(0x10)
    rc = lib.gsr_forward_project_batch(V, views, gauss, geoms, ctypes.addressof(words), made_up_stream, None)
    assert rc == -1, rc                                            # GSR_EINVAL
    assert list(words) == [0x1234, 0x5678], [hex(w) for w in words]
    assert geoms[0].sorted_idx is None and geoms[1].sorted_idx is None


def _header_code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrast.h")).read(), flags=re.S)


def _binding_structs():
    from dreamscene_amd import _lib
    return {n: t for n, t in vars(_lib).items() if isinstance(t, type) and issubclass(t, ctypes.Structure)}


def _binding_constants():
    from dreamscene_amd import _lib
    return {n: v for n, v in vars(_lib).items() if n.startswith("GSR_") and isinstance(v, int)}


@functools.lru_cache(maxsize=None)
def _compiler_view():
    """What gcc makes of gsrast.h for every struct, field and constant the binding has: one generated C program (a name the
    binding misread does not compile). -> ({struct: sizeof}, {(struct, field): (offsetof, sizeof)}, {constant: value})"""
    lines = []
    for s, t in _binding_structs().items():
        lines.append(f'printf("S {s} %zu\\n", sizeof({s}));')
        lines += [f'printf("F {s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f, _ in t._fields_]
    for c in _binding_constants():
        lines.append(f'printf("C {c} %llu\\n", (unsigned long long){c});' if c == "GSR_N_PENDING" else
                     f'printf("C {c} %lld\\n", (long long){c});')
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gsrast.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe], text=True)
    sizes, fields, consts = {}, {}, {}
    for kind, *w in (ln.split() for ln in out.splitlines()):
        if kind == "S":
            sizes[w[0]] = int(w[1])
        elif kind == "F":
            fields[w[0], w[1]] = (int(w[2]), int(w[3]))
        else:
            consts[w[0]] = int(w[1])
    return sizes, fields, consts


def test_struct_layouts_match_header(built_lib):
    """Every ctypes structure of the binding has the size the C compiler gives the header's struct, and every field of it the
    compiler's offset and size. The set of structs is the one a cruder reading of the header finds (none dropped)."""
    structs = _binding_structs()
    assert set(structs) == set(re.findall(r"typedef\s+struct\s+(\w+)\s*\{", _header_code())) and len(structs) == 22
    sizes, fields, _ = _compiler_view()
    assert sizes == {s: ctypes.sizeof(t) for s, t in structs.items()}
    mine = {(s, f): (getattr(t, f).offset, getattr(t, f).size) for s, t in structs.items() for f, _ in t._fields_}
    assert fields == mine, {k: (fields[k], mine[k]) for k in mine if fields[k] != mine[k]}


def test_constants_match_header(built_lib):
    """Every GSR_* #define and enumerator of the binding has the value the C compiler gives it, and the binding has every
    GSR_* name that stands in the header's code (none dropped)."""
    mine = _binding_constants()
    assert set(mine) == set(re.findall(r"\bGSR_[A-Z0-9_]+\b", _header_code())) and len(mine) == 46
    assert _compiler_view()[2] == mine
    assert mine["GSR_N_PENDING"] == 2 ** 64 - 1 and mine["GSR_ESCRATCH"] == -4 and mine["GSR_NOISE_SHS"] == 2


def test_derived_name_lists_follow_the_enums():
    from dreamscene_amd import _lib
    assert len(_lib.STAGES) == _lib.GSR_STAGE_COUNT and _lib.STAGES.index("render_bwd") == _lib.GSR_STAGE_RENDER_BWD
    assert _lib.STAGES[0] == "preprocess" and "count" not in _lib.STAGES
    assert _lib.GSR_DENSIFY_NAMES[_lib.GSR_DENSIFY_SCALING] == "scaling"
    assert len(_lib.GSR_DENSIFY_NAMES) == _lib.GSR_DENSIFY_TENSORS
    assert (_lib.GSR_OK, _lib.GSR_EINVAL, _lib.GSR_ECAPACITY, _lib.GSR_EHIP, _lib.GSR_ESCRATCH) == (0, -1, -2, -3, -4)


# every construct of gsrast.h's grammar, small; %s takes what a case adds
_TINY_HEADER = '''/* tiny.h -- a comment with a ; and a { in it */
#ifndef TINY_H
#define TINY_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_N 3 /* trailing comment */
#define GSR_FLAG 2u
#define GSR_BIG UINT64_MAX
enum {
  GSR_A = -1, /* explicit */
  GSR_B,
  GSR_C = 5, GSR_D
};
enum { GSR_KIND_X, GSR_KIND_Y, GSR_KIND_COUNT };
typedef struct GsrHandle GsrHandle;
typedef struct GsrIn {
  int32_t P, N;          /* several declarators */
  float *a, *b;
  const float* c;   uint8_t* d;    /* two declarations on one line */
  float m1[9], m2[GSR_N];
} GsrIn;
typedef struct GsrOut { GsrIn in[GSR_N]; const GsrIn* ref; const void* p[2]; uint64_t seed; double y; size_t n; } GsrOut;
%s
GsrHandle* gsr_open(void);
void gsr_close(GsrHandle*);
const char* gsr_name(int code);
size_t gsr_bytes(int32_t n, uint32_t m);
int gsr_run(const GsrIn* in, GsrOut* out /* [n] */, double* ms, uint64_t n, float f, const uint8_t* mask,
            void* stream, GsrHandle* h);
#ifdef __cplusplus
}
#endif
#endif /* TINY_H */
'''


def test_parser_reads_every_construct_of_the_grammar():
    from dreamscene_amd._lib import parse_header
    c = ctypes
    abi = parse_header(_TINY_HEADER % "", {("gsr_run", "ms"): c.POINTER(c.c_double)})
    assert abi.constants == dict(GSR_N=3, GSR_FLAG=2, GSR_BIG=2 ** 64 - 1, GSR_A=-1, GSR_B=0, GSR_C=5, GSR_D=6,
                                 GSR_KIND_X=0, GSR_KIND_Y=1, GSR_KIND_COUNT=2)
    assert abi.enums == [dict(GSR_A=-1, GSR_B=0, GSR_C=5, GSR_D=6), dict(GSR_KIND_X=0, GSR_KIND_Y=1, GSR_KIND_COUNT=2)]
    assert list(abi.structs) == ["GsrIn", "GsrOut"]
    In, Out = abi.structs["GsrIn"], abi.structs["GsrOut"]
    assert issubclass(In, c.Structure) and In.__name__ == "GsrIn"
    assert In._fields_ == [("P", c.c_int32), ("N", c.c_int32), ("a", c.c_void_p), ("b", c.c_void_p), ("c", c.c_void_p),
                           ("d", c.c_void_p), ("m1", c.c_float * 9), ("m2", c.c_float * 3)]
    assert Out._fields_ == [("in", In * 3), ("ref", c.POINTER(In)), ("p", c.c_void_p * 2), ("seed", c.c_uint64),
                            ("y", c.c_double), ("n", c.c_size_t)]
    assert abi.symbols == [
        ("gsr_open", c.c_void_p, []),
        ("gsr_close", None, [c.c_void_p]),
        ("gsr_name", c.c_char_p, [c.c_int]),
        ("gsr_bytes", c.c_size_t, [c.c_int32, c.c_uint32]),
        ("gsr_run", c.c_int, [c.POINTER(In), c.POINTER(Out), c.POINTER(c.c_double), c.c_uint64, c.c_float, c.c_void_p,
                              c.c_void_p, c.c_void_p])]
    # without the exception the host pointer is a plain address like every other pointer
    assert parse_header(_TINY_HEADER % "").symbols[4][2][2] is c.c_void_p


@pytest.mark.parametrize("extra, quoted", [
    ("typedef struct GsrCb { int32_t n; void (*cb)(int); } GsrCb;", "void (*cb)(int)"),       # function-pointer field
    ("typedef struct GsrBits { int32_t a : 3; } GsrBits;", "int32_t a : 3"),                   # bit-field
    ("typedef struct GsrU { int32_t n; foo_t x; } GsrU;", "foo_t"),                            # unknown type
    ("typedef struct GsrArr { float m[GSR_NOPE]; } GsrArr;", "GSR_NOPE"),                      # undefined array size
    ("int gsr_count = 3;", "int gsr_count = 3;"),                                              # stray statement
    ("typedef struct GsrEarly { const GsrLate* p; } GsrEarly;\ntypedef struct GsrLate { int32_t n; } GsrLate;", "GsrLate"),
    ("int gsr_arr(float center[3]);", "float center[3]"),                                      # array parameter
    ("#define GSR_HALF 0.5", "GSR_HALF"),                                                      # not an integer
    ("static int gsr_hidden(void);", "static"),                                                # a word left over
    ("#define GSR_N 4", "GSR_N"),                                                              # defined twice
], ids=["function_pointer", "bit_field", "unknown_type", "undefined_array_size", "stray_statement", "struct_before_definition",
        "array_parameter", "non_integer_define", "leftover_word", "defined_twice"])
def test_parser_refuses_what_it_does_not_recognise(extra, quoted):
    """The same header with one thing outside the grammar: GsrError, and the message quotes the offending text."""
    from dreamscene_amd._lib import GsrError, parse_header
    with pytest.raises(GsrError) as e:
        parse_header(_TINY_HEADER % extra)
    assert quoted in str(e.value), str(e.value)


@pytest.mark.parametrize("key", [("gsr_nope", "ms"), ("gsr_run", "nope")], ids=["no_such_function", "no_such_parameter"])
def test_host_pointer_exception_must_name_a_declared_parameter(key):
    from dreamscene_amd._lib import GsrError, parse_header
    with pytest.raises(GsrError) as e:
        parse_header(_TINY_HEADER % "", {key: ctypes.POINTER(ctypes.c_double)})
    assert key[0] in str(e.value) and key[1] in str(e.value)


def _build_c_caller(tmp, with_hip: bool) -> str:
    """tests/c_caller/caller.c: a caller written in plain C against include/gsrast.h (gcc, no Python, no torch)."""
    from dreamscene_amd import _lib
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = os.path.join(tmp, "caller_gpu" if with_hip else "caller")
    cmd = ["gcc", "-O1", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_caller", "caller.c"), "-o", exe, "-L", libdir, "-lgsrast",
           f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lm"]
    if with_hip:
        cmd[1:1] = ["-DWITH_HIP", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
        cmd += ["-lamdhip64"]
    subprocess.check_call(cmd)
    return exe


def test_c_only_caller_without_gpu(built_lib, tmp_path):
    """The boundary is usable from plain C: header compiles as C11, the library links, and the entry points that need
    no device (version, error strings, sizes, argument validation) behave as declared."""
    exe = _build_c_caller(str(tmp_path), with_hip=False)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "C_CALLER_NOGPU_OK" in out.stdout, (out.returncode, out.stdout, out.stderr)


@pytest.mark.gpu
def test_c_only_caller_renders_on_the_gpu(built_lib, tmp_path):
    """A C program (HIP runtime C API for memory, libgsrast.so for everything else) renders 256 Gaussians forward and
    backward on the default stream: no Python / torch anywhere in the process."""
    exe = _build_c_caller(str(tmp_path), with_hip=True)
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "C_CALLER_GPU_OK" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_interface_errors_like_the_reference():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    fields = GaussianRasterizationSettings._fields
    assert fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                      "projmatrix", "sh_degree", "campos", "prefiltered", "score_flag")
    s = GaussianRasterizationSettings(image_height=8, image_width=8, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                      scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                      campos=torch.zeros(3), prefiltered=False, score_flag=False)
    r = GaussianRasterizer(raster_settings=s)
    x = torch.zeros(4, 3)
    with pytest.raises(Exception):       # neither shs nor colors
        r(means3D=x, means2D=x, opacities=torch.zeros(4, 1), scales=x, rotations=torch.zeros(4, 4))
    with pytest.raises(Exception):       # both cov3D and scales
        r(means3D=x, means2D=x, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 1, 3), scales=x,
          rotations=torch.zeros(4, 4), cov3D_precomp=torch.zeros(4, 6))
    # CPU tensors: the product path refuses loudly (no CPU fallback)
    from dreamscene_amd._lib import GsrError
    with pytest.raises(GsrError):
        r(means3D=x, means2D=x, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 1, 3), scales=x,
          rotations=torch.zeros(4, 4))


def test_product_path_does_not_import_the_oracle():
    """oracle/ is test infrastructure: nothing under dreamscene_amd/ or diff_gaussian_rasterization/ may import it."""
    for pkg in ("dreamscene_amd", "diff_gaussian_rasterization"):
        for dp, _, fs in os.walk(os.path.join(ROOT, pkg)):
            for f in fs:
                txt = open(os.path.join(dp, f), errors="ignore").read() if f.endswith((".py", ".hip", ".h")) else ""
                if f.endswith(".py"):
                    assert not re.search(r"^\s*(import|from)\s+oracle\b", txt, flags=re.M), f
                    assert "libgsr_oracle" not in txt and "c_oracle" not in txt and "torch_oracle" not in txt, f
                elif txt:
                    assert not re.search(r"#\s*include.*oracle", txt), f
