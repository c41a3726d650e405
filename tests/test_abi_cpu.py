"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/*.h declares, and the ctypes binding
(ratrack_amd/abi.py) agrees with the headers: the kind of every argument of every entry point, and every struct's field names, order,
offsets and size as a host C compiler lays them out.  No compute call is made here (there is no GPU in the build container)."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

from ratrack_amd import _lib, abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_COMPUTE = {"rtk_last_error", "rtk_version"}      # bound by _lib.load() itself, with their own restype


def header_code():
    """include/*.h without comments and without the definition of RTK_EXPORT itself: what is left of that word marks a prototype."""
    text = ""
    for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))):
        code = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        code = re.sub(r"//[^\n]*", "", code)
        text += re.sub(r"#define\s+RTK_EXPORT[^\n]*", "", code)
    return text


def c_kind(param):
    """One parameter or field declaration (with its name) -> pointer / int / long / long long / float / double."""
    if "*" in param or "rtk_stream_t" in param:
        return "pointer"
    kind = " ".join(w for w in param.split()[:-1] if w != "const")
    assert kind in ("int", "long", "long long", "float", "double"), "unknown C type in %r" % param
    return kind


def prototypes():
    """{entry point: [kind of every parameter]} for every RTK_EXPORT prototype of the headers; none is skipped."""
    code = header_code()
    found = re.findall(r"RTK_EXPORT\s+[\w\s\*]+?\b(rtk_\w+)\s*\(([^()]*)\)\s*;", code)
    assert found and len(found) == code.count("RTK_EXPORT"), "parsed %d of %d prototypes" % (len(found), code.count("RTK_EXPORT"))
    protos = {name: [] if params.strip() == "void" else [c_kind(p) for p in params.split(",")] for name, params in found}
    assert len(protos) == len(found), "an entry point is declared twice"
    return protos


def declared_symbols():
    return sorted(prototypes())


def struct_fields():
    """{typedef name: [field names, flattened]} for every `typedef struct { ... } name;`: `int B, N;` is two fields, `int *a, *b;` too."""
    code = header_code()
    found = re.findall(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", code)
    assert found and len(found) == len(re.findall(r"typedef\s+struct\b", code)), "parsed %d structs" % len(found)
    fields = {}
    for body, name in found:
        fields[name] = [re.search(r"(\w+)\s*$", piece).group(1) for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    return fields


def host_cc():
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc())))
    for c in (os.environ.get("CC"), "cc", "gcc", "clang", os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang")):
        if c and shutil.which(c):
            return shutil.which(c)
    pytest.fail("no host C compiler (cc, gcc, clang, ROCm's clang): the struct layouts cannot be checked")


def c_layouts(fields, workdir):
    """{typedef name: (sizeof, {field: (offsetof, sizeof the field)})} as the host C compiler lays the headers' structs out."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "rtk_score.h"', '#include "rtk_train.h"', "int main(void) {"]
    for name, names in fields.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f, name, f) for f in names]
    lines += ["    return 0;", "}", ""]
    src, exe = os.path.join(str(workdir), "layout.c"), os.path.join(str(workdir), "layout")
    open(src, "w").write("\n".join(lines))
    subprocess.check_call([host_cc(), "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    sizes, offsets = {}, {name: {} for name in fields}
    for line in subprocess.check_output([exe]).decode().split("\n"):
        if line:
            key, *values = line.split()
            if "." in key:
                offsets[key.split(".")[0]][key.split(".")[1]] = tuple(int(v) for v in values)
            else:
                sizes[key] = int(values[0])
    return {name: (sizes[name], offsets[name]) for name in fields}


# which C kinds a ctypes argtype may stand for.  ctypes makes c_longlong an alias of c_long where the two have one size (LP64), so there
# the class cannot tell `long` from `long long`: it stands for both.
_CTYPES_KINDS = {}
for _t, _k in ((ctypes.c_int, "int"), (ctypes.c_long, "long"), (ctypes.c_longlong, "long long"), (ctypes.c_float, "float"),
               (ctypes.c_double, "double"), (ctypes.c_void_p, "pointer"), (ctypes.c_char_p, "pointer")):
    _CTYPES_KINDS.setdefault(_t, set()).add(_k)


def ctypes_kinds(t):
    return {"pointer"} if issubclass(t, ctypes._Pointer) else _CTYPES_KINDS[t]


def signature_mismatches(protos, table):
    """The entry points of `protos` whose argtypes in `table` are missing or differ from the prototype in count or in the kind of an argument."""
    bad = []
    for name, kinds in protos.items():
        args = table.get(name)
        if args is None or len(args) != len(kinds) or any(k not in ctypes_kinds(a) for k, a in zip(kinds, args)):
            bad.append(name)
    return sorted(bad)


def struct_mismatches(fields, layouts, structs):
    """The structs of `fields` whose mirror in `structs` is missing or differs in field names, their order, the offset or the size of a
    field, or the size of the whole."""
    bad = []
    for name, names in fields.items():
        cls = structs.get(name)
        size, offsets = layouts[name]
        if cls is None or [f[0] for f in cls._fields_] != names or ctypes.sizeof(cls) != size or \
                any((getattr(cls, f).offset, getattr(cls, f).size) != offsets[f] for f in names):
            bad.append(name)
    return sorted(bad)


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    return c_layouts(struct_fields(), tmp_path_factory.mktemp("abi"))


def compute_prototypes():
    protos = prototypes()
    assert NOT_COMPUTE <= set(protos)
    return {n: k for n, k in protos.items() if n not in NOT_COMPUTE}


def test_signatures_agree_with_the_prototypes():
    protos = compute_prototypes()
    assert set(abi.SIGNATURES) == set(protos), set(abi.SIGNATURES) ^ set(protos)
    assert _lib.SIGNATURES is abi.SIGNATURES
    assert signature_mismatches(protos, abi.SIGNATURES) == []


def test_structs_agree_with_the_c_layout(layouts):
    fields = struct_fields()
    assert set(abi.STRUCTS) == set(fields), set(abi.STRUCTS) ^ set(fields)
    assert struct_mismatches(fields, layouts, abi.STRUCTS) == []


def test_the_comparers_report_a_doctored_binding(layouts):
    protos, fields = compute_prototypes(), struct_fields()
    table = {n: list(a) for n, a in abi.SIGNATURES.items()}
    at = table["rtk_ball_query"].index(ctypes.c_int)
    table["rtk_ball_query"][at] = ctypes.c_float                    # one int bound as a float
    assert signature_mismatches(protos, table) == ["rtk_ball_query"]
    table = {n: list(a) for n, a in abi.SIGNATURES.items()}
    del table["rtk_knn"][0]                                         # one argument short
    assert signature_mismatches(protos, table) == ["rtk_knn"]

    class Swapped(ctypes.Structure):                                # rtk_layer_t with cin16 and cout16 transposed: same size, same offsets
        _fields_ = [(n, t) for n, t in abi.Layer._fields_[:2]] + [abi.Layer._fields_[3], abi.Layer._fields_[2]] + list(abi.Layer._fields_[4:])

    class Narrow(ctypes.Structure):                                  # rtk_copy_job_t with a 4-byte `bytes`: names, offsets and the padded size all agree
        _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("bytes", ctypes.c_int)]

    assert struct_mismatches(fields, layouts, dict(abi.STRUCTS, rtk_layer_t=Swapped)) == ["rtk_layer_t"]
    assert struct_mismatches(fields, layouts, dict(abi.STRUCTS, rtk_copy_job_t=Narrow)) == ["rtk_copy_job_t"]
    assert abi.STRUCTS["rtk_layer_t"] is abi.Layer and abi.SIGNATURES["rtk_ball_query"][at] is ctypes.c_int      # the real ones are untouched


def test_header_declares_the_reference_surface():
    names = declared_symbols()
    # one entry per pybind export of the reference (pointnet2_api.cpp:10-25) + knn_point
    for n in ["rtk_ball_query", "rtk_group_points", "rtk_group_points_grad", "rtk_gather_points",
              "rtk_gather_points_grad", "rtk_furthest_point_sampling", "rtk_knn", "rtk_three_nn",
              "rtk_three_interpolate", "rtk_three_interpolate_grad", "rtk_knn_point"]:
        assert n in names


def test_library_builds_loads_and_exports_everything():
    so = build.build(verbose=False)
    assert os.path.exists(so)
    lib = ctypes.CDLL(so)
    for name in declared_symbols():
        assert hasattr(lib, name), "librtk_hip.so does not export %s" % name
    lib.rtk_version.restype = ctypes.c_int
    assert lib.rtk_version() >= 1
    # the Python binding knows exactly the compute entry points the headers declare, whichever modules were imported
    assert set(_lib.SIGNATURES) | NOT_COMPUTE == set(declared_symbols()), set(_lib.SIGNATURES) ^ set(declared_symbols())


def test_no_cpu_fallback_in_product():
    """The product path must not import, load or execute anything under oracle/ (nor any CPU fallback):
    no import of the package, no string constant naming it outside docstrings."""
    import ast
    pkg = os.path.join(ROOT, "ratrack_amd")
    for path in glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True):
        tree = ast.parse(open(path).read())
        docstrings = set()
        for node in ast.walk(tree):
            if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and node.body and \
                    isinstance(node.body[0], ast.Expr) and isinstance(getattr(node.body[0], "value", None), ast.Constant):
                docstrings.add(id(node.body[0].value))
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                assert not any(a.name.split(".")[0] == "oracle" for a in node.names), path
            elif isinstance(node, ast.ImportFrom):
                assert (node.module or "").split(".")[0] != "oracle", path
            elif isinstance(node, ast.Constant) and isinstance(node.value, str) and id(node) not in docstrings:
                assert "oracle" not in node.value, "%s: string constant mentions oracle: %r" % (path, node.value[:60])
    # and the native library does not link the oracle
    for src in glob.glob(os.path.join(pkg, "csrc", "*")):
        code = re.sub(r"/\*.*?\*/", "", open(src).read(), flags=re.S)              # comments may cite the oracle
        code = re.sub(r"//[^\n]*", "", code)
        assert "__global__" in code or not src.endswith(".hip")
        assert "pointnet2_ref" not in code and "rtk_ref_" not in code, src


def test_ops_refuse_cpu_tensors():
    import torch
    from ratrack_amd import pointnet2_hip
    with pytest.raises(_lib.RtkError):
        pointnet2_hip.ball_query_wrapper(1, 4, 2, 1.0, 2, torch.zeros(1, 2, 3), torch.zeros(1, 4, 3),
                                         torch.zeros(1, 2, 2, dtype=torch.int32))
