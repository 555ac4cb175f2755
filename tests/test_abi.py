"""The C-ABI library loads and exports every symbol include/dcap.h declares (no compute: CPU-safe)."""
import os
import re

import pytest


def test_library_builds_loads_and_exports_every_declared_symbol(repo_root):
    import __graft_entry__ as G
    G.build()
    from image_captioning_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(repo_root, "include", "dcap.h")).read()
    declared = set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations found"
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.dc_version() == _lib.ABI_VERSION == 600


def test_structures_have_the_layout_the_c_compiler_gives_the_header(repo_root, tmp_path):
    """The Structures _lib.py reads out of include/dcap.h against a real compiler: a C program that includes the header prints sizeof of
    every struct and offsetof / size of every field, and every number must be ctypes' own."""
    import ctypes
    import shutil
    import subprocess
    from image_captioning_amd import _lib
    assert _lib.STRUCTURES
    lines = ['#include <stdio.h>', '#include "dcap.h"', 'int main(void) {']
    expected = []
    for c_name, cls in _lib.STRUCTURES.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        expected.append("%s %d" % (c_name, ctypes.sizeof(cls)))
        for field, _ in cls._fields_:
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (c_name, field, c_name, field, c_name, field))
            expected.append("%s.%s %d %d" % (c_name, field, getattr(cls, field).offset, getattr(cls, field).size))
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    cmd = [cc] if cc else [shutil.which("hipcc") or "/opt/rocm/bin/hipcc", "-x", "c"]
    subprocess.run(cmd + ["-I", os.path.join(repo_root, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")[:-1]
    assert len(got) == len(expected) > 400
    assert got == expected, [(g, e) for g, e in zip(got, expected) if g != e][:10]


def test_the_header_parser_is_strict_and_skips_nothing(repo_root):
    from image_captioning_amd import _lib
    ok = "#define DC_N 3\ntypedef struct { int a, b[DC_N]; const float* p; } dc_t_desc;\nint dc_f(const dc_t_desc* d, void* stream);\n"
    constants, structures, symbols = _lib.parse_header(ok)
    assert constants == {"DC_N": 3} and [n for n, _ in structures["dc_t_desc"]._fields_] == ["a", "b", "p"] and list(symbols) == ["dc_f"]
    assert structures["dc_t_desc"].__name__ == "TDesc" and len(structures["dc_t_desc"]().b) == 3
    import ctypes
    _, s2, f2 = _lib.parse_header("typedef struct { int* counts; const int* sizes; } dc_u_desc;\nint dc_g(const int* sizes, int* n, int k);\n")
    assert [t for _, t in s2["dc_u_desc"]._fields_] == [ctypes.c_void_p, ctypes.c_void_p]      # data pointers, whatever they point at
    assert f2["dc_g"][1] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]       # only a non-const int* argument is an output
    for bad, what in (("typedef struct { int a; quaternion_t q; } dc_t_desc;", "unknown type 'quaternion_t'"),          # unknown field type
                      ("int dc_f(const dc_missing_desc* d);", "unknown type 'dc_missing_desc\\*'"),                      # unknown struct
                      ("typedef struct { int a[DC_NOPE]; } dc_t_desc;", "unknown array bound 'DC_NOPE'"),
                      ("typedef struct { int a b; } dc_t_desc;", "cannot read the declaration 'int a b'"),               # malformed field
                      ("typedef struct { float* a, b; } dc_t_desc;", "cannot read the declaration"),                     # b would be a float
                      ("int dc_f(int (*callback)(int));", "cannot read the declaration that starts 'int dc_f"),          # malformed prototype
                      ("int dc_f(int);", "cannot read the argument 'int'"),
                      ("typedef struct { float; } dc_t_desc;", "cannot read the declaration 'float'"),
                      ("struct dc_other { int a; };", "cannot read the declaration that starts 'struct dc_other"),
                      ("#define DC_X (1 << 4)\n", "DC_X")):
        with pytest.raises(_lib.DcapError, match=what):
            _lib.parse_header(bad)
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(repo_root, "include", "dcap.h")).read(), flags=re.S)
    assert len(re.findall(r"\btypedef\s+struct\b", header)) == len(_lib.STRUCTURES) > 0
    assert len(re.findall(r"\bdc_\w+\s*\(", header)) == len(_lib.SYMBOLS) > 0
    assert len(re.findall(r"#define\s+DC_\w+\s+-?\d", header)) == len(_lib.CONSTANTS) > 0
    for cls in _lib.STRUCTURES.values():
        assert getattr(_lib, cls.__name__) is cls


def test_missing_library_fails_loudly(monkeypatch):
    from image_captioning_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libdcap_hip.so")
    with pytest.raises(_lib.DcapError, match="no CPU fallback"):
        _lib.load()


def test_ops_refuse_cpu_tensors():
    import torch
    from image_captioning_amd import ops, _lib
    with pytest.raises(_lib.DcapError):
        ops.gemm(torch.zeros(8, 8), torch.zeros(8, 8))


def test_device_code_is_built_without_compiler_packed_f32():
    """The build keeps -fno-slp-vectorize: with the compiler's v_pk_*_f32 packing dc_vocab_ce's gradient was not reproducible from call to
    call on MI355X (tests/test_gpu_bf16.py::test_vocab_ce_is_bit_identical_from_call_to_call)."""
    import __graft_entry__ as entry
    assert "-fno-slp-vectorize" in entry.FLAGS and "-O3" in entry.FLAGS


def test_library_binds_to_the_hip_runtime_torch_brought(repo_root):
    """One HIP / HSA runtime per process: loaded before torch, the library would map /opt/rocm's copy and torch then its own bundled
    one (same soname) -- on a GPU box the library's launches then fail with "no ROCm-capable device is detected" (round 6: build()
    followed by smoke() in one process).  _lib.load() imports torch first; checked in a fresh interpreter that has not imported it."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from image_captioning_amd import _lib\n"
            "assert 'torch' not in sys.modules\n"
            "_lib.load()\n"
            "libs = sorted(set(l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l or 'libhsa-runtime64' in l))\n"
            "print('\\n'.join(libs))\n") % repo_root
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    libs = out.stdout.split()
    assert len([l for l in libs if "libamdhip64" in l]) == 1 and len([l for l in libs if "libhsa-runtime64" in l]) == 1, libs
    assert all(os.sep + "torch" + os.sep in l for l in libs), libs


@pytest.mark.gpu
def test_build_then_smoke_in_one_process(repo_root):
    """What a driver may do on the GPU box: __graft_entry__.build() (loads the library before anything touched torch.cuda) and then
    smoke() in the same interpreter."""
    import subprocess
    import sys
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.build(); g.smoke()"], cwd=repo_root, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "smoke ok" in out.stdout, (out.stdout[-1000:], out.stderr[-2000:])
