"""The matrix-mode switch of libgcdm_ops.so (include/gcdm_matrix_mode.h) without a GPU: the two exports, their values, the Python wrappers and
the header as plain C.  No HIP call is made: the switch is a host-side atomic word that the GEMM entries read."""
import ctypes
import importlib
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("bio-diffusion_amd")
native = pkg._native
ops = pkg.ops
HEADER = os.path.join(ROOT, "include", "gcdm_matrix_mode.h")


@pytest.fixture()
def lib():
    assert os.path.exists(native.OPS_LIB_PATH), "libgcdm_ops.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(native.OPS_LIB_PATH)
    for name in ("gcdm_ops_set_matrix_mode", "gcdm_ops_get_matrix_mode"):
        assert hasattr(lib, name), f"libgcdm_ops.so does not export {name}"
    lib.gcdm_ops_set_matrix_mode.argtypes = [ctypes.c_int32]
    lib.gcdm_ops_set_matrix_mode.restype = ctypes.c_int
    lib.gcdm_ops_get_matrix_mode.argtypes = []
    lib.gcdm_ops_get_matrix_mode.restype = ctypes.c_int32
    try:
        yield lib
    finally:
        lib.gcdm_ops_set_matrix_mode(0)


def test_bound_in_a_table_of_their_own():
    assert sorted(native.MATRIX_MODE_SIGNATURES) == ["gcdm_ops_get_matrix_mode", "gcdm_ops_set_matrix_mode"]
    assert not set(native.MATRIX_MODE_SIGNATURES) & set(native.OPS_SIGNATURES)
    assert not set(native.MATRIX_MODE_SIGNATURES) & set(native.OPS_EXPORTS)
    assert native.MATRIX_MODES == {"f32": 0, "bf16x6": 1}


def test_default_is_f32_on_load():
    # a fresh process: whatever other tests of this session did to the switch cannot show here
    code = ("import ctypes, sys; lib = ctypes.CDLL(sys.argv[1]); lib.gcdm_ops_get_matrix_mode.restype = ctypes.c_int32; "
            "sys.exit(10 + lib.gcdm_ops_get_matrix_mode())")
    r = subprocess.run([sys.executable, "-c", code, native.OPS_LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 10, (r.returncode, r.stderr)


def test_set_accepts_the_two_modes_only(lib):
    assert lib.gcdm_ops_get_matrix_mode() == 0
    assert lib.gcdm_ops_set_matrix_mode(1) == 0
    assert lib.gcdm_ops_get_matrix_mode() == 1
    assert lib.gcdm_ops_set_matrix_mode(0) == 0
    assert lib.gcdm_ops_get_matrix_mode() == 0
    assert lib.gcdm_ops_set_matrix_mode(1) == 0
    for bad in (7, -1, 2, 2 ** 31 - 1, -2 ** 31):
        assert lib.gcdm_ops_set_matrix_mode(bad) == -1
        assert lib.gcdm_ops_get_matrix_mode() == 1          # a rejected value changes nothing
    assert lib.gcdm_ops_set_matrix_mode(0) == 0
    assert lib.gcdm_ops_set_matrix_mode(7) == -1
    assert lib.gcdm_ops_set_matrix_mode(-1) == -1
    assert lib.gcdm_ops_get_matrix_mode() == 0


def test_python_wrappers_and_context_manager(lib):
    assert ops.get_matrix_mode() == "f32"
    ops.set_matrix_mode("bf16x6")
    try:
        assert ops.get_matrix_mode() == "bf16x6"
        assert lib.gcdm_ops_get_matrix_mode() == 1           # one process-wide word, whichever handle looks at it
        with ops.matrix_mode("f32"):
            assert ops.get_matrix_mode() == "f32"
        assert ops.get_matrix_mode() == "bf16x6"
    finally:
        ops.set_matrix_mode("f32")
    with pytest.raises(ValueError):
        ops.set_matrix_mode("bf16")
    with pytest.raises(ValueError):
        with ops.matrix_mode("f16x3"):
            pass
    assert ops.get_matrix_mode() == "f32"
    with ops.matrix_mode("bf16x6"):
        assert ops.get_matrix_mode() == "bf16x6"
    assert ops.get_matrix_mode() == "f32"


def test_context_manager_restores_when_the_body_raises(lib):
    class Boom(Exception):
        pass

    with pytest.raises(Boom):
        with ops.matrix_mode("bf16x6"):
            assert ops.get_matrix_mode() == "bf16x6"
            raise Boom()
    assert ops.get_matrix_mode() == "f32"
    assert lib.gcdm_ops_get_matrix_mode() == 0


def test_header_compiles_and_links_from_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    assert gcc is not None, "no gcc"
    src = tmp_path / "t.c"
    src.write_text('#include "gcdm_matrix_mode.h"\n'
                   'int main(void) {\n'
                   '  if (GCDM_OPS_MATRIX_F32 != 0 || GCDM_OPS_MATRIX_BF16X6 != 1) return 1;\n'
                   '  if (gcdm_ops_get_matrix_mode() != GCDM_OPS_MATRIX_F32) return 2;\n'
                   '  if (gcdm_ops_set_matrix_mode(GCDM_OPS_MATRIX_BF16X6) != 0 || gcdm_ops_get_matrix_mode() != 1) return 3;\n'
                   '  if (gcdm_ops_set_matrix_mode(7) != -1 || gcdm_ops_set_matrix_mode(-1) != -1 || gcdm_ops_get_matrix_mode() != 1) return 4;\n'
                   '  if (gcdm_ops_set_matrix_mode(GCDM_OPS_MATRIX_F32) != 0 || gcdm_ops_get_matrix_mode() != 0) return 5;\n'
                   '  return 0; }\n')
    exe = tmp_path / "t"
    libdir = os.path.dirname(native.OPS_LIB_PATH)
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe), "-L", libdir,
                        "-l:libgcdm_ops.so", f"-Wl,-rpath,{libdir}", "-Wl,--unresolved-symbols=ignore-in-shared-libs"], text=True, capture_output=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
