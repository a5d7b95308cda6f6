"""ABI of ivfadc_set_u16_tables (no GPU needed): declared in the header, exported by the library, bound in Python, refused for a null handle
before any device call, usable from C99, and the ABI version is unchanged (the entry adds a symbol; no struct grew)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound(native):
    hdr = open(os.path.join(ROOT, "include", "ivfadc_hip.h")).read()
    assert re.search(r"\bint\s+ivfadc_set_u16_tables\s*\(\s*ivfadc_t\s*\*\s*h\s*,\s*int\s+mode\s*\)\s*;", hdr)
    assert re.search(r"#define\s+IVFADC_ABI_VERSION\s+4\b", hdr)
    lib = native.load_library()
    assert hasattr(lib, "ivfadc_set_u16_tables")
    from ivfadc_jl_amd import _native as nat
    assert nat.ABI_VERSION == 4
    assert nat.lib().ivfadc_set_u16_tables.argtypes == [C.c_void_p, C.c_int]
    assert callable(getattr(native.IVFADCIndex, "set_u16_tables"))


def test_null_handle_is_invalid_without_a_device(native):
    from ivfadc_jl_amd import _native as nat
    lib = nat.lib()
    for mode in (0, 1, 2, 3, -1):
        assert lib.ivfadc_set_u16_tables(None, mode) == nat.ERR_INVALID
    assert b"null handle" in native.load_library().ivfadc_last_error()


def test_entry_compiles_as_c99(tmp_path):
    src = os.path.join(str(tmp_path), "u16_tables.c")
    with open(src, "w") as f:
        f.write('#include "ivfadc_hip.h"\n'
                "int use(ivfadc_t *h) { int (*fn)(ivfadc_t *, int) = ivfadc_set_u16_tables; return fn(h, 1) == IVFADC_ERR_INVALID; }\n")
    obj = os.path.join(str(tmp_path), "u16_tables.o")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", obj])
    assert os.path.getsize(obj) > 0


def test_julia_shim_and_integration_doc_carry_the_wrapper():
    jl = open(os.path.join(ROOT, "julia", "IVFADCHip.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    line = [l for l in jl.splitlines() if "ivfadc_set_u16_tables" in l]
    assert len(line) == 1 and "ccall((:ivfadc_set_u16_tables, LIBIVFADC), Cint, (Ptr{Cvoid}, Cint)" in line[0]
    assert line[0] in doc
