"""Per-camera refinement's surface without a GPU: the two entries are declared and bound with the header's signatures, in the
experimental header alone, and a NULL handle, every bad option and a misaligned pointer are refused before a device is touched."""
import ctypes as C
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_refine_cameras", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    return L


def test_signatures_match_the_header(tmp_path):
    L = _lib_table()
    src = tmp_path / "rfc.c"
    src.write_text('#include <stdio.h>\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    int (*f)(c2b_problem *, const c2b_refine_options *, uint8_t *, int64_t *) = c2b_problem_refine_cameras;\n'
                   '    int (*g)(double *, const double *, int64_t, const uint64_t *, const uint32_t *, const double *, int, double, const double *,\n'
                   '             const double *, const double *, const double *, const c2b_refine_options *, const uint16_t *, uint8_t *, int64_t *,\n'
                   '             void *) = c2b_refine_cameras_rows;\n'
                   '    printf("%d\\n", f != 0 && g != 0);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "rfc"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "1", out.stderr
    res, args = L.SIGNATURES["c2b_problem_refine_cameras"]
    assert res is C.c_int and args == [C.c_void_p] * 4
    res, args = L.SIGNATURES["c2b_refine_cameras_rows"]
    assert res is C.c_int and len(args) == 17
    assert {k: a for k, a in enumerate(args) if a is not C.c_void_p} == {2: C.c_int64, 6: C.c_int, 7: C.c_double}
    stable = open(os.path.join(ROOT, "include", "city2ba_hip.h")).read()
    for name in ("refine_cameras_rows", "problem_refine_cameras"):
        assert name in stable, name                          # the header index (tools/abi_index.py --write)
        assert "int c2b_" + name + "(" not in stable         # declared in the experimental header alone
    exp = open(os.path.join(ROOT, "include", "city2ba_hip_experimental.h")).read()
    assert "int c2b_refine_cameras_rows(" in exp and "int c2b_problem_refine_cameras(" in exp


def test_null_handle_bad_options_and_misaligned_pointers_are_refused_without_a_device():
    entry.build()
    from city2ba_amd import _lib as L
    lib = L.lib()
    good = L.RefineOptions(10, 0, 1e-4, 0.0, 0.0, 0.0)
    assert lib.c2b_problem_refine_cameras(None, C.byref(good), None, None) == L.ERR_INVALID_ARGUMENT
    counts = (C.c_int64 * 6)(*([-7] * 6))
    inf, nan = float("inf"), float("nan")

    def rows(opt, n_cam=0, kind=0, a2=1.0, cn=counts, bal9=None, c0=None, cw=None, i0=None, iw=None, mask=None):
        return lib.c2b_refine_cameras_rows(bal9, None, n_cam, None, None, None, kind, a2, c0, cw, i0, iw, None if opt is None else C.byref(opt), mask,
                                           None, cn, None)
    for opt, word in ((L.RefineOptions(-1, 0, 1e-4, 0, 0, 0), b"max_rounds"), (L.RefineOptions(10, 1, 1e-4, 0, 0, 0), b"reserved"),
                      (L.RefineOptions(10, 0, 0.0, 0, 0, 0), b"lambda0"), (L.RefineOptions(10, 0, 1e33, 0, 0, 0), b"lambda0"),
                      (L.RefineOptions(10, 0, nan, 0, 0, 0), b"lambda0"), (L.RefineOptions(10, 0, 1e-4, -1.0, 0, 0), b"tolerances"),
                      (L.RefineOptions(10, 0, 1e-4, 0, inf, 0), b"tolerances"), (L.RefineOptions(10, 0, 1e-4, 0, 0, nan), b"tolerances"), (None, b"options")):
        assert rows(opt) == L.ERR_INVALID_ARGUMENT and word in lib.c2b_last_error(), lib.c2b_last_error()
    for n_cam, kind, a2, word in ((-1, 0, 1.0, b"n_cam"), (1 << 31, 0, 1.0, b"n_cam"), (0, 4, 1.0, b"loss"), (0, -1, 1.0, b"loss"), (0, 2, 0.0, b"loss"),
                                  (0, 2, nan, b"loss"), (0, 1, inf, b"loss")):
        assert rows(good, n_cam, kind, a2) == L.ERR_INVALID_ARGUMENT and word in lib.c2b_last_error(), lib.c2b_last_error()
    assert rows(good, cn=None) == L.ERR_INVALID_ARGUMENT and b"NULL" in lib.c2b_last_error()
    assert rows(good, n_cam=1) == L.ERR_INVALID_ARGUMENT and b"NULL" in lib.c2b_last_error()
    buf = (C.c_double * 8)()
    at = C.addressof(buf)
    assert rows(good, c0=at) == L.ERR_INVALID_ARGUMENT and b"pairs" in lib.c2b_last_error()
    assert rows(good, i0=at, iw=None) == L.ERR_INVALID_ARGUMENT and b"pairs" in lib.c2b_last_error()
    for kw in (dict(bal9=at + 4), dict(c0=at + 4, cw=at), dict(c0=at, cw=at + 4), dict(i0=at + 4, iw=at), dict(i0=at, iw=at + 4), dict(mask=at + 1)):
        assert rows(good, **kw) == L.ERR_INVALID_ARGUMENT and b"misaligned" in lib.c2b_last_error(), (kw, lib.c2b_last_error())
    assert lib.c2b_refine_cameras_rows(None, None, 0, None, None, None, 0, 1.0, None, None, None, None, C.byref(good), None, None,
                                       C.c_void_p(C.addressof(counts) + 4), None) == L.ERR_INVALID_ARGUMENT
    assert list(counts) == [-7] * 6                           # nothing was written
