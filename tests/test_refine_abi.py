"""Per-point refinement's surface without a GPU: the five statuses of the header are the binding's, the four entries are
declared and bound with the header's signatures, the option struct has the header's size and field offsets, and a NULL
handle and every bad option are refused before a device is touched."""
import ctypes as C
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_refine", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    return L


def test_constants_struct_and_signatures_match_the_header(tmp_path):
    L = _lib_table()
    src = tmp_path / "rfn.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    int (*f)(c2b_problem *, const c2b_refine_options *, uint8_t *, int64_t *) = c2b_problem_refine_points;\n'
                   '    int (*g)(const double *, double *, int64_t, const uint64_t *, const uint32_t *, const uint32_t *, const double *, int, double,\n'
                   '             const double *, const double *, const c2b_refine_options *, const uint8_t *, uint8_t *, int64_t *, void *) = c2b_refine_points_rows;\n'
                   '    int (*s)(c2b_problem *, int) = c2b_problem_set_inner_iterations;\n'
                   '    int (*t)(c2b_problem *, int *) = c2b_problem_get_inner_iterations;\n'
                   '    printf("%d %d %d %d %d %d\\n", C2B_REFINE_CONVERGED, C2B_REFINE_MAX_ROUNDS, C2B_REFINE_UNOBSERVED, C2B_REFINE_FAILED,\n'
                   '           C2B_REFINE_CONSTANT, f != 0 && g != 0 && s != 0 && t != 0);\n'
                   '    printf("%d %d %d %d %d %d %d\\n", (int)sizeof(c2b_refine_options), (int)offsetof(c2b_refine_options, max_rounds),\n'
                   '           (int)offsetof(c2b_refine_options, reserved), (int)offsetof(c2b_refine_options, lambda0),\n'
                   '           (int)offsetof(c2b_refine_options, function_tol), (int)offsetof(c2b_refine_options, gradient_tol),\n'
                   '           (int)offsetof(c2b_refine_options, parameter_tol));\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "rfn"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    first, second = out.stdout.strip().split("\n")
    assert first.split() == ["0", "1", "2", "3", "4", "1"]
    assert (L.REFINE_CONVERGED, L.REFINE_MAX_ROUNDS, L.REFINE_UNOBSERVED, L.REFINE_FAILED, L.REFINE_CONSTANT) == (0, 1, 2, 3, 4)
    assert L.REFINE_STATUS == ("converged", "max_rounds", "unobserved", "failed", "constant") and L.REFINE_COUNTS == L.REFINE_STATUS + ("moved",)
    O = L.RefineOptions
    assert [int(v) for v in second.split()] == [C.sizeof(O), O.max_rounds.offset, O.reserved.offset, O.lambda0.offset, O.function_tol.offset,
                                                O.gradient_tol.offset, O.parameter_tol.offset] == [40, 0, 4, 8, 16, 24, 32]
    res, args = L.SIGNATURES["c2b_problem_refine_points"]
    assert res is C.c_int and args == [C.c_void_p] * 4
    res, args = L.SIGNATURES["c2b_refine_points_rows"]
    assert res is C.c_int and len(args) == 16
    assert {k: a for k, a in enumerate(args) if a is not C.c_void_p} == {2: C.c_int64, 7: C.c_int, 8: C.c_double}
    assert L.SIGNATURES["c2b_problem_set_inner_iterations"] == (C.c_int, [C.c_void_p, C.c_int])
    res, args = L.SIGNATURES["c2b_problem_get_inner_iterations"]
    assert res is C.c_int and args[0] is C.c_void_p and args[1] is C.POINTER(C.c_int)
    head = open(os.path.join(ROOT, "include", "city2ba_hip.h")).read()
    for name in ("refine_points_rows", "problem_refine_points", "problem_set_inner_iterations", "problem_get_inner_iterations"):
        assert name in head, name                            # the header index (tools/abi_index.py --write)


def test_null_handle_and_bad_options_are_refused_without_a_device():
    entry.build()
    from city2ba_amd import _lib as L
    lib = L.lib()
    good = L.RefineOptions(10, 0, 1e-4, 0.0, 0.0, 0.0)
    assert lib.c2b_problem_refine_points(None, C.byref(good), None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_problem_set_inner_iterations(None, 1) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_problem_get_inner_iterations(None, None) == L.ERR_INVALID_ARGUMENT
    counts = (C.c_int64 * 6)(*([-7] * 6))
    inf, nan = float("inf"), float("nan")

    def rows(opt, n_pts=0, kind=0, a2=1.0, cn=counts):
        return lib.c2b_refine_points_rows(None, None, n_pts, None, None, None, None, kind, a2, None, None, None if opt is None else C.byref(opt), None, None, cn, None)
    for opt, word in ((L.RefineOptions(-1, 0, 1e-4, 0, 0, 0), b"max_rounds"), (L.RefineOptions(10, 1, 1e-4, 0, 0, 0), b"reserved"),
                      (L.RefineOptions(10, 0, 0.0, 0, 0, 0), b"lambda0"), (L.RefineOptions(10, 0, 1e33, 0, 0, 0), b"lambda0"),
                      (L.RefineOptions(10, 0, nan, 0, 0, 0), b"lambda0"), (L.RefineOptions(10, 0, 1e-4, -1.0, 0, 0), b"tolerances"),
                      (L.RefineOptions(10, 0, 1e-4, 0, inf, 0), b"tolerances"), (L.RefineOptions(10, 0, 1e-4, 0, 0, nan), b"tolerances"), (None, b"options")):
        assert rows(opt) == L.ERR_INVALID_ARGUMENT and word in lib.c2b_last_error(), lib.c2b_last_error()
    for n_pts, kind, a2, word in ((-1, 0, 1.0, b"n_pts"), (1 << 33, 0, 1.0, b"n_pts"), (0, 4, 1.0, b"loss"), (0, -1, 1.0, b"loss"), (0, 2, 0.0, b"loss"),
                                  (0, 2, nan, b"loss"), (0, 1, inf, b"loss")):
        assert rows(good, n_pts, kind, a2) == L.ERR_INVALID_ARGUMENT and word in lib.c2b_last_error(), lib.c2b_last_error()
    assert rows(good, cn=None) == L.ERR_INVALID_ARGUMENT
    assert list(counts) == [-7] * 6                           # nothing was written
