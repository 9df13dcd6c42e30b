"""The index noise's surface without a GPU: the eight entries are declared in the experimental header with the
signatures the binding holds, the stable header's entry count is untouched, NULL out-pointers are accepted, and a NaN fraction or
a NULL handle is refused before a device is touched."""
import ctypes as C
import os
import re
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBLEM = ("c2b_problem_drop_features", "c2b_problem_add_incorrect_correspondences", "c2b_problem_split_landmarks", "c2b_problem_join_landmarks")
ROWS = ("c2b_drop_keep_rows", "c2b_mismatch_partner_rows", "c2b_select_smallest_keys_rows", "c2b_nearest_points_rows")


def _lib_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_index_noise", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    return L


def test_entries_are_declared_in_the_experimental_header_and_link_from_c(tmp_path):
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)            # noqa: E731
    exp = strip(open(os.path.join(ROOT, "include", "city2ba_hip_experimental.h")).read())
    stable = strip(open(os.path.join(ROOT, "include", "city2ba_hip.h")).read())
    for name in PROBLEM + ROWS:
        assert re.search(r"\b%s\s*\(" % name, exp), name
        assert not re.search(r"\b%s\s*\(" % name, stable), name
    assert len(set(re.findall(r"\b(c2b_[a-z0-9_]+)\s*\(", stable))) == 120           # the stable boundary is as it was
    src = tmp_path / "idx.c"
    src.write_text('#include <stdio.h>\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    int (*p[4])(c2b_problem *, double, uint64_t, int64_t *) = {c2b_problem_drop_features, c2b_problem_add_incorrect_correspondences,\n'
                   '                                                               c2b_problem_split_landmarks, c2b_problem_join_landmarks};\n'
                   '    int (*a)(const uint64_t *, int64_t, int64_t, double, uint64_t, uint8_t *, void *) = c2b_drop_keep_rows;\n'
                   '    int (*b)(const uint64_t *, int64_t, const double *, int64_t, double, uint64_t, int32_t *, int64_t *, void *) = c2b_mismatch_partner_rows;\n'
                   '    int (*c)(const uint64_t *, int64_t, uint64_t, int, int, int64_t, uint8_t *, void *) = c2b_select_smallest_keys_rows;\n'
                   '    int (*d)(const double *, int64_t, const uint32_t *, int64_t, int32_t *, void *) = c2b_nearest_points_rows;\n'
                   '    int k, rc = 0;\n'
                   '    for (k = 0; k < 4; ++k) rc += p[k](NULL, 0.5, 1, NULL) == C2B_ERR_INVALID_ARGUMENT;\n'
                   '    printf("%d %d\\n", rc, a != 0 && b != 0 && c != 0 && d != 0);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "idx"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split() == ["4", "1"], (out.stdout, out.stderr)


def test_binding_signatures():
    L = _lib_table()
    for name in PROBLEM:
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and args[:3] == [C.c_void_p, C.c_double, C.c_uint64] and args[3] is C.POINTER(C.c_int64) and len(args) == 4
    assert [len(L.SIGNATURES[n][1]) for n in ROWS] == [7, 9, 8, 6]


def test_null_handles_nan_fractions_and_null_out_pointers_without_a_device():
    entry.build()
    from city2ba_amd import _lib as L
    lib = L.lib()
    nan = float("nan")
    n = C.c_int64(7)
    for name in PROBLEM:
        f = getattr(lib, name)
        assert f(None, 0.5, 1, None) == L.ERR_INVALID_ARGUMENT and b"problem is NULL" in lib.c2b_last_error()
        assert f(None, nan, 1, C.byref(n)) == L.ERR_INVALID_ARGUMENT
    # the row entries check their numbers before any pointer is followed or a device touched
    assert lib.c2b_drop_keep_rows(None, 0, 0, nan, 1, None, None) == L.ERR_INVALID_ARGUMENT and b"NaN" in lib.c2b_last_error()
    assert lib.c2b_mismatch_partner_rows(None, 0, None, 0, nan, 1, None, None, None) == L.ERR_INVALID_ARGUMENT and b"NaN" in lib.c2b_last_error()
    assert lib.c2b_mismatch_partner_rows(None, 1, None, (1 << 31) - 64, 0.5, 1, None, None, None) == L.ERR_INVALID_ARGUMENT
    assert b"n_obs" in lib.c2b_last_error()
    assert lib.c2b_drop_keep_rows(None, 0, 0, 0.5, 1, None, None) == 0                     # nothing to do: no launch, NULL accepted
    assert lib.c2b_drop_keep_rows(None, 2, 5, 0.5, 1, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_select_smallest_keys_rows(None, -1, 1, 8, 0, 1, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_select_smallest_keys_rows(None, 5, 1, -1, 0, 1, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_select_smallest_keys_rows(None, 0, 1, 8, 0, 3, None, None) == 0         # no entity: nothing is launched
    assert lib.c2b_nearest_points_rows(None, 1 << 31, None, 0, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_nearest_points_rows(None, 0, None, 4, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.c2b_nearest_points_rows(None, 0, None, 0, None, None) == 0
