"""The sub-problem entries' surface without a GPU: the four symbols are declared in the header with the signatures the
binding uses and are exported by the library, the two flags are the binding's, the ABI version is the header's, and NULL
arguments are refused before a device is touched."""
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_subset", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    return L


def test_symbols_flags_and_version_match_the_header(tmp_path):
    L = _lib_table()
    src = tmp_path / "sub.c"
    src.write_text('#include <stdio.h>\n#include "city2ba_hip.h"\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    int (*a)(c2b_problem *, const uint32_t *, int64_t, const uint32_t *, int64_t, int, c2b_problem *) = c2b_problem_subset;\n'
                   '    int (*b)(c2b_problem *, const uint8_t *, int, c2b_problem *) = c2b_problem_window;\n'
                   '    int (*c)(const c2b_problem *, uint32_t *, uint32_t *, uint8_t *, uint8_t *) = c2b_problem_get_origin;\n'
                   '    int (*d)(c2b_problem *, c2b_problem *, int64_t *, int64_t *) = c2b_problem_write_back;\n'
                   '    printf("%d %d %d %d %d\\n", C2B_SUBSET_CARRY, C2B_WINDOW_HALO, C2B_ABI_VERSION, c2b_abi_version(), a != 0 && b != 0 && c != 0 && d != 0);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "sub"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(L.SUBSET_CARRY), str(L.WINDOW_HALO), str(L.ABI_VERSION), str(L.ABI_VERSION), "1"]
    assert (L.SUBSET_CARRY, L.WINDOW_HALO, L.ABI_VERSION) == (1, 1, 10)
    import ctypes as C
    vp, i64 = C.c_void_p, C.c_int64
    assert L.SIGNATURES["c2b_problem_subset"] == (C.c_int, [vp, vp, i64, vp, i64, C.c_int, vp])
    assert L.SIGNATURES["c2b_problem_window"] == (C.c_int, [vp, vp, C.c_int, vp])
    assert L.SIGNATURES["c2b_problem_get_origin"] == (C.c_int, [vp, vp, vp, vp, vp])
    res, args = L.SIGNATURES["c2b_problem_write_back"]
    assert res is C.c_int and args[:2] == [vp, vp] and args[2] is C.POINTER(i64) and args[3] is C.POINTER(i64)


def test_the_four_entries_are_bound_and_refuse_null_without_a_device():
    import ctypes as C
    entry.build()
    from city2ba_amd import _lib as L
    lib = L.lib()
    assert lib.c2b_abi_version() == L.ABI_VERSION
    sel = (C.c_uint32 * 2)(0, 1)
    seed = (C.c_uint8 * 2)(1, 0)
    a, b = C.c_int64(-7), C.c_int64(-7)
    for call, word in ((lambda: lib.c2b_problem_subset(None, sel, 2, sel, 2, 0, None), b"problem_subset"),
                       (lambda: lib.c2b_problem_window(None, seed, L.WINDOW_HALO, None), b"problem_window"),
                       (lambda: lib.c2b_problem_get_origin(None, None, None, None, None), b"problem_get_origin"),
                       (lambda: lib.c2b_problem_write_back(None, None, C.byref(a), C.byref(b)), b"problem_write_back")):
        rc = call()
        assert rc == L.ERR_INVALID_ARGUMENT and word in lib.c2b_last_error() and b"NULL" in lib.c2b_last_error(), lib.c2b_last_error()
    assert (a.value, b.value) == (-7, -7)                    # nothing written on a refusal
