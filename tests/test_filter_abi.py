"""The outlier filter's surface without a GPU: the flag constant of the header is the binding's, both entries are declared
and bound, and `city2ba solve --help` names the three flags."""
import os
import re
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_filter", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    return L


def test_flag_constant_and_signatures_match_the_header(tmp_path):
    L = _lib_table()
    src = tmp_path / "flag.c"
    src.write_text('#include <stdio.h>\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    int (*f)(c2b_problem *, double, int, int64_t *) = c2b_problem_filter_observations;\n'
                   '    int (*g)(const double *, const double *, const uint64_t *, int64_t, const void *, const uint32_t *, const double *, int64_t,\n'
                   '             double, int, uint8_t *, void *) = c2b_residual_keep_rows;\n'
                   '    printf("%d %d\\n", C2B_FILTER_IN_FRONT, f != 0 && g != 0);\n    return 0;\n}\n')
    exe = tmp_path / "flag"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(L.FILTER_IN_FRONT), "1"] and L.FILTER_IN_FRONT == 1
    import ctypes as C
    res, args = L.SIGNATURES["c2b_problem_filter_observations"]
    assert res is C.c_int and args == [C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_int64)]
    res, args = L.SIGNATURES["c2b_residual_keep_rows"]
    assert res is C.c_int and len(args) == 12 and args[8] is C.c_double and args[9] is C.c_int and args[7] is C.c_int64


def test_solve_help_names_the_filter_flags(tmp_path):
    cli = entry.build_cli()
    out = subprocess.run([cli, "solve", "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    for flag in ("--filter-max-error", "--filter-rounds", "--filter-in-front"):
        assert flag in out.stdout, flag
    head = open(os.path.join(ROOT, "city2ba_amd", "cli", "main.cpp")).read().split("#include", 1)[0]
    for flag in ("--filter-max-error", "--filter-rounds", "--filter-in-front"):
        assert flag in head, flag                            # the header comment's synopsis
    a, b = str(tmp_path / "a.bal"), str(tmp_path / "b.bal")
    for args, message in ((("--filter-max-error", "-1"), "Invalid value for '--filter-max-error"),
                          (("--filter-max-error", "wide"), "Invalid value for '--filter-max-error <filter-max-error>': invalid float literal"),
                          (("--filter-rounds", "2"), "need --filter-max-error"),
                          (("--filter-in-front",), "need --filter-max-error"),
                          (("--filter-max-error", "0.1", "--filter-rounds", "-1"), "Invalid value for '--filter-rounds")):
        r = subprocess.run([cli, "solve", a, b] + list(args), capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)     # parsed before the device is touched
    assert re.search(r"filter-rounds <N> \[1\]", out.stdout)
