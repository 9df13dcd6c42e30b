"""Resection's surface without a GPU: the status constants of the header are the binding's, both entries are declared and
bound with the header's signatures, `city2ba resect --help` names its options, and bad values fail with their message
before the device is touched."""
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_resect", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    return L


def test_status_constants_and_signatures_match_the_header(tmp_path):
    L = _lib_table()
    src = tmp_path / "res.c"
    src.write_text('#include <stdio.h>\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    int (*f)(c2b_problem *, int, double, uint8_t *, int64_t *) = c2b_problem_resect_cameras;\n'
                   '    int (*g)(double *, const double *, const uint64_t *, int64_t, const uint32_t *, const double *, int, double,\n'
                   '             const c2b_camera_mask *, uint8_t *, int64_t *, void *) = c2b_resect_rows;\n'
                   '    printf("%d %d %d %d %d %d %d\\n", C2B_RES_OK, C2B_RES_TOO_FEW, C2B_RES_DEGENERATE, C2B_RES_BEHIND, C2B_RES_CONSTANT,\n'
                   '           C2B_CONST_POSE, f != 0 && g != 0);\n    return 0;\n}\n')
    exe = tmp_path / "res"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    want = [L.RES_OK, L.RES_TOO_FEW, L.RES_DEGENERATE, L.RES_BEHIND, L.RES_CONSTANT]
    assert out.stdout.split() == [str(v) for v in want] + ["63", "1"] and want == [0, 1, 2, 3, 4]
    assert L.RES_STATUS == ("resected", "too_few", "degenerate", "behind", "constant")
    import ctypes as C
    res, args = L.SIGNATURES["c2b_problem_resect_cameras"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    res, args = L.SIGNATURES["c2b_resect_rows"]
    assert res is C.c_int and len(args) == 12 and args[3] is C.c_int64 and args[6] is C.c_int and args[7] is C.c_double
    assert [k for k, a in enumerate(args) if a is not C.c_void_p] == [3, 6, 7]


def test_resect_help_names_its_options_and_bad_values_fail_before_the_device(tmp_path):
    cli = entry.build_cli()
    out = subprocess.run([cli, "resect", "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "city2ba resect <FILE> <OUT>" in out.stdout
    assert "--min-points <N> [6]" in out.stdout and "--min-gap <G> [1e-4]" in out.stdout
    top = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert top.returncode == 0 and "resect" in top.stdout
    head = open(os.path.join(ROOT, "city2ba_amd", "cli", "main.cpp")).read().split("#include", 1)[0]
    assert "city2ba resect IN OUT [--min-points N] [--min-gap G]" in head          # the header comment's synopsis
    a, b = str(tmp_path / "a.bal"), str(tmp_path / "b.bal")                  # neither exists: a parsed command would fail on the read
    gap = "Invalid value for '--min-gap <G>': expected a number in 0 ... 1 (1 excluded)"
    few = "Invalid value for '--min-points <N>': expected an integer of at least 6"
    for args, message in ((("--min-gap", "-1e-3"), gap), (("--min-gap", "1"), gap), (("--min-gap", "nan"), gap),
                          (("--min-points", "5"), few), (("--min-points", "0"), few),
                          (("--min-gap", "wide"), "Invalid value for '--min-gap <min-gap>': invalid float literal"),
                          (("--min-points", "six"), "Invalid value for '--min-points <min-points>': invalid digit found in string"),
                          (("--min-angle", "3"), "Found argument '--min-angle' which wasn't expected"),
                          (("--min-gap",), "requires a value but none was supplied")):
        r = subprocess.run([cli, "resect", a, b] + list(args), capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    r = subprocess.run([cli, "resect", a], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "required arguments were not provided" in r.stderr
    assert not os.path.exists(b)
