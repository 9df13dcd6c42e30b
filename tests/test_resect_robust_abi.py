"""Consensus resection's surface without a GPU: the new status and flag of the header are the binding's, both entries are
declared and bound with the header's signatures, `city2ba resect --help` names the four new flags after the text it had, and
bad values fail with their message before the device is touched."""
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_resect_robust", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    return L


def test_constants_and_signatures_match_the_header(tmp_path):
    L = _lib_table()
    src = tmp_path / "rrc.c"
    src.write_text('#include <stdio.h>\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    int (*f)(c2b_problem *, double, int, double, int, int, uint8_t *, int32_t *, int32_t *, uint8_t *, int64_t *, int64_t *) =\n'
                   '        c2b_problem_resect_consensus;\n'
                   '    int (*g)(double *, const double *, const uint64_t *, int64_t, const uint32_t *, const double *, int64_t, double, int, double,\n'
                   '             int, const c2b_camera_mask *, uint8_t *, int32_t *, int32_t *, uint8_t *, int64_t *, void *) =\n'
                   '        c2b_resect_consensus_rows;\n'
                   '    printf("%d %d %d %d\\n", C2B_RES_NO_CONSENSUS, C2B_RES_DROP_OUTLIERS, C2B_RES_CONSTANT, f != 0 && g != 0);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "rrc"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(L.RES_NO_CONSENSUS), str(L.RES_DROP_OUTLIERS), str(L.RES_CONSTANT), "1"]
    assert L.RES_NO_CONSENSUS == 5 and L.RES_DROP_OUTLIERS == 1
    assert L.RES_STATUS == ("resected", "too_few", "degenerate", "behind", "constant")
    assert L.RES_CONSENSUS_STATUS == L.RES_STATUS + ("no_consensus",)
    import ctypes as C
    res, args = L.SIGNATURES["c2b_problem_resect_consensus"]
    assert res is C.c_int and len(args) == 12 and args[1:6] == [C.c_double, C.c_int, C.c_double, C.c_int, C.c_int]
    assert args[0] is C.c_void_p and args[6:11] == [C.c_void_p] * 5 and args[11] is C.POINTER(C.c_int64)
    res, args = L.SIGNATURES["c2b_resect_consensus_rows"]
    assert res is C.c_int and len(args) == 18
    assert {k: a for k, a in enumerate(args) if a is not C.c_void_p} == {3: C.c_int64, 6: C.c_int64, 7: C.c_double, 8: C.c_int, 9: C.c_double, 10: C.c_int}


def test_null_handle_and_bad_values_are_refused_without_a_device():
    import ctypes as C
    entry.build()
    from city2ba_amd import _lib as L
    lib = L.lib()
    assert lib.c2b_problem_resect_consensus(None, 0.01, 6, 1e-4, 64, 0, None, None, None, None, None, None) == L.ERR_INVALID_ARGUMENT
    counts = (C.c_int64 * 6)()
    for err, mi, gap, mh, word in ((-1.0, 6, 1e-4, 64, b"max_error"), (float("inf"), 6, 1e-4, 64, b"max_error"), (float("nan"), 6, 1e-4, 64, b"max_error"),
                                   (0.01, 5, 1e-4, 64, b"min_inliers"), (0.01, 6, -1.0, 64, b"min_gap"), (0.01, 6, float("nan"), 64, b"min_gap"),
                                   (0.01, 6, 1.0, 64, b"min_gap"), (0.01, 6, 1e-4, 0, b"max_hypotheses"), (0.01, 6, 1e-4, 65, b"max_hypotheses")):
        rc = lib.c2b_resect_consensus_rows(None, None, None, 0, None, None, 0, err, mi, gap, mh, None, None, None, None, None, counts, None)
        assert rc == L.ERR_INVALID_ARGUMENT and word in lib.c2b_last_error(), (err, mi, gap, mh, lib.c2b_last_error())


def test_resect_help_names_the_new_flags_and_bad_values_fail_before_the_device(tmp_path):
    cli = entry.build_cli()
    out = subprocess.run([cli, "resect", "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    old = out.stdout.index("--min-gap <G> [1e-4]")
    assert out.stdout.index("--min-points <N> [6]") < old
    for flag in ("--max-error <X>", "--min-inliers <N> [6]", "--max-hypotheses <H> [64]", "--drop-outliers"):
        assert flag in out.stdout and out.stdout.index(flag) > old, flag
    head = open(os.path.join(ROOT, "city2ba_amd", "cli", "main.cpp")).read().split("#include", 1)[0]
    assert "city2ba resect IN OUT [--min-points N] [--min-gap G] [--max-error X [--min-inliers N] [--max-hypotheses H] [--drop-outliers]]" in head
    a, b = str(tmp_path / "a.bal"), str(tmp_path / "b.bal")                  # neither exists: a parsed command would fail on the read
    need = "--min-inliers, --max-hypotheses and --drop-outliers need --max-error <X>"
    for args, message in ((("--max-error", "-1"), "Invalid value for '--max-error <X>': expected a finite number >= 0"),
                          (("--max-error", "inf"), "Invalid value for '--max-error <X>': expected a finite number >= 0"),
                          (("--max-error", "nan"), "Invalid value for '--max-error <X>': expected a finite number >= 0"),
                          (("--max-error", "wide"), "Invalid value for '--max-error <max-error>': invalid float literal"),
                          (("--max-error",), "requires a value but none was supplied"),
                          (("--max-error", "0.01", "--min-inliers", "5"), "Invalid value for '--min-inliers <N>': expected an integer of at least 6"),
                          (("--max-error", "0.01", "--min-inliers", "six"), "Invalid value for '--min-inliers <min-inliers>'"),
                          (("--max-error", "0.01", "--max-hypotheses", "0"), "Invalid value for '--max-hypotheses <H>': expected an integer in 1 ... 64"),
                          (("--max-error", "0.01", "--max-hypotheses", "65"), "Invalid value for '--max-hypotheses <H>': expected an integer in 1 ... 64"),
                          (("--max-error", "0.01", "--min-gap", "1"), "Invalid value for '--min-gap <G>': expected a number in 0 ... 1 (1 excluded)"),
                          (("--max-error", "0.01", "--min-points", "8"), "--min-points does not go with --max-error <X>: --min-inliers <N> takes its place"),
                          (("--min-inliers", "6"), need), (("--max-hypotheses", "8"), need), (("--drop-outliers",), need)):
        r = subprocess.run([cli, "resect", a, b] + list(args), capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    assert not os.path.exists(b)
