"""Guided re-matching's surface without a GPU: the four statuses of the header are the binding's, both entries are declared
and bound with the header's signatures, a NULL handle and every bad value are refused before a device is touched, and
`city2ba rematch --help` names the flags after the text the help already had."""
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_rematch", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    return L


def test_constants_and_signatures_match_the_header(tmp_path):
    L = _lib_table()
    src = tmp_path / "rmt.c"
    src.write_text('#include <stdio.h>\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    int (*f)(c2b_problem *, double, double, int, uint8_t *, int64_t *, int64_t *) = c2b_problem_rematch_observations;\n'
                   '    int (*g)(const double *, const double *, int64_t, const uint64_t *, int64_t, const uint32_t *, const double *, int64_t,\n'
                   '             const uint8_t *, const uint8_t *, double, double, int32_t *, uint8_t *, int64_t *, void *) = c2b_rematch_rows;\n'
                   '    printf("%d %d %d %d %d\\n", C2B_REMATCH_FITS, C2B_REMATCH_SKIPPED, C2B_REMATCH_REASSIGNED, C2B_REMATCH_REMOVED, f != 0 && g != 0);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "rmt"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(L.REMATCH_FITS), str(L.REMATCH_SKIPPED), str(L.REMATCH_REASSIGNED), str(L.REMATCH_REMOVED), "1"]
    assert (L.REMATCH_FITS, L.REMATCH_SKIPPED, L.REMATCH_REASSIGNED, L.REMATCH_REMOVED) == (0, 1, 2, 3)
    assert L.REMATCH_STATUS == ("fits", "skipped", "reassigned", "removed")
    import ctypes as C
    res, args = L.SIGNATURES["c2b_problem_rematch_observations"]
    assert res is C.c_int and len(args) == 7 and args[:5] == [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p]
    assert args[5] is C.POINTER(C.c_int64) and args[6] is C.POINTER(C.c_int64)
    res, args = L.SIGNATURES["c2b_rematch_rows"]
    assert res is C.c_int and len(args) == 16
    assert {k: a for k, a in enumerate(args) if a is not C.c_void_p} == {2: C.c_int64, 4: C.c_int64, 7: C.c_int64, 10: C.c_double, 11: C.c_double}


def test_null_handle_and_bad_values_are_refused_without_a_device():
    import ctypes as C
    entry.build()
    from city2ba_amd import _lib as L
    lib = L.lib()
    assert lib.c2b_problem_rematch_observations(None, 0.5, 1e-2, 2, None, None, None) == L.ERR_INVALID_ARGUMENT
    counts = (C.c_int64 * 4)()
    inf, nan = float("inf"), float("nan")
    for radius, err, n_pts, n_obs, word in ((-1.0, 1e-2, 0, 0, b"radius"), (inf, 1e-2, 0, 0, b"radius"), (nan, 1e-2, 0, 0, b"radius"),
                                            (0.5, -1.0, 0, 0, b"max_error"), (0.5, inf, 0, 0, b"max_error"), (0.5, nan, 0, 0, b"max_error"),
                                            (0.5, 1e-2, 1 << 31, 0, b"n_pts"), (0.5, 1e-2, -1, 0, b"n_pts"), (0.5, 1e-2, 1, (1 << 31) - 64, b"n_obs"),
                                            (0.5, 1e-2, 1, -1, b"n_obs"), (0.5, 1e-2, 0, 5, b"without points")):
        rc = lib.c2b_rematch_rows(None, None, n_pts, None, 1, None, None, n_obs, None, None, radius, err, None, None, counts, None)
        assert rc == L.ERR_INVALID_ARGUMENT and word in lib.c2b_last_error(), (radius, err, n_pts, n_obs, lib.c2b_last_error())
    assert lib.c2b_rematch_rows(None, None, 0, None, 0, None, None, 0, None, None, 0.5, 1e-2, None, None, None, None) == L.ERR_INVALID_ARGUMENT


def test_rematch_help_names_the_flags_and_bad_values_fail_before_the_device(tmp_path):
    cli = entry.build_cli()
    out = subprocess.run([cli, "rematch", "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    for flag in ("city2ba rematch <FILE> <OUT>", "--radius <R>", "--max-error <X>", "--min-fits <N> [2]", "is removed", "Nothing is culled", "--device <N>"):
        assert flag in out.stdout, flag
    top = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert top.index("    rematch ") > top.index("    merge ") > top.index("    resect ")            # after the text the help already had
    head = open(os.path.join(ROOT, "city2ba_amd", "cli", "main.cpp")).read().split("#include", 1)[0]
    assert "city2ba rematch IN OUT --radius R --max-error X [--min-fits N]" in head
    assert head.index("city2ba rematch IN OUT") > head.index("city2ba merge IN OUT")
    a, b = str(tmp_path / "a.bal"), str(tmp_path / "b.bal")                  # neither exists: a parsed command would fail on the read
    finite = ": expected a finite number >= 0"
    for args, message in (((), "--radius <R> --max-error <X>"), (("--radius", "0.5"), "--radius <R> --max-error <X>"),
                          (("--max-error", "1e-2"), "--radius <R> --max-error <X>"),
                          (("--radius", "-1", "--max-error", "1e-2"), "Invalid value for '--radius <R>'" + finite),
                          (("--radius", "inf", "--max-error", "1e-2"), "Invalid value for '--radius <R>'" + finite),
                          (("--radius", "nan", "--max-error", "1e-2"), "Invalid value for '--radius <R>'" + finite),
                          (("--radius", "wide", "--max-error", "1e-2"), "Invalid value for '--radius <radius>': invalid float literal"),
                          (("--radius", "0.5", "--max-error", "-1"), "Invalid value for '--max-error <X>'" + finite),
                          (("--radius", "0.5", "--max-error", "inf"), "Invalid value for '--max-error <X>'" + finite),
                          (("--radius", "0.5", "--max-error", "nan"), "Invalid value for '--max-error <X>'" + finite),
                          (("--radius", "0.5", "--max-error"), "requires a value but none was supplied"),
                          (("--radius", "0.5", "--max-error", "1e-2", "--min-fits", "1000001"), "Invalid value for '--min-fits <N>': expected an integer in 0 ... 1000000"),
                          (("--radius", "0.5", "--max-error", "1e-2", "--min-fits", "-1"), "Invalid value for '--min-fits <min-fits>': invalid digit found in string"),
                          (("--radius", "0.5", "--max-error", "1e-2", "--min-fits", "two"), "Invalid value for '--min-fits <min-fits>'")):
        r = subprocess.run([cli, "rematch", a, b] + list(args), capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
    assert not os.path.exists(b)
