"""The direct solver's surface without a GPU: its six symbols are declared in the experimental header alone with the signatures the
binding uses, the three constants are the binding's, C2B_ABI_VERSION stays 10, and every refusal that needs no handle answers
before a device is touched and writes nothing (a shard, the cap and a problem without an upload need a handle, which needs a
device: tests/test_gpu_dense_solver.py)."""
import ctypes as C
import os
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("problem_set_linear_solver", "problem_get_linear_solver", "problem_linear_solver_bytes", "dense_scatter_rows", "dense_cholesky",
         "dense_cholesky_solve")


def _lib_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_dense_solver", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    return L


def _device_constant(name):
    import re
    text = open(os.path.join(ROOT, "city2ba_amd", "device.py")).read()
    return int(re.search(r"(?m)^%s = (\d+)" % name, text).group(1))


def test_signatures_match_the_header(tmp_path):
    L = _lib_table()
    src = tmp_path / "dn.c"
    src.write_text('#include <stdio.h>\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    int (*a)(c2b_problem *, int) = c2b_problem_set_linear_solver;\n'
                   '    int (*b)(const c2b_problem *, int *) = c2b_problem_get_linear_solver;\n'
                   '    int (*c)(c2b_problem *, int64_t *) = c2b_problem_linear_solver_bytes;\n'
                   '    int (*d)(const uint64_t *, const uint32_t *, int64_t, const double *, const double *, double *, int64_t, void *) =\n'
                   '        c2b_dense_scatter_rows;\n'
                   '    int (*e)(double *, int64_t, int64_t, int32_t *, void *) = c2b_dense_cholesky;\n'
                   '    int (*f)(const double *, int64_t, int64_t, double *, void *) = c2b_dense_cholesky_solve;\n'
                   '    printf("%d %d %d %d %d\\n", C2B_LINEAR_PCG, C2B_LINEAR_CHOLESKY, C2B_DENSE_MAX_CAMERAS, C2B_ABI_VERSION,\n'
                   '           a != 0 && b != 0 && c != 0 && d != 0 && e != 0 && f != 0);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "dn"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0", "1", "4096", "10", "1"]
    assert (L.LINEAR_KINDS["pcg"], L.LINEAR_KINDS["cholesky"], L.DENSE_MAX_CAMERAS) == (0, 1, 4096)
    assert _device_constant("DENSE_MAX_CAMERAS") == 4096
    assert L.ABI_VERSION == 10                               # entries were only added
    assert L.LINEAR_NAMES == {v: k for k, v in L.LINEAR_KINDS.items()}
    vp, i64, i = C.c_void_p, C.c_int64, C.c_int
    assert L.SIGNATURES["c2b_problem_set_linear_solver"] == (i, [vp, i])
    res, args = L.SIGNATURES["c2b_problem_get_linear_solver"]
    assert res is i and args[0] is vp and args[1] is C.POINTER(i)
    res, args = L.SIGNATURES["c2b_problem_linear_solver_bytes"]
    assert res is i and args[0] is vp and args[1] is C.POINTER(i64)
    assert L.SIGNATURES["c2b_dense_scatter_rows"] == (i, [vp, vp, i64, vp, vp, vp, i64, vp])
    assert L.SIGNATURES["c2b_dense_cholesky"] == (i, [vp, i64, i64, vp, vp])
    assert L.SIGNATURES["c2b_dense_cholesky_solve"] == (i, [vp, i64, i64, vp, vp])
    stable = open(os.path.join(ROOT, "include", "city2ba_hip.h")).read()
    exp = open(os.path.join(ROOT, "include", "city2ba_hip_experimental.h")).read()
    for name in NAMES:
        assert name in stable, name                          # the header index (tools/abi_index.py --write)
        assert " c2b_" + name + "(" not in stable            # declared in the experimental header alone
        assert " c2b_" + name + "(" in exp
    # c2b_step_info and c2b_lm_options did not change
    assert [f[0] for f in L.StepInfo._fields_] == ["iterations", "status", "rel_residual", "sum_sq", "model_decrease"]
    assert C.sizeof(L.StepInfo) == 32 and C.sizeof(L.LmOptions) == 48


def test_every_refusal_answers_without_a_device_and_writes_nothing():
    entry.build()
    from city2ba_amd import _lib as L
    lib = L.lib()
    buf = (C.c_uint64 * 64)(*([7] * 64))
    at = C.addressof(buf)
    err = lambda: lib.c2b_last_error()

    def scatter(nbr_ptr=at, nbr=at, n_cam=2, Sd=at, So=at, A=at, ld=64):
        return lib.c2b_dense_scatter_rows(nbr_ptr, nbr, n_cam, Sd, So, A, ld, None)

    for kw, word in ((dict(nbr_ptr=None), b"NULL"), (dict(Sd=None), b"NULL"), (dict(A=None), b"NULL"), (dict(n_cam=-1), b"n_cam"),
                     (dict(n_cam=1 << 31), b"n_cam"), (dict(n_cam=4097, ld=9 * 4096), b"C2B_DENSE_MAX_CAMERAS"), (dict(nbr_ptr=at + 4), b"misaligned"),
                     (dict(nbr=at + 2), b"misaligned"), (dict(Sd=at + 4), b"misaligned"), (dict(So=at + 4), b"misaligned"), (dict(A=at + 4), b"misaligned"),
                     (dict(ld=63), b"multiple of 64"), (dict(ld=65), b"multiple of 64"), (dict(ld=-64), b"out of range"), (dict(ld=64 * 577), b"out of range"),
                     (dict(n_cam=8, ld=64), b"exceeds ld")):
        assert scatter(**kw) == L.ERR_INVALID_ARGUMENT and b"dense_scatter_rows" in err() and word in err(), (kw, err())

    def factor(A=at, n=5, ld=64, info=at):
        return lib.c2b_dense_cholesky(A, n, ld, info, None)

    for kw, word in ((dict(A=None), b"NULL"), (dict(info=None), b"NULL"), (dict(A=at + 4), b"misaligned"), (dict(info=at + 2), b"misaligned"),
                     (dict(ld=63), b"multiple of 64"), (dict(ld=100), b"multiple of 64"), (dict(n=65), b"exceeds ld"), (dict(n=-1), b"out of range"),
                     (dict(ld=-64), b"out of range"), (dict(ld=64 * 577), b"out of range")):
        assert factor(**kw) == L.ERR_INVALID_ARGUMENT and b"dense_cholesky" in err() and word in err(), (kw, err())

    def solve(A=at, n=5, ld=64, x=at):
        return lib.c2b_dense_cholesky_solve(A, n, ld, x, None)

    for kw, word in ((dict(A=None), b"NULL"), (dict(x=None), b"NULL"), (dict(A=at + 4), b"misaligned"), (dict(x=at + 4), b"misaligned"),
                     (dict(ld=63), b"multiple of 64"), (dict(n=65), b"exceeds ld"), (dict(n=-1), b"out of range"), (dict(ld=64 * 577), b"out of range")):
        assert solve(**kw) == L.ERR_INVALID_ARGUMENT and b"dense_cholesky_solve" in err() and word in err(), (kw, err())
    assert list(buf) == [7] * 64                             # nothing was written

    n, k = C.c_int64(-7), C.c_int(-7)
    assert lib.c2b_problem_set_linear_solver(None, 1) == L.ERR_INVALID_ARGUMENT and b"problem_set_linear_solver" in err() and b"NULL" in err()
    assert lib.c2b_problem_get_linear_solver(None, C.byref(k)) == L.ERR_INVALID_ARGUMENT and b"NULL" in err()
    assert lib.c2b_problem_linear_solver_bytes(None, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"NULL" in err()
    assert (n.value, k.value) == (-7, -7) and list(buf) == [7] * 64
    for bad in ("dense", "Cholesky", None, 1.5):
        with pytest.raises(ValueError):
            L.linear_kind(bad)
    assert L.linear_kind("cholesky") == 1 and L.linear_kind("pcg") == 0 and L.linear_kind(1) == 1 and L.linear_kind(2) == 2
