"""The explicit Schur complement's surface without a GPU: its nine symbols are declared in the experimental header alone with
the signatures the binding uses, C2B_SCHUR_LDS_BLOCKS is the binding's constant, and every refusal that needs no handle
answers before a device is touched and writes nothing (a bad kind, a shard and a problem without an upload need a handle, which
needs a device: tests/test_gpu_schur_explicit.py)."""
import ctypes as C
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("problem_set_schur", "problem_get_schur", "problem_schur_bytes", "problem_schur_complement", "problem_get_schur_pattern",
         "schur_y_rows", "schur_y_rows_loss", "schur_blocks_rows", "schur_spmv_rows")


def _lib_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_schur_explicit", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    return L


def _device_constant(name):
    import re
    text = open(os.path.join(ROOT, "city2ba_amd", "device.py")).read()
    return int(re.search(r"(?m)^%s = (\d+)" % name, text).group(1))


def test_signatures_match_the_header(tmp_path):
    L = _lib_table()
    src = tmp_path / "sx.c"
    src.write_text('#include <stdio.h>\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    int (*a)(c2b_problem *, int) = c2b_problem_set_schur;\n'
                   '    int (*b)(const c2b_problem *, int *) = c2b_problem_get_schur;\n'
                   '    int (*c)(c2b_problem *, int64_t *) = c2b_problem_schur_bytes;\n'
                   '    int (*d)(c2b_problem *, double, double *, double *, double *, int64_t *) = c2b_problem_schur_complement;\n'
                   '    int (*e)(c2b_problem *, uint64_t *, uint32_t *) = c2b_problem_get_schur_pattern;\n'
                   '    int (*f)(const double *, const double *, const uint32_t *, const uint32_t *, const double *, int64_t, const double *, double,\n'
                   '             double *, void *) = c2b_schur_y_rows;\n'
                   '    int (*g)(const double *, const double *, const uint32_t *, const uint32_t *, const double *, int64_t, const double *, double,\n'
                   '             double *, int, double, void *) = c2b_schur_y_rows_loss;\n'
                   '    int (*h)(const uint64_t *, const uint32_t *, const uint64_t *, const uint32_t *, const uint32_t *, int64_t, int64_t,\n'
                   '             const uint64_t *, const uint32_t *, const double *, double *, double *, void *) = c2b_schur_blocks_rows;\n'
                   '    int (*i)(const uint64_t *, const uint32_t *, int64_t, const double *, const double *, const double *, double *, double *,\n'
                   '             void *) = c2b_schur_spmv_rows;\n'
                   '    printf("%d %d %d %d %d\\n", C2B_SCHUR_IMPLICIT, C2B_SCHUR_EXPLICIT, C2B_SCHUR_LDS_BLOCKS, C2B_ABI_VERSION,\n'
                   '           a != 0 && b != 0 && c != 0 && d != 0 && e != 0 && f != 0 && g != 0 && h != 0 && i != 0);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "sx"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    blocks = _device_constant("SCHUR_LDS_BLOCKS")
    assert out.stdout.split() == [str(L.SCHUR_KINDS["implicit"]), str(L.SCHUR_KINDS["explicit"]), str(blocks), "10", "1"]
    assert 1 <= blocks and blocks * 648 <= 64 * 1024         # a static LDS array of the light kernel
    assert L.ABI_VERSION == 10                               # entries were only added
    assert L.SCHUR_NAMES == {v: k for k, v in L.SCHUR_KINDS.items()}
    vp, i64, i, d = C.c_void_p, C.c_int64, C.c_int, C.c_double
    assert L.SIGNATURES["c2b_problem_set_schur"] == (i, [vp, i])
    res, args = L.SIGNATURES["c2b_problem_get_schur"]
    assert res is i and args[0] is vp and args[1] is C.POINTER(i)
    res, args = L.SIGNATURES["c2b_problem_schur_bytes"]
    assert res is i and args[0] is vp and args[1] is C.POINTER(i64)
    res, args = L.SIGNATURES["c2b_problem_schur_complement"]
    assert res is i and args[:5] == [vp, d, vp, vp, vp] and args[5] is C.POINTER(i64)
    assert L.SIGNATURES["c2b_problem_get_schur_pattern"] == (i, [vp, vp, vp])
    assert L.SIGNATURES["c2b_schur_y_rows"] == (i, [vp] * 5 + [i64, vp, d, vp, vp])
    assert L.SIGNATURES["c2b_schur_y_rows_loss"] == (i, [vp] * 5 + [i64, vp, d, vp, i, d, vp])
    assert L.SIGNATURES["c2b_schur_blocks_rows"] == (i, [vp] * 5 + [i64, i64] + [vp] * 6)
    assert L.SIGNATURES["c2b_schur_spmv_rows"] == (i, [vp, vp, i64] + [vp] * 6)
    stable = open(os.path.join(ROOT, "include", "city2ba_hip.h")).read()
    exp = open(os.path.join(ROOT, "include", "city2ba_hip_experimental.h")).read()
    for name in NAMES:
        assert name in stable, name                          # the header index (tools/abi_index.py --write)
        assert " c2b_" + name + "(" not in stable            # declared in the experimental header alone
        assert " c2b_" + name + "(" in exp


def test_every_refusal_answers_without_a_device_and_writes_nothing():
    entry.build()
    from city2ba_amd import _lib as L
    lib = L.lib()
    buf = (C.c_uint64 * 64)(*([7] * 64))
    at = C.addressof(buf)
    err = lambda: lib.c2b_last_error()

    def y(camblk=at, pts4=at, cam_idx=at, pt_idx=at, uv=at, n_obs=2, V=at, lam=1e-2, Y=at, kind=None, scale=1.0):
        if kind is None:
            return lib.c2b_schur_y_rows(camblk, pts4, cam_idx, pt_idx, uv, n_obs, V, lam, Y, None)
        return lib.c2b_schur_y_rows_loss(camblk, pts4, cam_idx, pt_idx, uv, n_obs, V, lam, Y, kind, scale, None)

    for kw, word in ((dict(camblk=None), b"NULL"), (dict(pts4=None), b"NULL"), (dict(cam_idx=None), b"NULL"), (dict(pt_idx=None), b"NULL"),
                     (dict(uv=None), b"NULL"), (dict(V=None), b"NULL"), (dict(Y=None), b"NULL"), (dict(camblk=at + 8), b"misaligned"),
                     (dict(pts4=at + 8), b"misaligned"), (dict(uv=at + 8), b"misaligned"), (dict(cam_idx=at + 2), b"misaligned"),
                     (dict(pt_idx=at + 1), b"misaligned"), (dict(V=at + 4), b"misaligned"), (dict(Y=at + 4), b"misaligned"),
                     (dict(n_obs=-1), b"n_obs"), (dict(n_obs=1 << 31), b"n_obs"), (dict(lam=0.0), b"lambda"), (dict(lam=1e33), b"lambda"),
                     (dict(lam=float("nan")), b"lambda")):
        for kind in (None, 2):
            assert y(kind=kind, **kw) == L.ERR_INVALID_ARGUMENT and b"schur_y_rows" in err() and word in err(), (kw, kind, err())
    assert y(kind=4) == L.ERR_INVALID_ARGUMENT and b"loss" in err()
    assert y(kind=1, scale=0.0) == L.ERR_INVALID_ARGUMENT and b"loss" in err()

    def blocks(row_ptr=at, pt_idx=at, pt_row_ptr=at, obs_of=at, cam_of=at, n_cam=2, n_obs=2, nbr_ptr=at, nbr=at, Y=at, Sd=at, So=at):
        return lib.c2b_schur_blocks_rows(row_ptr, pt_idx, pt_row_ptr, obs_of, cam_of, n_cam, n_obs, nbr_ptr, nbr, Y, Sd, So, None)

    for kw, word in ((dict(row_ptr=None), b"NULL"), (dict(pt_idx=None), b"NULL"), (dict(pt_row_ptr=None), b"NULL"), (dict(obs_of=None), b"NULL"),
                     (dict(cam_of=None), b"NULL"), (dict(nbr_ptr=None), b"NULL"), (dict(Y=None), b"NULL"), (dict(Sd=None), b"NULL"),
                     (dict(n_cam=0), b"without cameras"), (dict(n_cam=-1), b"n_cam"), (dict(n_cam=1 << 31), b"n_cam"), (dict(n_obs=-1), b"n_obs"),
                     (dict(n_obs=(1 << 31) - 64), b"n_obs"), (dict(row_ptr=at + 4), b"misaligned"), (dict(pt_row_ptr=at + 4), b"misaligned"),
                     (dict(pt_idx=at + 2), b"misaligned"), (dict(obs_of=at + 1), b"misaligned"), (dict(cam_of=at + 2), b"misaligned"),
                     (dict(nbr_ptr=at + 4), b"misaligned"), (dict(nbr=at + 2), b"misaligned"), (dict(Y=at + 4), b"misaligned"),
                     (dict(Sd=at + 4), b"misaligned"), (dict(So=at + 4), b"misaligned")):
        assert blocks(**kw) == L.ERR_INVALID_ARGUMENT and b"schur_blocks_rows" in err() and word in err(), (kw, err())

    def spmv(nbr_ptr=at, nbr=at, n_cam=2, Sd=at, So=at, x=at, yv=at, part=at):
        return lib.c2b_schur_spmv_rows(nbr_ptr, nbr, n_cam, Sd, So, x, yv, part, None)

    for kw, word in ((dict(nbr_ptr=None), b"NULL"), (dict(Sd=None), b"NULL"), (dict(x=None), b"NULL"), (dict(yv=None), b"NULL"),
                     (dict(n_cam=-1), b"n_cam"), (dict(n_cam=1 << 31), b"n_cam"), (dict(nbr_ptr=at + 4), b"misaligned"), (dict(nbr=at + 2), b"misaligned"),
                     (dict(Sd=at + 4), b"misaligned"), (dict(So=at + 4), b"misaligned"), (dict(x=at + 4), b"misaligned"), (dict(yv=at + 4), b"misaligned"),
                     (dict(part=at + 4), b"misaligned")):
        assert spmv(**kw) == L.ERR_INVALID_ARGUMENT and b"schur_spmv_rows" in err() and word in err(), (kw, err())
    assert list(buf) == [7] * 64                             # nothing was written

    n, k = C.c_int64(-7), C.c_int(-7)
    assert lib.c2b_problem_set_schur(None, 1) == L.ERR_INVALID_ARGUMENT and b"problem_set_schur" in err() and b"NULL" in err()
    assert lib.c2b_problem_get_schur(None, C.byref(k)) == L.ERR_INVALID_ARGUMENT and b"NULL" in err()
    assert lib.c2b_problem_schur_bytes(None, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"NULL" in err()
    assert lib.c2b_problem_get_schur_pattern(None, at, at) == L.ERR_INVALID_ARGUMENT and b"problem_get_schur_pattern" in err() and b"NULL" in err()
    assert lib.c2b_problem_schur_complement(None, 1e-2, at, at, at, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"NULL" in err()
    assert (n.value, k.value) == (-7, -7) and list(buf) == [7] * 64
    import pytest
    for bad in ("jacobi", None, 1.5):
        with pytest.raises(ValueError):
            L.schur_kind(bad)
    assert L.schur_kind("explicit") == 1 and L.schur_kind("implicit") == 0 and L.schur_kind(1) == 1
