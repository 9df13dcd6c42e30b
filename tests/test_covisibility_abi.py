"""The covisibility entries' surface without a GPU: the seven symbols are declared in the experimental header alone with the
signatures the binding uses, the table size is the binding's and a power of two, and every refusal the header lists answers
before a device is touched and writes nothing."""
import ctypes as C
import os
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("covisibility_temp_bytes", "covisibility_degree_rows", "covisibility_fill_rows", "covisibility_expand_rows", "problem_covisibility",
         "problem_get_covisibility", "problem_neighbourhood")


def _lib_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_covis", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    return L


def _device_constant(name):
    import re
    text = open(os.path.join(ROOT, "city2ba_amd", "device.py")).read()
    return int(re.search(r"(?m)^%s = (\d+)" % name, text).group(1))


def test_signatures_match_the_header(tmp_path):
    L = _lib_table()
    src = tmp_path / "cv.c"
    src.write_text('#include <stdio.h>\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    int64_t (*a)(int64_t, int) = c2b_covisibility_temp_bytes;\n'
                   '    int (*b)(const uint64_t *, const uint32_t *, const uint64_t *, const uint32_t *, const uint32_t *, int64_t, int64_t, int64_t, int,\n'
                   '             void *, uint64_t *, int64_t *, void *) = c2b_covisibility_degree_rows;\n'
                   '    int (*c)(const uint64_t *, const uint32_t *, const uint64_t *, const uint32_t *, const uint32_t *, int64_t, int64_t, int64_t, int,\n'
                   '             void *, const uint64_t *, uint32_t *, uint32_t *, void *) = c2b_covisibility_fill_rows;\n'
                   '    int (*d)(const uint64_t *, const uint32_t *, const uint32_t *, int64_t, int, const uint8_t *, const uint32_t *, int64_t, int,\n'
                   '             int32_t *, uint32_t *, uint32_t *, void *, void *) = c2b_covisibility_expand_rows;\n'
                   '    int (*e)(c2b_problem *, int, int64_t *) = c2b_problem_covisibility;\n'
                   '    int (*f)(c2b_problem *, uint64_t *, uint32_t *, uint32_t *, int *, int64_t *) = c2b_problem_get_covisibility;\n'
                   '    int (*g)(c2b_problem *, const uint8_t *, int, int, int64_t, const uint8_t *, uint8_t *, int32_t *, int64_t *) = c2b_problem_neighbourhood;\n'
                   '    printf("%d %d %d %d %d\\n", C2B_COVIS_WAVE_SLOTS, C2B_COVIS_TEMP_GRAPH, C2B_COVIS_TEMP_EXPAND, C2B_ABI_VERSION,\n'
                   '           a != 0 && b != 0 && c != 0 && d != 0 && e != 0 && f != 0 && g != 0);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "cv"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    slots = _device_constant("COVIS_WAVE_SLOTS")
    assert out.stdout.split() == [str(slots), str(L.COVIS_TEMP_GRAPH), str(L.COVIS_TEMP_EXPAND), "10", "1"]
    assert slots >= 64 and slots & (slots - 1) == 0          # a power of two
    assert L.ABI_VERSION == 10                               # entries were only added
    vp, i64, i = C.c_void_p, C.c_int64, C.c_int
    assert L.SIGNATURES["c2b_covisibility_temp_bytes"] == (i64, [i64, i])
    assert L.SIGNATURES["c2b_covisibility_degree_rows"] == (i, [vp] * 5 + [i64, i64, i64, i] + [vp] * 4)
    assert L.SIGNATURES["c2b_covisibility_fill_rows"] == (i, [vp] * 5 + [i64, i64, i64, i] + [vp] * 5)
    assert L.SIGNATURES["c2b_covisibility_expand_rows"] == (i, [vp, vp, vp, i64, i, vp, vp, i64, i, vp, vp, vp, vp, vp])
    res, args = L.SIGNATURES["c2b_problem_covisibility"]
    assert res is i and args[:2] == [vp, i] and args[2] is C.POINTER(i64)
    res, args = L.SIGNATURES["c2b_problem_get_covisibility"]
    assert res is i and args[:4] == [vp] * 4 and args[4] is C.POINTER(i) and args[5] is C.POINTER(i64)
    res, args = L.SIGNATURES["c2b_problem_neighbourhood"]
    assert res is i and args[:8] == [vp, vp, i, i, i64, vp, vp, vp] and args[8] is C.POINTER(i64)
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
    assert lib.c2b_covisibility_temp_bytes(1000, L.COVIS_TEMP_GRAPH) > lib.c2b_covisibility_temp_bytes(1000, L.COVIS_TEMP_EXPAND) > 0
    assert lib.c2b_covisibility_temp_bytes(-5, L.COVIS_TEMP_GRAPH) == lib.c2b_covisibility_temp_bytes(0, L.COVIS_TEMP_GRAPH)
    buf = (C.c_uint64 * 64)(*([7] * 64))
    at = C.addressof(buf)
    good = dict(row_ptr=at, pt_idx=at, pt_row_ptr=at, obs_of=at, cam_of=at, n_cam=2, n_pts=2, n_obs=2, min_shared=1, temp=at, o1=at, o2=at, o3=at)

    def degree(**kw):
        a = dict(good, **kw)
        return lib.c2b_covisibility_degree_rows(a["row_ptr"], a["pt_idx"], a["pt_row_ptr"], a["obs_of"], a["cam_of"], a["n_cam"], a["n_pts"], a["n_obs"],
                                                a["min_shared"], a["temp"], a["o1"], a["o2"], None)

    def fill(**kw):
        a = dict(good, **kw)
        return lib.c2b_covisibility_fill_rows(a["row_ptr"], a["pt_idx"], a["pt_row_ptr"], a["obs_of"], a["cam_of"], a["n_cam"], a["n_pts"], a["n_obs"],
                                              a["min_shared"], a["temp"], a["o1"], a["o2"], a["o3"], None)

    cases = ((dict(min_shared=0), b"min_shared"), (dict(min_shared=-3), b"min_shared"), (dict(n_cam=1 << 31), b"n_cam"), (dict(n_cam=-1), b"n_cam"),
             (dict(n_obs=(1 << 31) - 64), b"n_obs"), (dict(n_obs=-1), b"n_obs"), (dict(row_ptr=None), b"NULL"), (dict(pt_idx=None), b"NULL"),
             (dict(pt_row_ptr=None), b"NULL"), (dict(obs_of=None), b"NULL"), (dict(cam_of=None), b"NULL"), (dict(temp=None), b"NULL"),
             (dict(o1=None), b"NULL"), (dict(row_ptr=at + 4), b"misaligned"), (dict(pt_row_ptr=at + 4), b"misaligned"), (dict(pt_idx=at + 2), b"misaligned"),
             (dict(obs_of=at + 1), b"misaligned"), (dict(cam_of=at + 2), b"misaligned"), (dict(temp=at + 8), b"misaligned"), (dict(o1=at + 4), b"misaligned"))
    for call, who in ((degree, b"covisibility_degree_rows"), (fill, b"covisibility_fill_rows")):
        for kw, word in cases:
            assert call(**kw) == L.ERR_INVALID_ARGUMENT, (who, kw)
            assert who in lib.c2b_last_error() and word in lib.c2b_last_error(), (kw, lib.c2b_last_error())
    assert degree(o2=None) == L.ERR_INVALID_ARGUMENT and b"NULL" in lib.c2b_last_error()
    assert degree(o2=at + 4) == L.ERR_INVALID_ARGUMENT and b"misaligned" in lib.c2b_last_error()
    assert fill(o2=at + 2) == L.ERR_INVALID_ARGUMENT and b"misaligned" in lib.c2b_last_error()
    assert fill(o3=at + 2) == L.ERR_INVALID_ARGUMENT and b"misaligned" in lib.c2b_last_error()

    def expand(nbr_ptr=at, nbr=at, shared=at, n_cam=2, min_shared=1, within=None, frontier=at, n_frontier=1, hop=0, level=at, nxt=at, n_next=at, temp=at):
        return lib.c2b_covisibility_expand_rows(nbr_ptr, nbr, shared, n_cam, min_shared, within, frontier, n_frontier, hop, level, nxt, n_next, temp, None)
    for kw, word in ((dict(min_shared=0), b"min_shared"), (dict(n_cam=1 << 31), b"n_cam"), (dict(n_frontier=3), b"n_frontier"), (dict(hop=-1), b"hop"),
                     (dict(nbr_ptr=None), b"NULL"), (dict(level=None), b"NULL"), (dict(nxt=None), b"NULL"), (dict(n_next=None), b"NULL"),
                     (dict(temp=None), b"NULL"), (dict(frontier=None), b"NULL"), (dict(nbr_ptr=at + 4), b"misaligned"), (dict(level=at + 2), b"misaligned"),
                     (dict(temp=at + 8), b"misaligned")):
        assert expand(**kw) == L.ERR_INVALID_ARGUMENT and word in lib.c2b_last_error(), (kw, lib.c2b_last_error())
    assert list(buf) == [7] * 64                             # nothing was written

    n = C.c_int64(-7)
    seed = (C.c_uint8 * 2)(1, 0)
    member, level = (C.c_uint8 * 2)(9, 9), (C.c_int32 * 2)(9, 9)
    assert lib.c2b_problem_covisibility(None, 1, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"NULL" in lib.c2b_last_error()
    assert lib.c2b_problem_get_covisibility(None, None, None, None, None, C.byref(n)) == L.ERR_INVALID_ARGUMENT and b"NULL" in lib.c2b_last_error()
    assert lib.c2b_problem_neighbourhood(None, seed, 1, 1, 0, None, member, level, C.byref(n)) == L.ERR_INVALID_ARGUMENT
    assert b"problem_neighbourhood" in lib.c2b_last_error() and b"NULL" in lib.c2b_last_error()
    assert (n.value, list(member), list(level)) == (-7, [9, 9], [9, 9])
