"""The alignment entries' surface without a GPU: the symbols are declared in the experimental header alone with the
signatures and structures the binding uses, the header index lists them, Level 1's device memory is the one buffer type's, and every
refusal of Levels 0 and 1 answers before a device is touched and writes nothing."""
import ctypes as C
import os
import re
import subprocess

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("align_options_init", "similarity_from_moments", "align_finish_moments", "align_launch_shape", "align_means_rows", "align_moments_rows",
         "align_errors_rows", "align_rotation_errors_rows", "similarity_apply", "problem_align", "problem_transform")


def test_signatures_and_structures_match_the_header(tmp_path):
    entry.build()
    from city2ba_amd import _lib as L
    src = tmp_path / "al.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "city2ba_hip_experimental.h"\n'
                   'int main(void) {\n'
                   '    void (*a)(c2b_align_options *) = c2b_align_options_init;\n'
                   '    int (*b)(int64_t, const double *, const double *, double, double, const double *, int, c2b_similarity *, int *) = c2b_similarity_from_moments;\n'
                   '    int (*c)(const double *, const double *, double *, double *, double *, double *, double *, double *) = c2b_align_finish_moments;\n'
                   '    int (*d)(int *, int *, int *) = c2b_align_launch_shape;\n'
                   '    int (*e)(const double *, const double *, const uint8_t *, int64_t, const double *, const double *, const uint8_t *, int64_t, void *, double *,\n'
                   '             void *) = c2b_align_means_rows;\n'
                   '    int (*f)(const double *, const double *, const uint8_t *, int64_t, const double *, const double *, const uint8_t *, int64_t, const double *,\n'
                   '             void *, double *, void *) = c2b_align_moments_rows;\n'
                   '    int (*g)(const double *, const double *, int64_t, const c2b_similarity *, const uint8_t *, const uint8_t *, double, double *, uint8_t *, void *,\n'
                   '             double *, void *) = c2b_align_errors_rows;\n'
                   '    int (*h)(const double *, const double *, int64_t, const c2b_similarity *, const uint8_t *, double *, void *, double *, void *) =\n'
                   '        c2b_align_rotation_errors_rows;\n'
                   '    int (*i)(double *, int64_t, double *, int64_t, const c2b_similarity *, void *) = c2b_similarity_apply;\n'
                   '    int (*j)(c2b_problem *, c2b_problem *, const c2b_align_options *, c2b_similarity *, c2b_align_summary *, double *, double *, double *,\n'
                   '             uint8_t *, uint8_t *) = c2b_problem_align;\n'
                   '    int (*k)(c2b_problem *, const c2b_similarity *) = c2b_problem_transform;\n'
                   '    c2b_align_options o;\n'
                   '    c2b_align_options_init(&o);\n'
                   '    printf("%d %d %d %d %d %d %d ", C2B_ALIGN_CAMERAS, C2B_ALIGN_POINTS, C2B_ALIGN_BOTH, C2B_ALIGN_OK, C2B_ALIGN_TOO_FEW, C2B_ALIGN_DEGENERATE,\n'
                   '           C2B_ABI_VERSION);\n'
                   '    printf("%d %d %d %d %d ", (int)sizeof(c2b_similarity), (int)sizeof(c2b_align_options), (int)sizeof(c2b_align_stat),\n'
                   '           (int)sizeof(c2b_align_summary), (int)offsetof(c2b_align_summary, points));\n'
                   '    printf("%d %d %d %g %d %d\\n", o.on, o.scale, o.rounds, o.max_dist, o.use_cam == 0 && o.use_pt == 0,\n'
                   '           a != 0 && b != 0 && c != 0 && d != 0 && e != 0 && f != 0 && g != 0 && h != 0 && i != 0 && j != 0 && k != 0);\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "al"
    libdir = os.path.dirname(entry.build_hip())
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + libdir, "-lcity2ba_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    want = [L.ALIGN_ON["cameras"], L.ALIGN_ON["points"], L.ALIGN_ON["both"], L.ALIGN_OK, L.ALIGN_TOO_FEW, L.ALIGN_DEGENERATE, 10,
            C.sizeof(L.Similarity), C.sizeof(L.AlignOptions), C.sizeof(L.AlignStat), C.sizeof(L.AlignSummary), L.AlignSummary.points.offset,
            1, 1, 0, 0, 1, 1]                                # the defaults: cameras, with scale, one fit, no trimming, no masks
    assert [float(v) for v in out.stdout.split()] == [float(v) for v in want]
    assert L.ABI_VERSION == 10                               # entries were only added
    assert C.sizeof(L.Similarity) == 13 * 8
    vp, i64, i, d = C.c_void_p, C.c_int64, C.c_int, C.c_double
    assert L.SIGNATURES["c2b_align_means_rows"] == (i, [vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp])
    assert L.SIGNATURES["c2b_align_moments_rows"] == (i, [vp, vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp])
    assert L.SIGNATURES["c2b_align_errors_rows"] == (i, [vp, vp, i64, vp, vp, vp, d, vp, vp, vp, vp, vp])
    assert L.SIGNATURES["c2b_align_rotation_errors_rows"] == (i, [vp, vp, i64, vp, vp, vp, vp, vp, vp])
    assert L.SIGNATURES["c2b_similarity_apply"] == (i, [vp, i64, vp, i64, vp, vp])
    assert L.SIGNATURES["c2b_problem_align"] == (i, [vp] * 10)
    assert L.SIGNATURES["c2b_problem_transform"] == (i, [vp, vp])
    stable = open(os.path.join(ROOT, "include", "city2ba_hip.h")).read()
    exp = open(os.path.join(ROOT, "include", "city2ba_hip_experimental.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\b" % name, stable), name      # the header index (tools/abi_index.py --write)
        assert " c2b_" + name + "(" not in stable            # declared in the experimental header alone
        assert " c2b_" + name + "(" in exp
    assert L.align_launch_shape() == (256, 256, 4)


def test_level_1_of_the_alignment_owns_device_memory_through_the_buffer_type_alone():
    """what tests/test_device_buffer_ownership.py holds for the other Level 1 headers, for csrc/capi_align.hpp"""
    text = open(os.path.join(ROOT, "city2ba_amd", "csrc", "capi_align.hpp")).read()
    for call in ("hipMalloc(", "hipFree(", "hipMallocAsync(", "hipFreeAsync("):
        assert call not in text, call
    assert ".as<" not in text and not re.findall(r"\bDevBuf\s+\w", text) and "struct DevBuf" not in text
    assert len(re.findall(r"\bDevBuf<(?:uint8_t|double)>", text)) >= 2
    kernels = open(os.path.join(ROOT, "city2ba_amd", "csrc", "align_kernels.hpp")).read()
    assert "atomicAdd" not in kernels and "atomic_fetch_add" not in kernels        # no float atomics: the one fetch_add is ticket_arrive's


def test_every_refusal_answers_without_a_device_and_writes_nothing():
    entry.build()
    from city2ba_amd import _lib as L
    lib = L.lib()
    buf = (C.c_double * 64)(*([7.0] * 64))                   # (64-byte aligned or better by the allocator; checked below)
    raw = (C.c_char * 1024)()
    at = (C.addressof(raw) + 127) & ~127                     # a 128-byte aligned address inside raw: tables, workspace, results
    sim = L.similarity(1.0, [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0])
    ps = C.addressof(sim)
    err = lib.c2b_last_error

    def means(xc=at, yc=at, uc=None, nc=2, xp=at, yp=at, up=None, np_=2, ws=at, out=at + 256):
        return lib.c2b_align_means_rows(xc, yc, uc, nc, xp, yp, up, np_, ws, out, None)

    def moments(xc=at, yc=at, uc=None, nc=2, xp=at, yp=at, up=None, np_=2, ws=at, out=at + 256, mean=at + 512):
        return lib.c2b_align_moments_rows(xc, yc, uc, nc, xp, yp, up, np_, mean, ws, out, None)
    cases = ((dict(nc=-1), b"negative"), (dict(np_=-1), b"negative"), (dict(xc=None), b"NULL"), (dict(yc=None), b"NULL"), (dict(xp=None), b"NULL"),
             (dict(yp=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(out=None), b"NULL"), (dict(xc=at + 8), b"misaligned"), (dict(yc=at + 8), b"misaligned"),
             (dict(xp=at + 8), b"misaligned"), (dict(yp=at + 8), b"misaligned"), (dict(ws=at + 64), b"misaligned"), (dict(out=at + 4), b"misaligned"))
    for call, who in ((means, b"align_means_rows"), (moments, b"align_moments_rows")):
        for kw, word in cases:
            assert call(**kw) == L.ERR_INVALID_ARGUMENT, (who, kw)
            assert who in err() and word in err(), (kw, err())
    assert moments(mean=None) == L.ERR_INVALID_ARGUMENT and b"means7" in err()
    assert moments(mean=at + 4) == L.ERR_INVALID_ARGUMENT and b"means7" in err()

    def errors(x=at, y=at, n=2, T=ps, base=None, use=None, md=0.0, e=at + 256, nxt=None, ws=at, out=at + 512):
        return lib.c2b_align_errors_rows(x, y, n, T, base, use, md, e, nxt, ws, out, None)
    for kw, word in ((dict(n=-1), b"negative"), (dict(x=None), b"NULL"), (dict(y=None), b"NULL"), (dict(T=None), b"NULL"), (dict(ws=None), b"NULL"),
                     (dict(out=None), b"NULL"), (dict(x=at + 8), b"misaligned"), (dict(y=at + 8), b"misaligned"), (dict(e=at + 4), b"misaligned"),
                     (dict(out=at + 4), b"misaligned"), (dict(ws=at + 64), b"misaligned"), (dict(use=at + 700, nxt=at + 700), b"next must not be use"),
                     (dict(md=float("nan")), b"NaN")):
        assert errors(**kw) == L.ERR_INVALID_ARGUMENT and b"align_errors_rows" in err() and word in err(), (kw, err())

    def rot(x=at, y=at, n=2, T=ps, use=None, e=at + 256, ws=at, out=at + 512):
        return lib.c2b_align_rotation_errors_rows(x, y, n, T, use, e, ws, out, None)
    for kw, word in ((dict(n=-1), b"negative"), (dict(x=None), b"NULL"), (dict(y=None), b"NULL"), (dict(T=None), b"NULL"), (dict(ws=None), b"NULL"),
                     (dict(out=None), b"NULL"), (dict(x=at + 4), b"misaligned"), (dict(y=at + 4), b"misaligned"), (dict(e=at + 4), b"misaligned"),
                     (dict(ws=at + 64), b"misaligned")):
        assert rot(**kw) == L.ERR_INVALID_ARGUMENT and b"align_rotation_errors_rows" in err() and word in err(), (kw, err())

    def apply(cam=at, nc=1, pts=at, np_=1, T=ps):
        return lib.c2b_similarity_apply(cam, nc, pts, np_, T, None)
    mirror = L.similarity(1.0, [1, 0, 0, 0, 1, 0, 0, 0, -1], [0, 0, 0])
    skew = L.similarity(1.0, [1, 1e-8, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0])
    bad = [(L.similarity(0.0, [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0]), b"scale must be > 0"), (L.similarity(-2.0, [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0]), b"scale must be > 0"),
           (L.similarity(float("inf"), [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0]), b"not finite"), (L.similarity(1.0, [1, 0, 0, 0, float("nan"), 0, 0, 0, 1], [0, 0, 0]), b"not finite"),
           (L.similarity(1.0, [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, float("inf"), 0]), b"not finite"), (mirror, b"reflection"), (skew, b"not orthonormal")]
    for kw, word in ((dict(nc=-1), b"negative"), (dict(np_=-1), b"negative"), (dict(cam=None), b"NULL"), (dict(pts=None), b"NULL"), (dict(T=None), b"NULL"),
                     (dict(cam=at + 4), b"misaligned"), (dict(pts=at + 8), b"misaligned")) + tuple((dict(T=C.addressof(T)), w) for T, w in bad):
        assert apply(**kw) == L.ERR_INVALID_ARGUMENT and b"similarity_apply" in err() and word in err(), (kw, err())
    assert raw.raw == b"\0" * 1024 and list(buf) == [7.0] * 64             # nothing was written

    # Level 1: no handle exists without a device; a NULL one is refused before anything is read or written
    o = L.AlignOptions()
    lib.c2b_align_options_init(C.byref(o))
    S = L.AlignSummary()
    S.status = 9
    T = L.similarity(3.0, [1, 0, 0, 0, 1, 0, 0, 0, 1], [1, 2, 3])
    assert lib.c2b_problem_align(None, None, C.byref(o), C.byref(T), C.byref(S), None, None, None, None, None) == L.ERR_INVALID_ARGUMENT
    assert b"problem_align" in err() and b"NULL" in err()
    assert (S.status, T.scale, list(T.translation)) == (9, 3.0, [1.0, 2.0, 3.0])
    assert lib.c2b_problem_transform(None, C.byref(T)) == L.ERR_INVALID_ARGUMENT and b"problem_transform" in err() and b"NULL" in err()
