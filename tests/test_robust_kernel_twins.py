"""The weighted kernels of the robust losses (k_*_loss in csrc/normal_kernels.hpp and csrc/schur_kernels.hpp) are copies
of the squared-loss kernels' text with one line added, because the squared-loss kernels are pinned to the code they
compiled to before losses existed.  Nothing but this test keeps a copy in step with its original: each
twin, with its added line, its name and its two extra arguments taken out, must be its original's text -- for
k_normal_cameras_loss the original without the sum of squares, whose every fragment is listed here."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "city2ba_amd", "csrc")

# what k_normal_cameras carries for its sum of squares and its twin does not (each must occur exactly once)
CAMERA_SUM = [
    "template <bool WITH_SUM>\n",
    "    double ssq = 0.0;                                                // lane gl == 0 of a group: its cameras' sums, in order\n",
    ", sq = 0.0;",
    "            sq += r0 * r0 + r1 * r1;\n",
    "            sq += __shfl_xor(sq, off, 64);\n",
    "            ssq += sq;\n",
    "    if (WITH_SUM) {                                                  // one partial per wave\n"
    "        const double w = wave_sum(ssq);\n"
    "        if (lane == 0) block_part[blockIdx.x * kWaves + wave] = w;\n"
    "    }\n",
    ",\n    double *__restrict__ block_part) {",
]


def _kernel(text, name):
    """the definition of __global__ kernel `name`, from its `template` line (if any) to the closing brace in column 0"""
    m = re.search(r"(?m)^(template <[^>\n]*>\n)?__global__ [^\n]*\bvoid %s\(" % re.escape(name), text)
    assert m, name
    return text[m.start():text.index("\n}\n", m.start()) + 3]


def _strip_twin(src, name, arg):
    """the twin as its original would read: name, the loss_scale_obs line and the (kind, a2) arguments removed"""
    assert src.count("void %s_loss(" % name) == 1
    src = src.replace("void %s_loss(" % name, "void %s(" % name)
    lines = [ln for ln in src.split("\n") if "loss_scale_obs(" not in ln]
    assert len(lines) == src.count("\n") + 1 - 1, "exactly one loss_scale_obs line"
    src = "\n".join(lines)
    m = re.search(r",\s*int kind, double %s\) \{" % arg, src)
    assert m and len(re.findall(r"int kind", src)) == 1
    return src[:m.start()] + ") {" + src[m.end():]


@pytest.mark.parametrize("header,name,arg", [("normal_kernels.hpp", "k_normal_points", "a2"),
                                             ("schur_kernels.hpp", "k_schur_points", "la2"),
                                             ("schur_kernels.hpp", "k_schur_cameras", "la2"),
                                             ("schur_kernels.hpp", "k_schur_model", "la2")])
def test_weighted_twin_is_its_original_plus_one_line(header, name, arg):
    text = open(os.path.join(CSRC, header)).read()
    want = _kernel(text, name)
    got = _strip_twin(_kernel(text, name + "_loss"), name, arg)
    assert "jacobian_obs(" in want and re.sub(r"\s+", " ", got) == re.sub(r"\s+", " ", want)


def test_weighted_camera_pass_is_the_original_without_its_sum():
    text = open(os.path.join(CSRC, "normal_kernels.hpp")).read()
    want = _kernel(text, "k_normal_cameras")
    for frag in CAMERA_SUM[:-1]:
        assert want.count(frag) == 1, frag
        want = want.replace(frag, ";" if frag == CAMERA_SUM[2] else "")
    assert want.count(CAMERA_SUM[-1]) == 1
    want = want.replace(CAMERA_SUM[-1], ") {")
    assert not re.search(r"\b(ssq|sq|WITH_SUM|block_part)\b", want)
    got = _strip_twin(_kernel(text, "k_normal_cameras_loss"), "k_normal_cameras", "a2")
    assert re.sub(r"\s+", " ", got) == re.sub(r"\s+", " ", want)
