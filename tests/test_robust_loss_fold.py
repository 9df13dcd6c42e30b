"""The weighted passes of the robust losses are instances of the squared-loss kernels' own templates: each
pass over the observations in csrc/normal_kernels.hpp and csrc/schur_kernels.hpp carries a trailing parameter pack
`class... Loss`; empty, it is the squared-loss kernel, <..., int, double> takes (kind, a2) last and makes the one
loss_scale_obs call.  There is no second text to keep in step, so what is held here is that it stays that way: no copy
comes back, each pass is defined once, and the weighting is that one line and nothing else.  That both instances of
every pass compile to the registers they had as separate kernels is tests/test_isa_pins.py's."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "city2ba_amd", "csrc")

FOLDED = [("normal_kernels.hpp", "k_normal_cameras"), ("normal_kernels.hpp", "k_normal_points"),
          ("schur_kernels.hpp", "k_schur_points"), ("schur_kernels.hpp", "k_schur_cameras"),
          ("schur_kernels.hpp", "k_schur_jacobi"), ("schur_kernels.hpp", "k_schur_model")]
LOSS_LINE = "if constexpr (sizeof...(Loss) > 0) loss_scale_obs(loss..., r0, r1, jc, jp);"


def _sources():
    return {p: open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if p.endswith((".hip", ".hpp", ".inc"))}


def _kernel(text, name):
    """the definition of __global__ kernel `name`, from its `template` line to the closing brace in column 0"""
    m = re.search(r"(?m)^(template <[^>\n]*>\n)?__global__ [^\n]*\bvoid %s\(" % re.escape(name), text)
    assert m, name
    return text[m.start():text.index("\n}\n", m.start()) + 3]


def test_no_weighted_copy_of_a_kernel_exists():
    for path, text in _sources().items():
        assert not re.findall(r"\bk_\w+_loss\b", text), path


@pytest.mark.parametrize("header,name", FOLDED)
def test_pass_is_defined_once_and_weighted_by_one_line(header, name):
    defs = [p for p, text in _sources().items() for _ in re.findall(r"\bvoid %s\(" % name, text)]
    assert defs == [os.path.join(CSRC, header)], defs
    src = _kernel(open(os.path.join(CSRC, header)).read(), name)
    # the pack is the last template parameter and the last argument
    assert re.match(r"template <([^>\n]*, )?class\.\.\. Loss>\n", src), src.split("\n")[0]
    assert re.search(r",\s*Loss\.\.\. loss\) \{\n", src) and src.count("Loss... loss") == 1
    # one call, on the one line, the statement right after the one jacobian_obs call
    assert src.count("loss_scale_obs(") == 1 and src.count("jacobian_obs(") == 1
    assert [ln.strip() for ln in src.split("\n") if "loss_scale_obs(" in ln] == [LOSS_LINE]
    after = src[src.index("jacobian_obs("):]
    after = after[after.index(";") + 1:]
    assert after.lstrip().startswith(LOSS_LINE), after[:120]
    # and nothing else depends on the pack
    rest = src.replace(LOSS_LINE, "")
    assert len(re.findall(r"\bloss\b", rest)) == 1, "the pack is used by the one line alone"
    assert len(re.findall(r"\bLoss\b", rest)) == (3 if name == "k_normal_cameras" else 2)


def test_weighted_camera_pass_with_the_sum_cannot_be_instantiated():
    """k_normal_cameras<true, int, double> needs two scalar registers more than there are: the weighted sum of
    squares is k_robust_cost<true>'s, and the template refuses the instance"""
    src = _kernel(open(os.path.join(CSRC, "normal_kernels.hpp")).read(), "k_normal_cameras")
    assert src.count("static_assert(!(WITH_SUM && sizeof...(Loss) > 0),") == 1
