"""The resident problem's device memory has one owner type ("Who owns it"): DevBuf<T>, defined once in csrc/capi.hip.
Every device array of struct c2b_problem and every temporary of csrc/capi_problem.hpp, the two headers split from it (capi_solve.hpp, capi_graph.hpp) and
csrc/capi_files.hpp is one, so none of them allocates or frees by hand: there is no free list to keep in step with the members, and a launch takes
the buffer as the typed pointer it holds.  What is held here is that it stays that way.  (That nothing leaks through
it on the device is tests/test_gpu_leak.py's.)"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "city2ba_amd", "csrc")
LEVEL1 = ("capi_problem.hpp", "capi_solve.hpp", "capi_graph.hpp", "capi_files.hpp")
DEFINITION = r"(?m)^template <class T>\nstruct DevBuf \{\n"


def _sources():
    return {p: open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if p.endswith((".hip", ".hpp", ".inc"))}


def _buffer_type(text):
    """the definition of DevBuf in `text`, from its `template` line to the closing brace in column 0 ("" if it has none)"""
    m = re.search(DEFINITION, text)
    return text[m.start():text.index("\n};\n", m.start()) + 4] if m else ""


def _outside_the_buffer_type(text):
    return text.replace(_buffer_type(text), "") if _buffer_type(text) else text


def test_the_buffer_type_is_defined_exactly_once():
    defs = [p for p, text in _sources().items() for _ in re.findall(r"\bstruct DevBuf\b", text)]
    assert defs == [os.path.join(CSRC, "capi.hip")], defs
    body = _buffer_type(open(defs[0]).read())
    # it owns by malloc / free, moves and never copies
    assert body.count("hipMalloc(") == 1 and body.count("hipFree(") == 1
    assert "DevBuf(const DevBuf &) = delete;" in body and "DevBuf &operator=(const DevBuf &) = delete;" in body
    assert "DevBuf(DevBuf &&o)" in body and "DevBuf &operator=(DevBuf &&o)" in body


def test_level_1_allocates_and_frees_through_the_buffer_type_alone():
    for name in LEVEL1:
        rest = _outside_the_buffer_type(open(os.path.join(CSRC, name)).read())
        for call in ("hipMalloc(", "hipFree("):
            lines = [ln.strip() for ln in rest.split("\n") if call in ln]
            assert not lines, (name, lines[:3])


def test_no_untyped_access_is_left():
    for name in LEVEL1:
        text = open(os.path.join(CSRC, name)).read()
        assert ".as<" not in text, name
        assert not re.findall(r"\bDevBuf\s+\w", text), name + ": a DevBuf without its element type"
