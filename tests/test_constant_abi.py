"""The boundary of the constant-parameter masks (c2b_problem_set_constant / c2b_problem_get_constant): the
entries exist under a new ABI number, answer a NULL handle without a device, and solve.py names the bits as the header
does.  What the masks do to the step is tests/test_gpu_constant.py."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("c2b_problem_set_constant", "c2b_problem_get_constant")
BITS = dict(ROTATION=0x007, TRANSLATION=0x038, POSE=0x03f, FOCAL=0x040, K1=0x080, K2=0x100, INTRINSICS=0x1c0, ALL=0x1ff)


def _parent_abi_version():
    """C2B_ABI_VERSION of the parent commit's header, or None where the history is not there to ask"""
    try:
        old = subprocess.run(["git", "show", "HEAD~:include/city2ba_hip.h"], cwd=ROOT, capture_output=True, text=True, timeout=30)
    except (OSError, subprocess.SubprocessError):
        return None
    m = re.search(r"(?m)^#define C2B_ABI_VERSION (\d+)", old.stdout) if old.returncode == 0 else None
    return int(m.group(1)) if m else None


def test_library_exports_the_constant_entries_under_a_new_abi_number():
    import __graft_entry__ as entry
    entry.build()
    from city2ba_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW_ENTRIES:
        assert hasattr(raw, n), "library does not export " + n
        assert n in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "city2ba_hip.h")).read()
    version = int(re.search(r"(?m)^#define C2B_ABI_VERSION (\d+)", header).group(1))
    raw.c2b_abi_version.restype = C.c_int
    assert raw.c2b_abi_version() == version == _lib.ABI_VERSION
    parent = _parent_abi_version()
    # the commit that adds the entries raises the number; a later commit's parent already carries it
    assert version >= 9 and (parent is None or version >= parent)
    if parent is not None and parent < 9:
        assert version > parent
    # without a device the handle cannot exist; the argument checks that need none still answer
    assert raw.c2b_problem_set_constant(None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert raw.c2b_problem_get_constant(None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT


def test_bit_constants_are_the_headers():
    from city2ba_amd import solve
    exp = open(os.path.join(ROOT, "include", "city2ba_hip_experimental.h")).read()
    for name, value in BITS.items():
        assert getattr(solve, name) == value, name
        m = re.search(r"(?m)^#define C2B_CONST_%s (0x[0-9a-fA-F]+)$" % name, exp)
        assert m and int(m.group(1), 16) == value, name
    assert solve.ROTATION | solve.TRANSLATION == solve.POSE and solve.FOCAL | solve.K1 | solve.K2 == solve.INTRINSICS
    assert solve.POSE | solve.INTRINSICS == solve.ALL and solve.POSE & solve.INTRINSICS == 0
