"""The boundary of the priors (c2b_problem_set_priors ... c2b_prior_model_rows): the entries exist under a new
ABI number and answer a NULL handle without a device.  What the priors do to the step is tests/test_gpu_priors.py."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("c2b_problem_set_priors", "c2b_problem_get_priors", "c2b_problem_prior_cost", "c2b_problem_prior_residual_jacobian",
               "c2b_prior_cameras_rows", "c2b_prior_points_rows", "c2b_prior_model_rows")


def _parent_abi_version():
    """C2B_ABI_VERSION of the parent commit's header, or None where the history is not there to ask"""
    try:
        old = subprocess.run(["git", "show", "HEAD~:include/city2ba_hip.h"], cwd=ROOT, capture_output=True, text=True, timeout=30)
    except (OSError, subprocess.SubprocessError):
        return None
    m = re.search(r"(?m)^#define C2B_ABI_VERSION (\d+)", old.stdout) if old.returncode == 0 else None
    return int(m.group(1)) if m else None


def test_library_exports_the_prior_entries_under_a_new_abi_number():
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
    assert version >= 10 and (parent is None or version >= parent)
    if parent is not None and parent < 10:
        assert version > parent
    # without a device the handle cannot exist; the argument checks that need none still answer
    assert raw.c2b_problem_set_priors(None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert raw.c2b_problem_get_priors(None, None, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert raw.c2b_problem_prior_cost(None, None) == _lib.ERR_INVALID_ARGUMENT
    assert raw.c2b_problem_prior_residual_jacobian(None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    # the Level-0 passes refuse a target without its weights before they look at a device
    raw.c2b_prior_points_rows.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 8
    one = (C.c_double * 4)()
    assert raw.c2b_prior_points_rows(None, 1, one, None, None, None, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT


def test_python_surface_names_the_priors():
    from city2ba_amd import device as D, solve as S
    from city2ba_amd.baproblem import BAProblem
    import inspect
    for name in ("set_priors", "priors", "prior_cost", "prior_residual_jacobian"):
        assert hasattr(BAProblem, name), name
    assert list(inspect.signature(BAProblem.set_priors).parameters)[1:] == [
        "camera_centers", "camera_center_weights", "intrinsics", "intrinsics_weights", "points", "point_weights"]
    for f in (S.levenberg_marquardt, S.levenberg_marquardt_device):
        assert "priors" in inspect.signature(f).parameters
    for name in ("prior_cameras_rows", "prior_points_rows", "prior_model_rows"):
        assert callable(getattr(D, name)), name
