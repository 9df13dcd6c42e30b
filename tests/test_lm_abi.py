"""The three structs of c2b_problem_levenberg_marquardt as a C99 compiler lays them out against the ctypes.Structure
layouts city2ba_amd/_lib.py passes for them: size and every field's offset."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"c2b_lm_options": ("LmOptions", {}), "c2b_lm_iteration": ("LmIteration", {"lambda": "lam"}), "c2b_lm_summary": ("LmSummary", {})}
C_FIELDS = {
    "c2b_lm_options": ("max_iterations", "pcg_max_iters", "lambda0", "pcg_rel_tol", "function_tol", "gradient_tol", "parameter_tol"),
    "c2b_lm_iteration": ("cost", "cost_trial", "lambda", "model_decrease", "gradient_max", "step_norm", "x_norm", "pcg_rel_residual",
                         "accepted", "pcg_iterations", "status", "reserved"),
    "c2b_lm_summary": ("iterations", "termination", "initial_cost", "final_cost", "lambda_next"),
}


def test_struct_layouts_match_the_binding(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("_c2b_lib_layout", os.path.join(ROOT, "city2ba_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)                               # the table of signatures alone: no library is loaded
    lines = []
    for name, fields in C_FIELDS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f in fields:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "city2ba_hip_experimental.h"\nint main(void) {\n    %s\n    return 0;\n}\n'
                   % "\n    ".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = dict(ln.split() for ln in out.stdout.splitlines())
    for name, (cls_name, rename) in STRUCTS.items():
        cls = getattr(L, cls_name)
        assert int(got[name]) == C.sizeof(cls), name
        assert [rename.get(f, f) for f in C_FIELDS[name]] == [f for f, _ in cls._fields_], name
        for f in C_FIELDS[name]:
            assert int(got["%s.%s" % (name, f)]) == getattr(cls, rename.get(f, f)).offset, (name, f)
    assert int(got["c2b_lm_iteration"]) == 80 and int(got["c2b_lm_options"]) == 48 and int(got["c2b_lm_summary"]) == 32
