"""The triangle test of csrc/tri_math.hpp - the error bound's minima as min_abs3, and the form that leaves out the verdicts t itself
carries (POS) - against the oracle's o_ray_shear + o_intersect_triangle, with o_set_double_fallback 0 and 1: csrc/host/tri_verdict_check.cpp,
built with the library's exact flags and run from here on oracle/libray_oracle.so, which it loads. 6e7 cases per setting; what is compared
and on which inputs is written at the head of that file. No GPU needed; the kernels' side is tests/test_tri_verdict_gpu.py."""
import subprocess
from pathlib import Path

import ipu_ray_lib_amd as irl
import oracle_lib


def test_triangle_test_equals_the_oracle_bit_for_bit_and_pos_form_is_accepted_alike(tmp_path):
    root = Path(irl.REPO_ROOT)
    oracle_lib.lib()      # (raises when the oracle is not built)
    exe = tmp_path / "tri_verdict_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-pthread", "-o", str(exe),
                    str(root / "ipu_ray_lib_amd" / "csrc" / "host" / "tri_verdict_check.cpp"), "-ldl"], check=True)
    out = subprocess.run([str(exe), str(oracle_lib.ORACLE_SO)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "tri_verdict_check OK" in out.stdout, out.stdout + out.stderr
