"""The cheaper forms of K1w's SHADE / GEN turn in csrc/ray_math.h - the two bounded-range sincos (sincos_deg_table_small, _turn) and
the dielectric bounce on per-material constants (dielectric_consts, dielectric_with) - against the forms they stand in for, bit for bit: csrc/host/shade_consts_check.cpp, built and run from here. No GPU needed; the device's
shift-add scrambler of rng_next is checked by tests/test_shade_consts_gpu.py."""
import subprocess
from pathlib import Path

import ipu_ray_lib_amd as irl


def test_cheaper_forms_equal_the_forms_they_replace_bit_for_bit(tmp_path):
    root = Path(irl.REPO_ROOT)
    exe = tmp_path / "shade_consts_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-pthread", "-o", str(exe),
                    str(root / "ipu_ray_lib_amd" / "csrc" / "host" / "shade_consts_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "shade_consts_check OK" in out.stdout, out.stdout + out.stderr
