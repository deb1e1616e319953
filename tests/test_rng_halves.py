"""rotl64 on the two 32-bit halves (csrc/ray_math.h; two v_alignbit_b32 on the device) against the plain 64-bit rotation, and rng_next over it
against a copy of the generator on the plain form: csrc/host/rotl_halves_check.cpp, built with the library's exact flags and run from here - and
once more as a stand-alone program under -fsanitize=address,undefined. What is compared and on which values is written at the head of that file.
No GPU needed; on the device every render test that compares a frame with the oracle runs the same text."""
import subprocess
from pathlib import Path

import pytest

import ipu_ray_lib_amd as irl

SRC = Path(irl.REPO_ROOT) / "ipu_ray_lib_amd" / "csrc" / "host" / "rotl_halves_check.cpp"


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_halves_rotation_and_generator_equal_the_plain_form(tmp_path, extra):
    exe = tmp_path / "rotl_halves_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", *extra, "-o", str(exe), str(SRC)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and "rotl_halves_check OK" in out.stdout and "differences 0" in out.stdout, out.stdout + out.stderr
