"""Which build of K1w a launch runs (csrc/k1w_builds.hpp select_k1w), on the CPU: csrc/host/k1w_select_check.cpp, built with g++ and
run from here. SITUATIONS is written by hand from README.md ("Two builds of one source") and the options' documentation - it is what
a launch must run, not a copy of the function. The program's own sweep over every value of every K1wChoice field checks that the
function is total, returns only builds its library has, and leaves no build of a library unselected. tests/test_k1w_builds_gpu.py
renders a dozen of the same situations and reads the build's name off the launch."""
import subprocess
from pathlib import Path

import pytest

import ipu_ray_lib_amd as irl

# the scene kinds: no vertex normals with pre-rotated leaf records (the built-in scenes), and vertex normals (test_scene.dae with normals)
FLAT, NORMALS = "hasNormals=0 rotLeaves=1", "hasNormals=1 rotLeaves=0"
V = "variants=1"
SITUATIONS = [
    # plain renders, default options
    ("flat scene", FLAT, "K1wPlainRot"),
    ("flat scene, leaf_rot 0", FLAT + " leafRot=0", "K1wPlainLean"),
    ("flat scene whose records were not rotated", "hasNormals=0 rotLeaves=0", "K1wPlainLean"),
    ("flat scene, lean_hit 0", FLAT + " leanHit=0", "K1wPlainBary"),
    ("vertex normals", NORMALS, "K1wPlainBary"),
    # NIF slots
    ("NIF, flat scene", FLAT + " slots=1", "K1wSlotsRot"),
    ("NIF, leaf_rot 0", FLAT + " slots=1 leafRot=0", "K1wSlotsLean"),
    ("NIF, lean_hit 0", FLAT + " slots=1 leanHit=0", "K1wSlotsBary"),
    ("NIF, vertex normals", NORMALS + " slots=1", "K1wSlotsBary"),
    # hot_nodes on: Rot and Bary have HOT builds, Lean has none; NIF launches never take them
    ("hot, flat scene", FLAT + " hotOn=1", "K1wHotRot"),
    ("hot, vertex normals", NORMALS + " hotOn=1", "K1wHotBary"),
    ("hot, lean_hit 0", FLAT + " hotOn=1 leanHit=0", "K1wHotBary"),
    ("hot, leaf_rot 0", FLAT + " hotOn=1 leafRot=0", "K1wPlainLean"),
    ("hot, NIF", FLAT + " hotOn=1 slots=1", "K1wSlotsRot"),
    # arithmetic and instrumented
    ("full_stats", FLAT + " stats=1", "K1wStats"),
    ("full_stats, hot", FLAT + " stats=1 hotOn=1", "K1wStatsHot"),
    ("full_stats, hot, NIF", FLAT + " stats=1 hotOn=1 slots=1", "K1wStats"),
    ("double_fallback", FLAT + " doubleFallback=1", "K1wDoubleFallback"),
    ("double_fallback, full_stats", FLAT + " doubleFallback=1 stats=1", "K1wDoubleFallbackStats"),
    ("fast", FLAT + " fast=1", "K1wFast"),
    ("fast, hot nodes on: the tier has one build", FLAT + " fast=1 hotOn=1", "K1wFast"),
    ("fast, NIF: refused", FLAT + " fast=1 slots=1", "refused: fast"),
    ("fast, full_stats: refused", FLAT + " fast=1 stats=1", "refused: fast"),
    # the variants library: the same defaults ...
    ("variants, flat scene", f"{V} {FLAT}", "K1wPlainRot"),
    ("variants, hot, vertex normals", f"{V} {NORMALS} hotOn=1", "K1wHotBary"),
    ("variants, full_stats", f"{V} {FLAT} stats=1", "K1wStats"),
    # ... and the families that were measured and not made the default
    ("spec", f"{V} {FLAT} specLeaf=1", "K1wSpec5"),
    ("spec, full_stats", f"{V} {FLAT} specLeaf=1 stats=1", "K1wSpecStats4"),
    ("weights, 6 waves", f"{V} {FLAT} defaultWeights=0", "K1wWeights6"),
    ("weights, 5 waves", f"{V} {FLAT} defaultWeights=0 wavesPerSimd=5", "K1wWeights5"),
    ("merge 0", f"{V} {FLAT} mergeTurns=0", "K1wTwoTurns"),
    ("merge 0, NIF", f"{V} {FLAT} mergeTurns=0 slots=1", "K1wTwoTurnsSlots"),
    ("waves 7", f"{V} {FLAT} wavesPerSimd=7", "K1wWaves7"),
    # (seven waves have no NIF build and the default form is asked for by waves = 6 alone: what is left is the build of every default, as before)
    ("waves 7, NIF", f"{V} {FLAT} wavesPerSimd=7 slots=1", "K1wWaves4"),
    ("waves 5", f"{V} {FLAT} wavesPerSimd=5", "K1wWaves5"),
    ("waves 5, NIF", f"{V} {FLAT} wavesPerSimd=5 slots=1", "K1wWaves5Slots"),
    ("waves 4", f"{V} {FLAT} wavesPerSimd=4", "K1wWaves4"),
    ("kernel 2", f"{V} {FLAT} kernelChoice=2", "K1wLdsPrefix"),
    ("kernel 2, full_stats", f"{V} {FLAT} kernelChoice=2 stats=1", "K1wLdsPrefixStats"),
    ("kernel 2, NIF: kernel 1", f"{V} {FLAT} kernelChoice=2 slots=1", "K1wSlotsRot"),
    ("kernel 2, empty tree: kernel 1", f"{V} {FLAT} kernelChoice=2 hasNodes=0", "K1wPlainRot"),
    ("kernel 3", f"{V} {FLAT} kernelChoice=3", "path pool"),
    ("kernel 3, NIF", f"{V} {FLAT} kernelChoice=3 slots=1", "path pool"),
    ("kernel 3 past the pool's limits: kernel 1", f"{V} {FLAT} kernelChoice=3 poolFits=0", "K1wPlainRot"),
    # precedence: double_fallback before everything, fast next, then the variants-only branches in their order
    ("double_fallback over kernel 3, spec, weights, merge, waves", f"{V} {FLAT} doubleFallback=1 kernelChoice=3 specLeaf=1 defaultWeights=0 mergeTurns=0 wavesPerSimd=5", "K1wDoubleFallback"),
    ("double_fallback over fast", f"{V} {FLAT} doubleFallback=1 fast=1", "K1wDoubleFallback"),
    ("fast over kernel 3, spec, weights", f"{V} {FLAT} fast=1 kernelChoice=3 specLeaf=1 defaultWeights=0", "K1wFast"),
    ("kernel 3 over spec", f"{V} {FLAT} kernelChoice=3 specLeaf=1", "path pool"),
    ("kernel 2 over spec", f"{V} {FLAT} kernelChoice=2 specLeaf=1", "K1wLdsPrefix"),
    ("spec over weights, merge, waves", f"{V} {FLAT} specLeaf=1 defaultWeights=0 mergeTurns=0 wavesPerSimd=7", "K1wSpec5"),
    ("weights over merge and waves 7", f"{V} {FLAT} defaultWeights=0 mergeTurns=0 wavesPerSimd=7", "K1wWeights5"),
    ("merge over waves 7", f"{V} {FLAT} mergeTurns=0 wavesPerSimd=7", "K1wTwoTurns"),
    ("full_stats over weights, merge, waves", f"{V} {FLAT} stats=1 defaultWeights=0 mergeTurns=0 wavesPerSimd=5", "K1wStats"),
    # the shipped library has none of those options: whatever the fields say, it runs its own builds
    ("shipped, variants-only fields set", f"{FLAT} kernelChoice=3 specLeaf=1 defaultWeights=0 mergeTurns=0 wavesPerSimd=4", "K1wPlainRot"),
]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("k1w") / "k1w_select_check"
    src = Path(irl.REPO_ROOT) / "ipu_ray_lib_amd" / "csrc" / "host" / "k1w_select_check.cpp"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", str(exe), str(src)], check=True)
    return exe


def test_every_named_situation_runs_its_build(checker):
    out = subprocess.run([str(checker), "-"], input="".join(fields + "\n" for _, fields, _ in SITUATIONS), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(SITUATIONS)
    wrong = [f"{what}: {have}, not {want}" for (what, _, want), have in zip(SITUATIONS, got) if have != want]
    assert not wrong, "\n".join(wrong)


def test_sweep_of_every_choice(checker):
    out = subprocess.run([str(checker)], capture_output=True, text=True)
    assert out.returncode == 0 and "k1w_select_check OK" in out.stdout, out.stdout + out.stderr
