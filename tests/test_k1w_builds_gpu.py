"""The launch says which build of K1w it ran (pytest -m gpu): a dozen of the situations of tests/test_k1w_builds.py rendered, each with
say_grid set. The launch's line on stderr must name the build the situation calls for (csrc/k1w_builds.hpp), and every byte of the
stream must be the oracle's - a wrong pick is otherwise silent, every build being exact. The tolerance tier (fast) is compared with a
second render of itself. The NIF-slot builds are left to the NIF tests of test_gpu_parity.py, which have an oracle for them."""
import re
from pathlib import Path

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
import oracle_lib as ol
from test_gpu_parity import assert_streams_identical

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 3
HOT = 32          # nodes staged by the HOT builds (clamped to the tree); 0 = the shared arrays


def _stream(desc):
    import ctypes as C
    rays = np.zeros(desc.num_rays, dtype=irl.TRACE_RESULT)
    irl.host_lib().mi_init_ray_stream(C.byref(desc), rays.ctypes.data, rays.size)
    return rays


@pytest.fixture(scope="module")
def scenes():
    """name -> (scene, desc, the oracle's stream, the oracle's stream under double_fallback); the scenes are kept: the descs point into them"""
    out = {}
    for name, s in (("box", irl.HostScene.builtin("box")),
                    ("normals", irl.HostScene.import_file(Path(irl.REPO_ROOT) / "assets" / "test_scene.dae", load_normals=True))):
        d = s.desc
        d.set_image(W, H); d.samples_per_pixel = SPP; d.path_trace = 1
        want, want_df = _stream(d), _stream(d)
        ol.path_trace_pixel_rng(d, want, 16)
        with ol.double_fallback():
            ol.path_trace_pixel_rng(d, want_df, 16)
        for a in (want, want_df):
            a.setflags(write=False)
        out[name] = (s, d, want, want_df)
    return out


def _render(scene_desc, capfd, variants, options):
    dev = irl.IpuScene(scene_desc, variants=variants).set_option("say_grid", 1)
    for k, v in options.items():
        dev.set_option(k, v)
    got = _stream(scene_desc)
    capfd.readouterr()
    dev.run(got, irl.MODE_PATH_TRACE)
    said = re.findall(r"mi_raylib: grid .*, build (\w+)", capfd.readouterr().err)
    dev.close()
    return got, said


CASES = [
    # (what, scene, variants library, options, the build)
    ("flat scene", "box", False, {"hot_nodes": 0}, "K1wPlainRot"),
    ("flat scene, leaf_rot 0", "box", False, {"hot_nodes": 0, "leaf_rot": 0}, "K1wPlainLean"),
    ("flat scene, lean_hit 0", "box", False, {"hot_nodes": 0, "lean_hit": 0}, "K1wPlainBary"),
    ("vertex normals", "normals", False, {"hot_nodes": 0}, "K1wPlainBary"),
    ("hot, flat scene", "box", False, {"hot_nodes": HOT}, "K1wHotRot"),
    ("hot, vertex normals", "normals", False, {"hot_nodes": HOT}, "K1wHotBary"),
    ("hot, leaf_rot 0: Lean has no HOT build", "box", False, {"hot_nodes": HOT, "leaf_rot": 0}, "K1wPlainLean"),
    ("full_stats", "box", False, {"hot_nodes": 0, "full_stats": 1}, "K1wStats"),
    ("full_stats, hot", "box", False, {"hot_nodes": HOT, "full_stats": 1}, "K1wStatsHot"),
    ("double_fallback", "normals", False, {"double_fallback": 1}, "K1wDoubleFallback"),
    ("spec", "box", True, {"spec": 1}, "K1wSpec5"),
    ("merge 0", "box", True, {"merge": 0}, "K1wTwoTurns"),
    ("waves 7", "box", True, {"waves": 7}, "K1wWaves7"),
]


@pytest.mark.parametrize("what,scene,variants,options,build", CASES, ids=[c[0] for c in CASES])
def test_the_launch_names_its_build_and_the_stream_is_the_oracles(scenes, capfd, what, scene, variants, options, build):
    _, d, want, want_df = scenes[scene]
    got, said = _render(d, capfd, variants, options)
    assert said == [build], f"{what}: the launch said {said}"
    assert_streams_identical(got, want_df if options.get("double_fallback") else want, what)


def test_fast_names_its_build_and_repeats_itself(scenes, capfd):
    _, d, _, _ = scenes["box"]
    first, said = _render(d, capfd, False, {"fast": 1})
    assert said == ["K1wFast"]
    again, said = _render(d, capfd, False, {"fast": 1})
    assert said == ["K1wFast"]
    assert_streams_identical(again, first, "fast, rendered twice")
