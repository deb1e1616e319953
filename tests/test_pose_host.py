"""Rigid poses on the host (no GPU): mi_pose_geometry_host - the twin of the pose pass of mi_scene_set_poses* - against the numpy
restatement of the header (pose_cases.PoseChecker) byte for byte, against exact cases (the 24 cube rotations, scaled quaternions,
powers of two, the identity), its refusals, a binary64 reference with a bound set from the checker, and the refit of the posed
arrays."""
import math

import numpy as np
import pytest

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import id_cases as ic
import obox_cases as oc
import pose_cases as po
import refit_cases as rc

F = np.float32
SCENES = ("soup", "soup-normals", "spheres", "box", "many_geoms")
SEEDS = {"soup": range(6), "soup-normals": range(6), "spheres": range(6), "box": range(6), "many_geoms": (1,)}
# The bound of test_float64_reference: k x 2^-24 x (scale (|x| + |y| + |z|) + |t_k|). Over the seeded set above the CHECKER's largest
# ratio is 5.79 (many_geoms: 65 535 poses; 3.20 on the four small scenes); doubled and rounded up to a power of two: 16. The margin is
# for the rounding of the nine frame entries, which the eight operations of the point formula do not count.
K_BOUND = 16


def scene(name):
    return ic.scene(name) if name == "many_geoms" else rc.scene(name)


def twin(hs, poses):
    return irl.pose_geometry_host(hs.desc, poses)


def refused(desc, poses, words):
    with pytest.raises(irl.RaylibError) as e:
        irl.pose_geometry_host(desc, poses)
    msg = str(e.value)
    assert "failed (1)" in msg and "mi_pose_geometry_host" in msg and words in msg, msg
    return msg


@pytest.mark.parametrize("name", SCENES)
def test_twin_equals_the_checker(name):
    hs = scene(name)
    ck = po.PoseChecker(hs.desc)
    G = hs.desc.num_geometry
    for seed in SEEDS[name]:
        p = po.seeded_poses(hs, seed)
        po.assert_arrays_equal(twin(hs, p), ck.apply(p), f"{name}, seed {seed}")
    # the hand-placed poses, each on one geometry among seeded ones; an invalid one is refused by its index
    base = po.seeded_poses(hs, 77)
    for k, (what, (row, valid)) in enumerate(po.HAND.items()):
        p = base.copy()
        g = (k * 7) % G
        p[g] = po.pose_row(row)[0]
        assert bool(ck.valid(p)[g]) == valid, what
        if valid:
            po.assert_arrays_equal(twin(hs, p), ck.apply(p), f"{name}, {what}")
        else:
            refused(hs.desc, p, f"pose {g} is not valid")
            with pytest.raises(po.Refused, match=f"pose {g} is not valid"):
                ck.apply(p)
    # a translation far outside is a valid pose: the twin moves the geometry, the refit refuses it
    p = po.with_pose(G, 0, po.TOO_FAR)
    a = twin(hs, p)
    po.assert_arrays_equal(a, ck.apply(p), f"{name}, far translation")
    if G > 1:
        with pytest.raises(irl.RaylibError, match="Cannot compress BVH bounds into fp16"):
            po.with_arrays(hs, a)


def test_cube_rotations_are_exact():
    hs = oc.dyadic_scene()
    rest = po.arrays_of(hs.desc)
    G = hs.desc.num_geometry
    assert rest["vertices"].size and rest["spheres"].size and rest["discs"].size
    for q, R in po.cube_poses():
        got = twin(hs, qb.make_poses(G, quat=np.tile(np.array(q, F), (G, 1))))
        want = {k: v.copy() for k, v in rest.items()}
        for kind, names in (("vertices", "xyz"), ("spheres", "xyz"), ("discs", ("cx", "cy", "cz")), ("discs", ("nx", "ny", "nz"))):
            p = np.stack([rest[kind][n] for n in names], 1).astype(np.int64)
            assert np.array_equal(p, np.stack([rest[kind][n] for n in names], 1)), "small integers"
            r = p @ R.T
            for k, n in enumerate(names):
                want[kind][n] = r[:, k]
        for kind in po.KINDS:      # (numerically: the bytes may differ in the sign of a zero, a sum like 0 x + (-1) 0)
            for n in want[kind].dtype.names:
                assert np.array_equal(got[kind][n], want[kind][n]), (q, kind, n)
        assert np.array_equal(got["spheres"]["radius"], rest["spheres"]["radius"]) and np.array_equal(got["discs"]["r"], rest["discs"]["r"])


@pytest.mark.parametrize("name", ("soup-normals", "spheres"))
def test_scaled_quaternion_gives_the_same_bytes(name):
    hs = scene(name)
    p = po.seeded_poses(hs, 5)
    big = p.copy()
    big["quat"] *= F(1024.0)
    small = p.copy()
    small["quat"] *= F(2.0 ** -30)
    want = twin(hs, p)
    po.assert_arrays_equal(twin(hs, big), want, "quaternions x 1024")
    po.assert_arrays_equal(twin(hs, small), want, "quaternions x 2^-30")


def test_power_of_two_scale_is_ldexp():
    hs = scene("soup-normals")
    rest = po.arrays_of(hs.desc)
    G = hs.desc.num_geometry
    for e in (-3, -1, 1, 3, 10):
        got = twin(hs, qb.make_poses(G, scale=F(2.0 ** e)))
        for kind, moved, kept in (("vertices", "xyz", ()), ("normals", (), "xyz"), ("spheres", ("x", "y", "z", "radius"), ()),
                                  ("discs", ("cx", "cy", "cz", "r"), ("nx", "ny", "nz"))):
            for n in moved:
                assert np.array_equal(got[kind][n], np.ldexp(rest[kind][n], e)), (e, kind, n)
            for n in kept:
                assert np.array_equal(got[kind][n], rest[kind][n]), (e, kind, n)


def test_identity_keeps_every_byte():
    hs = scene("soup-normals")
    rest = {k: v.copy() for k, v in po.arrays_of(hs.desc).items()}
    # -0 coordinates, and a NaN: an identity pose copies, it does not compute
    rest["vertices"]["x"][::5] = F(-0.0)
    rest["normals"]["y"][::3] = F(-0.0)
    rest["spheres"]["z"][0] = F(-0.0)
    rest["discs"]["ny"][0] = F(-0.0)
    rest["vertices"]["z"][7] = np.nan
    d = irl.SceneDesc.from_buffer_copy(hs.desc)
    d.mesh_verts, d.mesh_normals, d.spheres, d.discs = (rest[k].ctypes.data for k in po.KINDS)
    G = d.num_geometry
    for what in ("identity", "identity -0"):
        p = np.tile(po.pose_row(po.HAND[what][0]), G)
        po.assert_arrays_equal(irl.pose_geometry_host(d, p), rest, what)
    # (computed, -0 x 1 + 0 is +0: a pose one ulp off the identity does change those bytes)
    near = qb.make_poses(G, scale=np.nextafter(F(1), F(2)))
    assert irl.pose_geometry_host(d, near)["vertices"].tobytes() != rest["vertices"].tobytes()


def test_unowned_records_stay():
    e = po.edge("unowned")
    rest = po.arrays_of(e.desc)
    ck = po.PoseChecker(e.desc)
    own = ck.derive_owners()
    assert (own["vertices"] == po.UNOWNED).sum() == 4 and own["vertices"][0] == po.UNOWNED and own["vertices"][-1] == po.UNOWNED
    assert (own["spheres"] == po.UNOWNED).sum() == 2
    p = po.seeded_poses(e, 9)
    got = twin(e, p)
    po.assert_arrays_equal(got, ck.apply(p), "unowned")
    for kind in ("vertices", "spheres"):
        free = own[kind] == po.UNOWNED
        assert got[kind][free].tobytes() == rest[kind][free].tobytes(), kind
        assert (got[kind][~free] != rest[kind][~free]).all(), kind


def test_posing_from_rest_does_not_drift():
    hs = scene("soup-normals")
    a, b = po.seeded_poses(hs, 1), po.seeded_poses(hs, 2)
    once = twin(hs, b)
    twin(hs, a)
    po.assert_arrays_equal(twin(hs, b), once, "B after A")
    # (what drifting would look like: B applied to A's result is another scene)
    moved = po.with_arrays(hs, twin(hs, a))
    assert irl.pose_geometry_host(moved.desc, b)["vertices"].tobytes() != once["vertices"].tobytes()


def test_ownership_conflicts_are_refused_by_name():
    hs = scene("soup")
    view = irl.HostScene._view
    G = hs.desc.num_geometry
    p = qb.make_poses(G)
    # two meshes whose vertex ranges intersect
    info = view(None, hs.desc.mesh_info, hs.desc.num_meshes, irl.MESH_INFO).copy()
    info[1]["firstVertex"] -= 1
    d = irl.SceneDesc.from_buffer_copy(hs.desc)
    d.mesh_info = info.ctypes.data
    msg = refused(d, p, "the vertex ranges of geometries 0 and 1 intersect")
    assert f"vertex {int(info[1]['firstVertex'])}" in msg
    with pytest.raises(po.Refused, match="vertex ranges of geometries 0 and 1 intersect"):
        po.PoseChecker(d).apply(p)
    # one mesh, one sphere referenced by two geometry entries
    geom = view(None, hs.desc.geometry, G, irl.GEOM_REF).copy()
    assert [int(t) for t in geom["type"]] == [0, 0, 1, 2]
    for g, kind in ((1, "mesh"), (3, "sphere")):
        twice = geom.copy()
        twice[g] = twice[g - 1] if kind == "mesh" else twice[2]
        d = irl.SceneDesc.from_buffer_copy(hs.desc)
        d.geometry = twice.ctypes.data
        first = g - 1 if kind == "mesh" else 2
        refused(d, p, f"geometries {first} and {g} both reference {kind} {int(twice[g]['index'])}")
        with pytest.raises(po.Refused, match=f"geometries {first} and {g} both reference {kind}"):
            po.PoseChecker(d).apply(p)
    # nothing was written by a refused call, and the counts are checked
    refused(hs.desc, qb.make_poses(G + 1), "num_geometry differs")
    refused(hs.desc, qb.make_poses(G - 1), "num_geometry differs")


def test_float64_reference():
    worst_checker, worst_twin = 0.0, 0.0
    for name in SCENES:
        hs = scene(name)
        ck = po.PoseChecker(hs.desc)
        for seed in SEEDS[name]:
            p = po.seeded_poses(hs, seed)
            worst_checker = max(worst_checker, po.worst_ratio(ck, p, ck.apply(p)))
            worst_twin = max(worst_twin, po.worst_ratio(ck, p, twin(hs, p)))
    k = 2 ** math.ceil(math.log2(2.0 * worst_checker))
    print(f"largest ratio: checker {worst_checker:.3f}, twin {worst_twin:.3f}; k = {k}")
    assert k == K_BOUND, f"the checker's largest ratio {worst_checker} sets k = {k}, the test records {K_BOUND}"
    assert worst_twin <= K_BOUND, f"a posed coordinate lies {worst_twin} x 2^-24 x (scale (|x| + |y| + |z|) + |t_k|) from the reference"


@pytest.mark.parametrize("name", ("soup", "soup-normals", "spheres"))
def test_refit_nodes_of_the_posed_scene(name):
    hs = scene(name)
    p = po.seeded_poses(hs, 3)
    p["translation"] *= F(0.25)
    got = po.posed(hs, p)
    want_arrays = po.PoseChecker(hs.desc).apply(p)
    d = irl.SceneDesc.from_buffer_copy(hs.desc)
    for key, ptr in (("vertices", "mesh_verts"), ("normals", "mesh_normals"), ("spheres", "spheres"), ("discs", "discs")):
        if want_arrays[key].size:
            setattr(d, ptr, want_arrays[key].ctypes.data)
    rc.assert_nodes_equal(got.nodes, rc.numpy_refit(d, hs.nodes), f"{name}: refit of the posed scene")
    assert got.nodes.tobytes() != hs.nodes.tobytes()
