"""Shared by the id-range tests (test_id_range_host.py, test_id_range_gpu.py): two scenes that reach the upper half of both ids -
many_geoms (65 535 geometries, geomIDs up to 0xFFFE) and long_mesh (130 050 triangles in one mesh, primIDs past 65 536) -, each built
once per process by numpy alone, and THE CLOSED FORMS: because both scenes are grids, which (geomID, primID) a box, a point, a
query triangle or a vertical ray of a cell must return, and in which order, follows from integer arithmetic on the cell's number.
No geometry code of the project is used for that, so neither the device nor its host twin can share a bug with it. Where an order
needs a distance (neighbours) it is computed in binary64 from the arrays the scenes were built from (point_cases.tri_dist64 and
the sphere / disc formulas of point_cases.brute_force, restricted to the candidates the grid admits).

The Python checkers of the other families (near_cases.NearChecker, box_cases.BoxChecker, tri_cases.TriChecker, count_cases.Checker,
list_cases.ListChecker) resolve every node in a Python loop when they are made: seconds for a quarter of a million nodes. Here they
are made by their `lazy` constructors."""
import ctypes as C

import numpy as np

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import oracle_lib as ol
import point_cases as pc

F = np.float32

# ------------------------------------------------------------------------------------------------------
# many_geoms: 65 535 geometries of one primitive each, point_cases.hand_scene's order (triangles, spheres, discs)
# ------------------------------------------------------------------------------------------------------
G = 0xFFFF                      # geometries: geomIDs 0 .. 0xFFFE
PER_KIND = G // 3               # 21 845 one-triangle meshes, spheres, discs
CELLS, GRID_X, GRID_Y = 8192, 128, 64
LAYERS, LAYER_Z = 8, 0.25
N_MATS = 19                     # more than the 16 a workgroup stages in LDS
PROBE = (0.15, 0.15)            # where a cell's vertical probes stand: inside its triangles (x + y < .5), its spheres' and discs' xy

_cache = {}


def kind_of(g):
    """0 triangle, 1 sphere, 2 disc."""
    return int(g) // PER_KIND


def stack(cell):
    """The geomIDs stacked in a cell, bottom layer first: cell + 8192 k."""
    return [cell + CELLS * k for k in range(LAYERS) if cell + CELLS * k < G]


def cell_xy(cell):
    return cell % GRID_X, cell // GRID_X


def mat_of(g):
    g = np.asarray(g, np.int64)
    return (g + (g >> 13)) % N_MATS


def materials19():
    """19 materials with distinct albedos; 5 is specular, 11 a dielectric, 0 emits."""
    m = np.zeros(N_MATS, irl.MATERIAL)
    k = np.arange(N_MATS)
    m["albedo"]["x"] = (0.15 + 0.04 * k).astype(F)
    m["albedo"]["y"] = (0.9 - 0.035 * k).astype(F)
    m["albedo"]["z"] = (0.2 + 0.03 * ((7 * k) % N_MATS)).astype(F)
    m["ior"] = 1.5
    m["type"][5], m["type"][11] = 1, 2
    m["emission"]["x"][0] = m["emission"]["y"][0] = m["emission"]["z"][0] = 2.0
    m["emissive"][0] = 1
    return m


def geometry_desc(tri_verts=None, spheres=None, discs=None, mats=None, mat_ids=None, mesh=None):
    """A geometry-only SceneDesc (what HostScene.from_arrays takes) over numpy arrays, which it keeps alive in ._keep: tri_verts
    [T, 3, 3] float32 = one mesh of one triangle each; or mesh = (verts [V, 3] float32, tris [T, 3] uint16) = one mesh; spheres
    [S] SPHERE; discs [D] DISC."""
    if mesh is not None:
        verts, idx = np.asarray(mesh[0], F), np.ascontiguousarray(mesh[1], np.uint16)
        info = np.zeros(1, irl.MESH_INFO)
        info[0] = (0, 0, len(idx), len(verts))
    else:
        nt = 0 if tri_verts is None else len(tri_verts)
        verts = np.asarray(tri_verts, F).reshape(-1, 3) if nt else np.zeros((0, 3), F)
        idx = np.tile(np.arange(3, dtype=np.uint16), (nt, 1))
        info = np.zeros(nt, irl.MESH_INFO)
        info["firstIndex"], info["firstVertex"], info["numTriangles"], info["numVertices"] = np.arange(nt), 3 * np.arange(nt), 1, 3
    v = np.zeros(len(verts), irl.VEC3)
    v["x"], v["y"], v["z"] = verts[:, 0], verts[:, 1], verts[:, 2]
    sph = np.zeros(0, irl.SPHERE) if spheres is None else np.ascontiguousarray(spheres, irl.SPHERE)
    dsc = np.zeros(0, irl.DISC) if discs is None else np.ascontiguousarray(discs, irl.DISC)
    ng = len(info) + len(sph) + len(dsc)
    if mats is None:
        mats = np.zeros(1, irl.MATERIAL)
        mats["ior"] = 1.5
    if mat_ids is None:
        mat_ids = np.zeros(max(ng, 1), np.uint32)
    mat_ids = np.ascontiguousarray(mat_ids, np.uint32)
    g = irl.SceneDesc()
    ptr = lambda a: a.ctypes.data if len(a) else None
    g.mesh_info, g.num_meshes = ptr(info), len(info)
    g.mesh_tris, g.num_tris = ptr(idx), len(idx)
    g.mesh_verts, g.num_verts = ptr(v), len(v)
    g.mat_ids, g.num_mat_ids = mat_ids.ctypes.data, ng
    g.materials, g.num_materials = mats.ctypes.data, len(mats)
    g.spheres, g.num_spheres = ptr(sph), len(sph)
    g.discs, g.num_discs = ptr(dsc), len(dsc)
    g.fov_radians = 0.9
    g._keep = [info, idx, v, sph, dsc, mats, mat_ids]
    return g


def _origins(g):
    g = np.asarray(g, np.int64)
    cell = g % CELLS
    return np.stack([cell % GRID_X, cell // GRID_X, LAYER_Z * (g // CELLS)], 1).astype(F)      # (every value is exact in binary32)


def many_geoms_arrays(shift=(0.0, 0.0, 0.0)):
    """(tri_verts [21845, 3, 3], spheres, discs, materials, mat_ids): the arrays many_geoms is built from (shift: see VIEW)."""
    if ("mg-arrays", shift) not in _cache:
        org = _origins(np.arange(G)) + np.array(shift, F)
        t = org[:PER_KIND]
        tv = np.stack([t, t + np.array([.5, 0, 0], F), t + np.array([0, .5, 0], F)], 1).astype(F)
        s = org[PER_KIND:2 * PER_KIND] + np.array([.25, .25, .05], F)
        sph = np.zeros(PER_KIND, irl.SPHERE)
        sph["x"], sph["y"], sph["z"], sph["radius"] = s[:, 0], s[:, 1], s[:, 2], F(0.2)
        d = org[2 * PER_KIND:] + np.array([.25, .25, .1], F)
        dsc = np.zeros(PER_KIND, irl.DISC)
        dsc["nz"], dsc["r"] = 1.0, F(0.3)
        dsc["cx"], dsc["cy"], dsc["cz"] = d[:, 0], d[:, 1], d[:, 2]
        _cache[("mg-arrays", shift)] = (tv, sph, dsc, materials19(), mat_of(np.arange(G)).astype(np.uint32))
    return _cache[("mg-arrays", shift)]


def many_geoms(shift=(0.0, 0.0, 0.0)):
    if ("mg", shift) not in _cache:
        tv, sph, dsc, mats, mat_ids = many_geoms_arrays(shift)
        g = geometry_desc(tv, sph, dsc, mats, mat_ids)
        hs = irl.HostScene.from_arrays(g)
        hs._keep = g._keep
        hs.desc.set_image(64, 64)
        _cache[("mg", shift)] = hs
    return _cache[("mg", shift)]


def spheres_desc(n):
    """A geometry-only desc of n unit spheres on a grid 256 wide: what the limit tests hand to the entries that must refuse 65 536 and
    more."""
    sph = np.zeros(n, irl.SPHERE)
    sph["x"], sph["y"], sph["radius"] = 3.0 * (np.arange(n) % 256), 3.0 * (np.arange(n) // 256), 1.0
    return geometry_desc(spheres=sph, mat_ids=np.zeros(n, np.uint32))


# ------------------------------------------------------------------------------------------------------
# long_mesh: one mesh on a 256 x 256 vertex grid, 130 050 triangles, and a sphere above it
# ------------------------------------------------------------------------------------------------------
SIDE = 256
QUADS = (SIDE - 1) * (SIDE - 1)            # 65 025: triangle q is the lower-left half of quad q, triangle QUADS + q its upper-right half
LM_TRIS = 2 * QUADS
COPIES = (65535, 65536, 65537)             # given triangle 0's indices: four coincident triangles with primIDs 0, 65 535, 65 536, 65 537
LM_SPHERE = (128.0, 128.0, 20.0, 4.0)


def long_mesh_arrays(shift=(0.0, 0.0, 0.0)):
    """(verts [65536, 3] float32, tris [130050, 3] uint16)."""
    if ("lm-arrays", shift) not in _cache:
        j, i = np.divmod(np.arange(SIDE * SIDE), SIDE)
        verts = np.stack([i, j, np.zeros_like(i)], 1).astype(F) + np.array(shift, F)
        cy, cx = np.divmod(np.arange(QUADS), SIDE - 1)
        v00 = cy * SIDE + cx
        ll = np.stack([v00, v00 + 1, v00 + SIDE], 1)
        ur = np.stack([v00 + 1, v00 + SIDE + 1, v00 + SIDE], 1)
        tris = np.concatenate([ll, ur]).astype(np.uint16)
        tris[list(COPIES)] = tris[0]
        _cache[("lm-arrays", shift)] = (verts, tris)
    return _cache[("lm-arrays", shift)]


def long_mesh(shift=(0.0, 0.0, 0.0)):
    if ("lm", shift) not in _cache:
        verts, tris = long_mesh_arrays(shift)
        sph = np.zeros(1, irl.SPHERE)
        sph[0] = tuple(np.array(LM_SPHERE[:3], F) + np.array(shift, F)) + LM_SPHERE[3:]
        mats = materials19()[:3].copy()
        g = geometry_desc(mesh=(verts, tris), spheres=sph, mats=mats, mat_ids=np.array([1, 0], np.uint32))      # (the sphere emits)
        hs = irl.HostScene.from_arrays(g)
        hs._keep = g._keep
        hs.desc.set_image(64, 64)
        _cache[("lm", shift)] = hs
    return _cache[("lm", shift)]


def scene(name):
    return {"many_geoms": many_geoms, "long_mesh": long_mesh}[name]()


# A path trace starts at the camera: the origin, looking along -z. The two scenes lie at z >= 0, behind it. For path traces alone
# each scene is also built moved by VIEW - the same grid, the same ids and materials - so that the camera looks down on its middle.
VIEW = {"many_geoms": (-64.0, -32.0, -42.0), "long_mesh": (-127.5, -127.5, -60.0)}


def view_scene(name):
    return {"many_geoms": many_geoms, "long_mesh": long_mesh}[name](VIEW[name])


SCENES = ("many_geoms", "long_mesh")


# ------------------------------------------------------------------------------------------------------
# the cells the tests aim at
# ------------------------------------------------------------------------------------------------------
def mg_cells(n_random=24, seed=20):
    """Cells 0, 1, 8190 (its top is 0xFFFE), 8191 (seven geometries; its layer 3 is 0x7FFF; cell 0's layer 4 is 0x8000), and some
    random ones."""
    rng = np.random.default_rng(seed)
    return [0, 1, 8190, 8191] + sorted(int(c) for c in rng.choice(np.arange(2, 8190), n_random, replace=False))


def lm_quads(n_random=12, seed=21):
    """Quads 0 (the coincident stack; its upper-right half is primID 65 025), 510 .. 512 (their upper-right halves are the copies, so
    they are holes), 51 100 (upper-right half 116 125), 65 024 (upper-right half 130 049: the last), and some random ones."""
    rng = np.random.default_rng(seed)
    return [0, 1, 509, 510, 511, 512, 513, 51100, QUADS - 1] + sorted(int(q) for q in rng.choice(np.arange(600, QUADS - 1), n_random, replace=False))


# ------------------------------------------------------------------------------------------------------
# closed forms, many_geoms. Heights are in units of 0.05: layer L's triangle lies at 5 L, its disc at 5 L + 2, its sphere spans
# 5 L - 3 .. 5 L + 5; queries are cut at half units, so no comparison of the code under test is ever closer than 0.025.
# ------------------------------------------------------------------------------------------------------
UNIT = 0.05


def _z_range(g):
    """(lowest, highest) height of geometry g in units."""
    z = 5 * (g // CELLS)
    return {0: (z, z), 1: (z - 3, z + 5), 2: (z + 2, z + 2)}[kind_of(g)]


def mg_box(cell, lo_units=-20.5, hi_units=60.5):
    """(lo, hi) of a box over the whole of a cell in x and y (no neighbour reaches it) and between two heights, and what it must list:
    [(geomID, 0, contained)] ascending. A primitive touches when its height range meets the slab and is contained when it lies inside."""
    x, y = cell_xy(cell)
    found = []
    for g in stack(cell):
        a, b = _z_range(g)
        if b > lo_units and a < hi_units:
            found.append((g, 0, a > lo_units and b < hi_units))
    return (x - 0.2, y - 0.2, lo_units * UNIT), (x + 0.7, y + 0.7, hi_units * UNIT), found


def mg_block_box(cell, nx, ny):
    """A box over nx x ny whole cells from `cell` on, all heights: lists every geometry stacked in them, ascending."""
    x, y = cell_xy(cell)
    assert x + nx <= GRID_X and y + ny <= GRID_Y
    found = sorted((g, 0, True) for j in range(ny) for i in range(nx) for g in stack(cell + j * GRID_X + i))
    return (x - 0.2, y - 0.2, -1.0), (x + nx - 0.3, y + ny - 0.3, 3.0), found


def mg_sliver(cell):
    """A query triangle standing in the cell, a sliver about the probe line from below every layer to above: it pierces every
    triangle and disc of the stack and leaves every sphere through its shell. (a, b, c) and [(geomID, 0)] ascending."""
    x, y = cell_xy(cell)
    a = (x + PROBE[0], y + PROBE[1], -1.0)
    b = (x + PROBE[0] + 0.05, y + PROBE[1], 3.0)
    c = (x + PROBE[0], y + PROBE[1] + 0.05, 3.0)
    return (a, b, c), [(g, 0) for g in stack(cell)]


HALF_CHORD = 0.2 * np.sqrt(1.0 - (0.1 ** 2 + 0.1 ** 2) / 0.04) / UNIT      # of a sphere on the probe line: 2.83 units
UP = (1e-3, 2e-3, 1.0)          # "upwards": see mg_vertical


def _sphere_roots64(o, d, c, r):
    """(near, far) parameters of the line o + t d on the sphere, binary64."""
    o, d, c = (np.asarray(v, np.float64) for v in (o, d, c))
    f = c - o
    dd = d @ d
    tca = (f @ d) / dd
    l = f - d * tca
    td = np.sqrt((r * r - l @ l) / dd)
    return float(tca - td), float(tca + td)


def mg_vertical(cell, down=True, shift=(0.0, 0.0, 0.0)):
    """A ray along the cell's probe line, from above every layer straight down or from below upwards, and the crossings it must
    list in order: (origin, direction, [(geomID, 0, far)], their t in binary64). Triangles and discs are crossed once, spheres
    twice - the near root before the MI_CROSS_FAR one. WHICH primitives are crossed and in WHICH order follows from the layer
    numbers alone (heights in units differ by at least 0.17, 0.0085 in the scene; asserted against the t); the t themselves are
    binary64 solutions for the binary32 ray and primitive.

    Upwards is UP, not (0, 0, 1). The reference's ray shear (RayShearParams, Primitives.cpp:9-21) picks its axis with
    Vec3fa::maxi, which returns the index of the SMALLEST signed component: for (0, 0, 1) exactly that is a zero component, the
    shear divides by it and every triangle misses; for (0, 0, -1) it is z and the test works. UP's smallest component is not zero.
    The triangle test itself is two-sided (Mesh.cpp:59-73).

    A disc is crossed only where n . c < 0: the reference's disc test takes the plane as n . x = -|n . c| (Primitives.cpp:48-55),
    the true plane for such a disc and its mirror image through the origin otherwise, where the ray's point is outside the
    radius. many_geoms' discs - normal (0, 0, 1), above z = 0 - are of the second kind: no ray sees them. With shift =
    VIEW["many_geoms"] every disc lies below z = 0 and is seen, so the ray families run on that copy (ray_scene) and reach
    0xFFFE; the point, box and triangle families use the true plane and run on many_geoms itself."""
    tv, sph, dsc, _, _ = many_geoms_arrays(shift)
    x, y = cell_xy(cell)
    o = np.array([x + PROBE[0] + shift[0], y + PROBE[1] + shift[1], shift[2] + (5.0 if down else -5.0)], F)
    d = np.array((0.0, 0.0, -1.0) if down else UP, F)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    ev = []                                          # (height in units, t, geomID, far)
    for g in stack(cell):
        z = 5 * (g // CELLS)
        if kind_of(g) == 0:
            ev.append((float(z), (float(tv[g, 0, 2]) - o64[2]) / d64[2], g, 0))
        elif kind_of(g) == 2:
            cz = float(dsc[g - 2 * PER_KIND]["cz"])
            if cz < 0:                               # n . c < 0: the plane the reference tests is the disc's own
                ev.append((z + 2.0, (cz - o64[2]) / d64[2], g, 0))
        else:
            s = sph[g - PER_KIND]
            near, far = _sphere_roots64(o64, d64, (s["x"], s["y"], s["z"]), float(s["radius"]))
            ev.append((z + 1 + (HALF_CHORD if down else -HALF_CHORD), near, g, 0))
            ev.append((z + 1 - (HALF_CHORD if down else -HALF_CHORD), far, g, 1))
    ev.sort(reverse=down)
    ts = [e[1] for e in ev]
    assert all(b - a > 0.005 for a, b in zip(ts, ts[1:])) and ts[0] > 1.0, "the layer numbers and the t disagree about the order"
    return tuple(float(v) for v in o), tuple(float(v) for v in d), [(g, 0, far) for _, _, g, far in ev], ts


def mg_row_ray(row, layer, shift=(0.0, 0.0, 0.0)):
    """A ray along row `row` of the grid through the centres of `layer`'s spheres (layers 3 and 4 are spheres in every cell: geomIDs
    24 576 .. 32 767 and 32 768 .. 40 959), from x = -1 in +x: it crosses the sphere of every cell of the row in turn, near root
    then far root, and nothing else (triangles and discs are parallel to it, the spheres of the layers beside end 0.05 away).
    (origin, direction, [(geomID, 0, far)] in order, their t)."""
    assert layer in (3, 4)
    _, sph, _, _, _ = many_geoms_arrays(shift)
    z = float(sph[layer * CELLS + row * GRID_X - PER_KIND]["z"])
    found, ts = [], []
    for i in range(GRID_X):
        g = layer * CELLS + row * GRID_X + i
        if g < G:
            found += [(g, 0, 0), (g, 0, 1)]
            ts += [i + 1.05, i + 1.45]
    return (-1.0 + shift[0], row + 0.25 + shift[1], z), (1.0, 0.0, 0.0), found, ts


def mg_dist64(pos, g, shift=(0.0, 0.0, 0.0)):
    """Distance in binary64 of position pos [3] from geometry g of many_geoms (moved by shift)."""
    tv, sph, dsc, _, _ = many_geoms_arrays(shift)
    p = np.asarray(pos, np.float64)
    k = kind_of(g)
    if k == 0:
        t = tv[g].astype(np.float64)
        return float(pc.tri_dist64(p[None, None, :], t[None, None, 0], t[None, None, 1], t[None, None, 2])[0, 0])
    if k == 1:
        s = sph[g - PER_KIND]
        c = np.array([s["x"], s["y"], s["z"]], np.float64)
        return abs(float(np.linalg.norm(p - c)) - float(s["radius"]))
    d = dsc[g - 2 * PER_KIND]
    v = p - np.array([d["cx"], d["cy"], d["cz"]], np.float64)
    u = float(np.hypot(v[0], v[1]))
    return abs(v[2]) if u <= float(d["r"]) else float(np.hypot(v[2], u - float(d["r"])))


def mg_neighbours(cell, z, radius):
    """The neighbours a point on the cell's probe line at height z must list for radius < 0.6 (nothing of another cell is that near):
    (position, [(dist in binary64, geomID, 0)] sorted by (dist, geomID))."""
    assert radius < 0.6
    x, y = cell_xy(cell)
    pos = tuple(float(v) for v in np.array([x + PROBE[0], y + PROBE[1], z], F))       # the binary32 point the query carries
    found = sorted((mg_dist64(pos, g), g, 0) for g in stack(cell))
    return pos, [f for f in found if f[0] < radius]


def mg_tie(cell, shift=(0.0, 0.0, 0.0)):
    """A point of a cell >= 2730 that is exactly as far from the triangle of layer 1 (geomID 8192 + cell) as from the disc of layer 5
    (geomID 40960 + cell): the two ids differ in bit 15 alone. Both primitives are horizontal and the point stands inside both
    outlines, so both distances are height differences, exact in binary32 because the midpoint of the two heights is a binary32
    number (asserted). (position, the two geomIDs, the distance: 0.55; nothing of another cell is nearer than 0.6). With a shift:
    the same in the scene moved by it."""
    lo_g, hi_g = CELLS + cell, 5 * CELLS + cell
    assert kind_of(lo_g) == 0 and kind_of(hi_g) == 2 and lo_g ^ hi_g == 0x8000
    tv, _, dsc, _, _ = many_geoms_arrays(shift)
    z_tri = np.float64(tv[lo_g, 0, 2])
    z_disc = np.float64(dsc[hi_g - 2 * PER_KIND]["cz"])
    z = F((z_tri + z_disc) / 2)
    assert np.float64(z) - z_tri == z_disc - np.float64(z), "the midpoint is not a binary32 number: no exact tie"
    x, y = cell_xy(cell)
    return (float(F(x + PROBE[0] + shift[0])), float(F(y + PROBE[1] + shift[1])), float(z)), (lo_g, hi_g), float(np.float64(z) - z_tri)


TIE_CELLS = (2730, 4000, 5000, 5460)         # (from 5461 on layer 2 is a sphere, as far from the tie point as layer 4's to 5e-8)


def view_tie_batch():
    """The tie points of TIE_CELLS in view_scene("many_geoms"): (POINT array of radius 0.58, per point [(distance, geomID, 0)] sorted).
    There the HIGHER of the two tied ids lies nearer the origin, so the builders, which put the child nearer the origin first, make
    the walk meet it before the lower one: a key that cannot tell the two apart leaves them in that order, the wrong one. (In
    many_geoms itself the lower id is met first, and such a key would pass unnoticed.)"""
    if "view-ties" not in _cache:
        shift = VIEW["many_geoms"]
        pos, want = [], []
        for c in TIE_CELLS:
            p, (lo_g, hi_g), d = mg_tie(c, shift)
            f = sorted((mg_dist64(p, g, shift), g, 0) for g in stack(c))
            f = [x for x in f if x[0] < 0.58]
            assert [x[1] for x in f[-2:]] == [lo_g, hi_g] and f[-2][0] == f[-1][0] == d and len(f) == 5
            pos.append(p); want.append(f)
        _cache["view-ties"] = (points(pos, 0.58), want)
    return _cache["view-ties"]


# ------------------------------------------------------------------------------------------------------
# closed forms, long_mesh
# ------------------------------------------------------------------------------------------------------
def _lm_fix(prims):
    """The copies: primIDs 65 535 .. 65 537 left their quads and lie on triangle 0."""
    s = set(prims) - set(COPIES)
    if 0 in s:
        s |= set(COPIES)
    return sorted(s)


def quad_xy(q):
    return q % (SIDE - 1), q // (SIDE - 1)


def lm_box(q, where):
    """A small box (half size 0.1) in quad q - where = "ll": inside the lower-left half, "ur": inside the upper-right half, "mid": on
    the diagonal, "corner": about the quad's lower-left vertex, which up to six triangles share - and the primIDs of geometry 0 it
    must list, ascending. None is contained: a triangle is a unit across."""
    cx, cy = quad_xy(q)
    if where == "corner":
        c = (cx, cy)
        prims = []
        for a, b in ((cx, cy), (cx - 1, cy), (cx, cy - 1)):
            if 0 <= a < SIDE - 1 and 0 <= b < SIDE - 1:
                prims.append(b * (SIDE - 1) + a)
        for a, b in ((cx - 1, cy), (cx - 1, cy - 1), (cx, cy - 1)):
            if 0 <= a < SIDE - 1 and 0 <= b < SIDE - 1:
                prims.append(QUADS + b * (SIDE - 1) + a)
    else:
        off = {"ll": 0.25, "ur": 0.75, "mid": 0.5}[where]
        c = (cx + off, cy + off)
        prims = {"ll": [q], "ur": [QUADS + q], "mid": [q, QUADS + q]}[where]
    return (c[0] - 0.1, c[1] - 0.1, -0.1), (c[0] + 0.1, c[1] + 0.1, 0.1), [(0, p, False) for p in _lm_fix(prims)]


def lm_vertical(q, where, down=True):
    """A vertical ray through quad q's lower-left ("ll") or upper-right ("ur") half from z = 1 down (or z = -1 up) and the primIDs of
    geometry 0 it must cross, all at t = 1, ascending: four through the coincident stack, none through a hole. Up is UP
    (mg_vertical): the ray drifts 2e-3 sideways on its way, inside the same half."""
    cx, cy = quad_xy(q)
    off = {"ll": 0.25, "ur": 0.75}[where]
    prims = _lm_fix([q] if where == "ll" else [QUADS + q])
    return (cx + off, cy + off, 1.0 if down else -1.0), ((0.0, 0.0, -1.0) if down else UP), prims


def lm_point(q, where, h=0.25):
    """A point h above a half of quad q, 0.25 from its two short edges: (position, the primIDs of geometry 0 at distance h exactly,
    ascending - the half's own triangle, or the four of the coincident stack, or none above a hole)."""
    cx, cy = quad_xy(q)
    off = {"ll": 0.25, "ur": 0.75}[where]
    return (cx + off, cy + off, h), _lm_fix([q] if where == "ll" else [QUADS + q])


def lm_dist64(pos, prims):
    verts, tris = long_mesh_arrays()
    t = verts[tris[np.asarray(prims, np.int64)].astype(np.int64)].astype(np.float64)
    p = np.asarray(pos, np.float64)
    return pc.tri_dist64(p[None, None, :], t[None, :, 0], t[None, :, 1], t[None, :, 2])[0]


def lm_neighbours(pos, radius):
    """Every triangle of long_mesh within `radius` of pos, brute force in binary64 over the quads within reach (integer arithmetic picks
    them): [(dist, 0, primID)] sorted by (dist, primID). The sphere is never within reach of the sheet's neighbourhood used here."""
    x0, x1 = int(np.floor(pos[0] - radius)) - 1, int(np.ceil(pos[0] + radius)) + 1
    y0, y1 = int(np.floor(pos[1] - radius)) - 1, int(np.ceil(pos[1] + radius)) + 1
    prims = []
    for b in range(max(y0, 0), min(y1, SIDE - 2) + 1):
        for a in range(max(x0, 0), min(x1, SIDE - 2) + 1):
            prims += [b * (SIDE - 1) + a, QUADS + b * (SIDE - 1) + a]
    prims = _lm_fix(prims)
    d = lm_dist64(pos, prims)
    return sorted((float(d[i]), 0, p) for i, p in enumerate(prims) if d[i] < radius)


# ------------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------------
def boxes(rows):
    rows = list(rows)
    return qb.make_boxes(np.array([r[0] for r in rows], F).reshape(-1, 3), np.array([r[1] for r in rows], F).reshape(-1, 3))


def rays(rows, t_max=np.inf):
    rows = list(rows)
    return qb.make_rays(np.array([r[0] for r in rows], F).reshape(-1, 3), np.array([r[1] for r in rows], F).reshape(-1, 3), 0.0, t_max)


def points(rows, radius):
    return qb.make_points(np.array(list(rows), F).reshape(-1, 3), np.asarray(radius, F))


def tris(rows):
    a = np.array(list(rows), F).reshape(-1, 3, 3)
    return qb.make_tris(a[:, 0], a[:, 1], a[:, 2])


# What a binary32 distance may differ by from the binary64 one of the same binary32 point and primitive. The contract forms the
# closest point q in scene coordinates and then |p - q|: q's x and y are rounded where coordinates reach up to 256 - half an ulp
# there, 2^-17, on each of the two axes (z stays below 2) - and around that stand at most eight rounded operations on lengths of at
# most 0.6, the reach of every query here. The neighbours of a batch are held at least 1e-4 apart, nine times this, or exactly tied.
DIST_TOL = np.sqrt(2.0) * 2.0 ** -17 + 8 * 2.0 ** -24 * 0.6


def unsigned_key(recs):
    """The key a box or triangle list is sorted by, as an unsigned number per record: geomID, then primID."""
    return (recs["geomID"].astype(np.uint64) << np.uint64(32)) | recs["primID"].astype(np.uint64)


def assert_ascending(offsets, recs, what):
    k = unsigned_key(recs)
    same = np.ones(len(k), bool)
    same[np.asarray(offsets[:-1], np.int64)[np.asarray(offsets[:-1], np.int64) < len(k)]] = False
    bad = np.nonzero(same[1:] & ~(k[1:] > k[:-1]))[0]
    assert bad.size == 0, f"{what}: a list is not strictly ascending in (geomID, primID) at record {bad[:4] + 1}"


def layers_seen(geom_ids):
    """What the reference side of every many_geoms comparison is held to: ids of all eight layers, 0x7FFF, 0x8000 and 0xFFFE."""
    g = np.asarray(list(geom_ids), np.int64)
    return set((g // CELLS).tolist()) == set(range(LAYERS)) and {0x7FFF, 0x8000, 0xFFFE} <= set(g.tolist())


def prims_seen(prim_ids):
    """The same for long_mesh: primIDs at and past 65 536, and the 65 535 | 65 536 neighbours."""
    p = set(int(x) for x in prim_ids)
    return {0, 65535, 65536, 65537} <= p and max(p) >= QUADS + 51100


# ------------------------------------------------------------------------------------------------------
# the existing checkers over a quarter of a million nodes: their lazy constructors (near_cases.NearChecker.lazy,
# count_cases.Checker.lazy) fill the tables by numpy and resolve a leaf when a walk first reaches it
# ------------------------------------------------------------------------------------------------------
def checker(cls, hs, nodes=None):
    """cls (NearChecker, BoxChecker or TriChecker) over hs's nodes (or `nodes`)."""
    return cls.lazy(hs, nodes)


def ray_checker(cls, hs):
    """cls (count_cases.Checker or list_cases.ListChecker) over hs."""
    return cls.lazy(hs)


def leaf_ids(nodes):
    """(geomID, primID) of every leaf of a node array, as a uint64 key array."""
    leaf = nodes["geomID"] != irl.INVALID_GEOM
    return (nodes["geomID"][leaf].astype(np.uint64) << np.uint64(32)) | nodes["link"][leaf].astype(np.uint64)


def expected_leaf_ids(name):
    """What leaf_ids must give, sorted: every primitive of the scene exactly once."""
    if name == "many_geoms":
        return np.arange(G, dtype=np.uint64) << np.uint64(32)
    return np.concatenate([np.arange(LM_TRIS, dtype=np.uint64), [np.uint64(1) << np.uint64(32)]])


# ------------------------------------------------------------------------------------------------------
# the batches of the two test files, with what the closed forms say of them; made once. Each asserts, on the reference side alone,
# that it reaches the ids it is there for.
# ------------------------------------------------------------------------------------------------------
SLABS = ((-20.5, 60.5), (-0.5, 17.5), (12.5, 22.5), (18.5, 40.5))      # all heights; layers 0 .. 3; parts of layers 2 .. 4; layers 4 .. 7


def _once(fn):
    def get(name):
        if (fn.__name__, name) not in _cache:
            _cache[(fn.__name__, name)] = fn(name)
        return _cache[(fn.__name__, name)]
    return get


@_once
def box_batch(name):
    """(BOX array, per box [(geomID, primID, contained)] ascending)."""
    rows, want = [], []
    if name == "many_geoms":
        for c in mg_cells():
            for lo, hi in SLABS:
                a, b, f = mg_box(c, lo, hi)
                rows.append((a, b)); want.append(f)
        for c, nx, ny in ((0, 3, 2), (8192 - 2 * GRID_X - 3, 3, 2), (4000, 2, 2)):
            a, b, f = mg_block_box(c, nx, ny)
            rows.append((a, b)); want.append(f)
        assert layers_seen(g for f in want for g, _, _ in f)
        assert any(g >= 0x8000 and not inside for f in want for g, _, inside in f) and any(g >= 0x8000 and inside for f in want for g, _, inside in f)
    else:
        for q in lm_quads():
            for w in ("ll", "ur", "mid", "corner"):
                a, b, f = lm_box(q, w)
                rows.append((a, b)); want.append(f)
        assert prims_seen(p for f in want for _, p, _ in f)
        assert [p for _, p, _ in want[3]] == [0, 65535, 65536, 65537] and any(len(f) == 6 for f in want) and any(len(f) == 0 for f in want)
    return boxes(rows), want


@_once
def tri_batch(name):
    """(TRI array, per query triangle [(geomID, primID)] ascending)."""
    rows, want = [], []
    if name == "many_geoms":
        for c in mg_cells():
            t, f = mg_sliver(c)
            rows.append(t); want.append(f)
        assert layers_seen(g for f in want for g, _ in f)
    else:
        for q in lm_quads():
            for w in ("ll", "ur"):
                o, _, prims = lm_vertical(q, w)
                rows.append(((o[0], o[1], -1.0), (o[0] + 0.05, o[1], 1.0), (o[0], o[1] + 0.05, 1.0)))      # a sliver through the sheet
                want.append([(0, p) for p in prims])
        assert prims_seen(p for f in want for _, p in f)
    return tris(rows), want


@_once
def near_batch(name):
    """(POINT array, per point [(distance in binary64, geomID, primID)] sorted by (distance, geomID, primID), the indices of the
    points whose list ends in an exact tie of two ids)."""
    pos, radius, want, ties = [], [], [], []
    if name == "many_geoms":
        for c in mg_cells():
            for z, r in ((-0.1, 0.45), (0.4, 0.5), (1.0, 0.58), (1.9, 0.33)):
                p, f = mg_neighbours(c, z, r)
                pos.append(p); radius.append(r); want.append(f)
        for c in TIE_CELLS:
            p, (lo_g, hi_g), d = mg_tie(c)
            f = mg_neighbours(c, p[2], 0.58)[1]
            assert [x[1] for x in f[-2:]] == [lo_g, hi_g] and f[-2][0] == f[-1][0] == d
            ties.append(len(pos)); pos.append(p); radius.append(0.58); want.append(f)
        assert layers_seen(g for f in want for _, g, _ in f)
    else:
        for q in lm_quads():
            for w in ("ll", "ur"):
                p, prims = lm_point(q, w)
                f = lm_neighbours(p, 0.3)            # (the triangles beside are 0.354 away, two by two equally far)
                assert [x[2] for x in f] == prims and all(x[0] == 0.25 for x in f)
                if len(prims) == 4:
                    ties.append(len(pos))
                pos.append(p); radius.append(0.3); want.append(f)
        assert prims_seen(p for f in want for _, _, p in f) and ties
    for f in want:                          # margin: apart from exact ties no two distances, and no distance and the radius, are close
        d = np.array([x[0] for x in f])
        gap = np.diff(d)
        assert np.all((gap == 0) | (gap > 1e-4)), "two neighbours are nearly as far: choose another point"
    assert all(abs(x[0] - r) > 1e-3 for f, r in zip(want, radius) for x in f), "a neighbour is nearly as far as the radius"
    return points(pos, radius), want, ties


def ray_scene(name):
    """The scene the ray families run on: many_geoms moved by VIEW, where rays see the discs (mg_vertical); long_mesh itself."""
    return view_scene(name) if name == "many_geoms" else scene(name)


def _ray_batch(name, shift):
    rows, want, ts = [], [], []
    if name == "many_geoms":
        for c in mg_cells():
            for down in (True, False):
                o, d, f, t = mg_vertical(c, down, shift)
                rows.append((o, d)); want.append(f); ts.append(t)
        for row, layer in ((0, 3), (63, 3), (0, 4), (63, 4), (17, 4)):
            o, d, f, t = mg_row_ray(row, layer, shift)
            rows.append((o, d)); want.append(f); ts.append(t)
        if shift[2] < -2:                         # every disc below z = 0: rays reach what the other families reach
            assert layers_seen(g for f in want for g, _, _ in f)
            assert all(f[0][0] // CELLS == len(stack(f[0][0] % CELLS)) - 1 for f in want[0:2 * len(mg_cells()):2]), "from above the top layer is hit"
            assert all(f[0][0] // CELLS == 0 for f in want[1:2 * len(mg_cells()):2]), "from below layer 0 is hit"
        assert sum(g >= 0x8000 for f in want for g, _, _ in f) * 4 >= sum(len(f) for f in want)
    else:
        for q in lm_quads():
            for w in ("ll", "ur"):
                for down in (True, False):
                    o, d, prims = lm_vertical(q, w, down)
                    rows.append((o, d)); want.append([(0, p, 0) for p in prims]); ts.append([1.0] * len(prims))
        # through the sphere (geometry 1), 0.25 off its axis both ways, then the sheet in the lower-left half of quad (128, 128)
        rows.append(((LM_SPHERE[0] + 0.25, LM_SPHERE[1] + 0.25, 30.0), (0.0, 0.0, -1.0)))
        chord = float(np.sqrt(LM_SPHERE[3] ** 2 - 0.125))
        want.append([(1, 0, 0), (1, 0, 1), (0, 128 * (SIDE - 1) + 128, 0)])
        ts.append([30.0 - LM_SPHERE[2] - chord, 30.0 - LM_SPHERE[2] + chord, 30.0])
        assert prims_seen(p for f in want for _, p, _ in f)
    return rays(rows), want, ts


@_once
def ray_batch(name):
    """(RAY array, per ray [(geomID, primID, far)] in the list's order, per ray the crossings' t) for ray_scene(name)."""
    return _ray_batch(name, VIEW[name] if name == "many_geoms" else (0.0, 0.0, 0.0))


@_once
def ray_batch_home(name):
    """The same rays in scene(name) itself: in many_geoms no disc is crossed there (mg_vertical)."""
    return _ray_batch(name, (0.0, 0.0, 0.0))
