"""Shared by the crossing-list tests (test_list_abi.py, test_list_checker.py, test_list_gpu.py): THE LIST CHECKER - count_cases.Checker's
walk (the oracle's box test over the fixed interval, its triangle and disc tests) collecting the crossings instead of counting them,
with sphere_roots restated in numpy binary32 from the text of csrc/cross_math.hpp -, the sort by the contract's key, records cut or
padded to a length, and the `layers` scene: long lists with exact ties. Expected results are computed once per process and shared."""
import ctypes as C
import functools
import types

import numpy as np

import ipu_ray_lib_amd as irl
from ipu_ray_lib_amd import query_batches as qb
import oracle_lib as ol
import count_cases as cc

F = np.float32
INF = F(np.inf)


# ------------------------------------------------------------------------------------------------------
# sphere_roots in numpy binary32: (mask, t0, t1); bit 0 = the near root t0 accepted, bit 1 = the far root t1
# ------------------------------------------------------------------------------------------------------
def sphere_roots32(c, radius2, o, d, t_min, t_max):
    c, o, d = np.asarray(c, F), np.asarray(o, F), np.asarray(d, F)
    radius2, t_min, t_max = F(radius2), F(t_min), F(t_max)
    with np.errstate(all="ignore"):
        f = (c - o).astype(F)
        dd = cc.dot32(d, d)
        tca = F(cc.dot32(f, d) / dd)
        l = (f - (d * tca).astype(F)).astype(F)
        l2 = cc.dot32(l, l)
        if not (l2 <= radius2):
            return 0, None, None
        td = F(np.sqrt(F(F(radius2 - l2) / dd)))
        t0, t1 = F(tca - td), F(tca + td)
        return int(t0 > t_min and t0 < t_max) | (int(t1 > t_min and t1 < t_max) << 1), t0, t1


# ------------------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------------------
def with_nodes(hs, nodes):
    """`hs` as the checker reads it, with another tree over the same primitives (irl.build_lbvh's)."""
    return types.SimpleNamespace(desc=hs.desc, nodes=nodes, tris=hs.tris, verts=hs.verts, geometry=hs.geometry, mesh_info=hs.mesh_info,
                                 spheres=hs.spheres, discs=hs.discs)


def key(rec):
    """The contract's order: t (as a float: -0 == +0), geomID, primID, near before far."""
    return (float(rec[0]), rec[1], rec[2], rec[3])


class ListChecker(cc.Checker):
    """Checker's walk, collecting (t, geomID, primID, far) where Checker.count counts. A triangle's primID is its node's; a sphere's
    and a disc's is 0, as every query reports them."""

    def crossings(self, ray):
        """The sorted crossings of one RAY record: a list of (t float32, geomID, primID, far 0 | 1)."""
        o = ol.lib()
        if self.n == 0:
            return []
        r = ol.Ray.from_buffer_copy(np.asarray(ray).tobytes())
        t_min, t_max = F(r.tMin), F(r.tMax)
        with np.errstate(all="ignore"):
            inv = [float(F(1) / F(x)) for x in (r.direction.x, r.direction.y, r.direction.z)]
        inv = ol.Vec3(*inv)
        sh = None
        bary = (C.c_float * 3)()
        t0, t1 = C.c_float(), C.c_float()
        found = []
        stack = [0]
        while stack:
            cur = stack.pop()
            t0.value, t1.value = r.tMin, r.tMax
            if not o.o_node_intersect(C.byref(self.nodes[cur]), r.origin, inv, C.byref(t0), C.byref(t1)):
                continue
            if self.geom[cur] == irl.INVALID_GEOM:
                stack.append(self.link[cur])
                stack.append(cur + 1)
                continue
            kind, prim = self.prims[cur]
            g = self.geom[cur]
            if kind == 0:
                if sh is None:
                    sh = ol.Shear()
                    o.o_ray_shear(C.byref(r), C.byref(sh))
                t = F(o.o_intersect_triangle(prim[0], prim[1], prim[2], C.byref(sh), INF, bary))
                if t > 0 and t < INF and t > t_min and t < t_max:
                    found.append((t, g, self.link[cur], 0))
            elif kind == 1:
                mask, ta, tb = sphere_roots32(prim[0], prim[1], (r.origin.x, r.origin.y, r.origin.z),
                                              (r.direction.x, r.direction.y, r.direction.z), t_min, t_max)
                if mask & 1:
                    found.append((ta, g, 0, 0))
                if mask & 2:
                    found.append((tb, g, 0, 1))
            else:
                t = F(o.o_disc_intersect(C.byref(prim), C.byref(r)))
                if t > t_min and t < t_max:
                    found.append((t, g, 0, 0))
        found.sort(key=key)
        return found

    def lists(self, rays):
        return [self.crossings(rays[i]) for i in range(rays.size)]


def records(found, ray, length=None):
    """One ray's crossings as CROSSING records, cut or padded with the empty record to `length` (None: as many as there are)."""
    length = len(found) if length is None else length
    out = np.zeros(length, irl.CROSSING)
    out["t"], out["primID"], out["geomID"], out["flags"], out["ray"] = np.inf, irl.INVALID_PRIM, irl.INVALID_GEOM, irl.FLAG_ESCAPED, ray
    for j, (t, g, p, far) in enumerate(found[:length]):
        out[j] = (t, p, g, irl.CROSS_FAR if far else 0, ray)
    return out


def packed(lists, first_ray=0):
    """(offsets uint64 [n + 1], hits CROSSING [total]): what list_crossings returns for these lists."""
    offsets = np.zeros(len(lists) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    parts = [records(x, first_ray + i) for i, x in enumerate(lists)]
    return offsets, (np.concatenate(parts) if parts else np.zeros(0, irl.CROSSING))


def first_k(lists, k):
    """CROSSING [n, k]: what first_crossings(rays, k) returns for these lists."""
    return np.stack([records(x, i, k) for i, x in enumerate(lists)]) if lists else np.zeros((0, k), irl.CROSSING)


# ------------------------------------------------------------------------------------------------------
# the layers scene: long lists, exact ties
# ------------------------------------------------------------------------------------------------------
def layers_mesh(rng, shift=(0.0, 0.0, 0.0)):
    """54 quads of two triangles on [-3, 3]^2: 48 at z = a permutation of 0 .. 47 times 0.25 - 6, then the first six z again - six
    pairs of identical quads, whose crossings tie in t exactly and are told apart by primID."""
    z = rng.permutation(np.arange(48)) * 0.25 - 6.0
    z = np.concatenate([z, z[:6]])
    verts, tris = [], []
    for q, zq in enumerate(z):
        verts += [(-3, -3, zq), (3, -3, zq), (3, 3, zq), (-3, 3, zq)]
        tris += [(4 * q, 4 * q + 1, 4 * q + 2), (4 * q, 4 * q + 2, 4 * q + 3)]
    return (np.array(verts, F) + np.asarray(shift, F)).astype(F), np.array(tris, np.uint16)


LAYER_SPHERES = tuple((0.0, 0.0, 8.0, float(r)) for r in np.linspace(0.5, 4.0, 8))
LAYER_DISC = ((0.0, 0.0, 1.0, 2.5, 0.0, 0.0, -8.0),)


def layers_rays(rng, n=2000):
    o = np.zeros((n, 3), F)
    o[:, :2] = rng.uniform(-2.5, 2.5, (n, 2))
    o[:, 2] = rng.choice(np.array([-20.0, 20.0, 0.1]), n)
    d = np.zeros((n, 3), F)
    d[:, :2] = rng.normal(0.0, 0.05, (n, 2))
    d[:, 2] = np.where(o[:, 2] < -1, 1.0, np.where(o[:, 2] > 1, -1.0, rng.choice(np.array([-1.0, 1.0]), n)))
    rays = qb.make_rays(o, d)
    sel = rng.random(n) < 0.2
    rays["tMax"][sel] = rng.uniform(5, 30, int(sel.sum()))
    sel = rng.random(n) < 0.2
    rays["tMin"][sel] = rng.uniform(0, 15, int(sel.sum()))
    return rays


def layers():
    """(host scene, 2 000 rays)"""
    rng = np.random.default_rng(3)
    hs = cc.mesh_scene(*layers_mesh(rng), spheres=LAYER_SPHERES, discs=LAYER_DISC)
    hs.desc.set_image(64, 64)
    return hs, layers_rays(rng)


def scene_and_rays(name):
    """layers: its own 2 000 rays | any count_cases scene: 1 500 mixed rays"""
    if name == "layers":
        return layers()
    hs = cc.scene(name)
    return hs, cc.mixed_rays(hs, 1500, seed=11)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (host scene, rays, the checker's lists on the scene's own tree). Computed once; nobody changes it."""
    hs, rays = scene_and_rays(name)
    lists = ListChecker(hs).lists(rays)
    if name == "layers":
        lens = np.array([len(x) for x in lists])
        ties = sum(1 for x in lists if any(a[0] == b[0] for a, b in zip(x, x[1:])))
        assert lens.mean() > 20 and ties > 0, f"the layers recipe drifted: mean length {lens.mean():.1f}, {ties} rays with ties"
    return hs, rays, lists
