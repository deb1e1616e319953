"""Ray batches for ray queries, built on the host with numpy alone (no oracle): a scene's primary camera rays, cosine-distributed
diffuse bounce rays from their first hits, and shadow rays from those hits to a point light. tools/bench_query.py measures the
query kernels on them; tests/test_query_gpu.py checks them at scale. And point batches for point queries (make_points: tools/bench_point_query.py)."""
from __future__ import annotations

import numpy as np

from . import RAY, POINT, POINT_HIT, BOX, TRI, OBOX, CAPSULE, FRUSTUM, POSE, INVALID_PRIM     # noqa: F401  (the record dtypes of ray and point queries, side by side)

RAY_EPSILON = np.float32(5.9604644775390625e-08 * 1500.0)       # ray_math.h kRayEpsilon (precision_utils.hpp)
LIGHT = np.array([18.0, 257.0, -1060.0], np.float32)            # the reference's shadow-trace light (trace.cpp:247)


def _vec(a: np.ndarray, field: str) -> np.ndarray:
    return np.stack([a[field][c] for c in "xyz"], 1).astype(np.float32)


def make_rays(origins: np.ndarray, directions: np.ndarray, t_min=0.0, t_max=np.inf) -> np.ndarray:
    """A RAY array from [N, 3] origins and directions."""
    n = len(origins)
    r = np.zeros(n, RAY)
    for k, c in enumerate("xyz"):
        r["origin"][c] = origins[:, k]
        r["direction"][c] = directions[:, k]
    r["tMin"] = t_min
    r["tMax"] = t_max
    return r


def make_points(positions: np.ndarray, radius=np.inf) -> np.ndarray:
    """A POINT array from [N, 3] positions and a radius (a number or [N])."""
    p = np.zeros(len(positions), POINT)
    for k, c in enumerate("xyz"):
        p[c] = positions[:, k]
    p["radius"] = radius
    return p


def make_boxes(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """A BOX array from [N, 3] lower and upper corners (box queries: IpuScene.touches / count_overlaps / list_overlaps)."""
    b = np.zeros(len(lo), BOX)
    b["lo"] = lo
    b["hi"] = hi
    return b


def make_tris(a: np.ndarray, b: np.ndarray, c: np.ndarray | None = None) -> np.ndarray:
    """A TRI array (triangle queries: IpuScene.tri_touches / count_contacts / list_contacts) from three [N, 3] arrays of corners, or,
    with two arguments, from (vertices [V, 3], faces [F, 3]): the batch is vertices[faces]."""
    if c is None:
        corners = np.asarray(a, np.float32)[np.asarray(b, np.int64)]
    else:
        corners = np.stack([np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32)], axis=1)
    assert corners.ndim == 3 and corners.shape[1:] == (3, 3)
    return np.ascontiguousarray(corners, np.float32).reshape(-1, 9).view(TRI).reshape(-1)


def matrix_to_quat(matrix: np.ndarray) -> np.ndarray:
    """[n, 3, 3] rotation matrices (columns = the rotated axes) as [n, 4] quaternions x, y, z, w, in float64: the branch on the
    largest diagonal term (Shepperd), so that the divisor is never small."""
    m = np.asarray(matrix, np.float64)
    assert m.ndim == 3 and m.shape[1:] == (3, 3)
    m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
    tr = m00 + m11 + m22
    q = np.empty((len(m), 4), np.float64)
    pick = np.where(tr > 0, 3, np.argmax(np.stack([m00, m11, m22], 1), axis=1))
    for k in range(4):
        i = pick == k
        if not i.any():
            continue
        a = m[i]
        if k == 3:
            w = np.sqrt(1.0 + tr[i]) * 0.5
            q[i] = np.stack([(a[:, 2, 1] - a[:, 1, 2]) / (4 * w), (a[:, 0, 2] - a[:, 2, 0]) / (4 * w), (a[:, 1, 0] - a[:, 0, 1]) / (4 * w), w], 1)
        elif k == 0:
            x = np.sqrt(1.0 + a[:, 0, 0] - a[:, 1, 1] - a[:, 2, 2]) * 0.5
            q[i] = np.stack([x, (a[:, 0, 1] + a[:, 1, 0]) / (4 * x), (a[:, 0, 2] + a[:, 2, 0]) / (4 * x), (a[:, 2, 1] - a[:, 1, 2]) / (4 * x)], 1)
        elif k == 1:
            y = np.sqrt(1.0 - a[:, 0, 0] + a[:, 1, 1] - a[:, 2, 2]) * 0.5
            q[i] = np.stack([(a[:, 0, 1] + a[:, 1, 0]) / (4 * y), y, (a[:, 1, 2] + a[:, 2, 1]) / (4 * y), (a[:, 0, 2] - a[:, 2, 0]) / (4 * y)], 1)
        else:
            z = np.sqrt(1.0 - a[:, 0, 0] - a[:, 1, 1] + a[:, 2, 2]) * 0.5
            q[i] = np.stack([(a[:, 0, 2] + a[:, 2, 0]) / (4 * z), (a[:, 1, 2] + a[:, 2, 1]) / (4 * z), z, (a[:, 1, 0] - a[:, 0, 1]) / (4 * z)], 1)
    return q


def make_oboxes(centre: np.ndarray, half: np.ndarray, quat: np.ndarray | None = None, matrix: np.ndarray | None = None) -> np.ndarray:
    """An OBOX array (oriented-box queries: IpuScene.obox_touches / count_obox_overlaps / list_obox_overlaps) from [N, 3] centres and
    half extents and EITHER quat, [N, 4] quaternions x, y, z, w (they need not be unit), OR matrix, [N, 3, 3] rotation matrices whose
    columns are the box's axes in world coordinates (converted by matrix_to_quat). Exactly one of the two must be given."""
    if (quat is None) == (matrix is None):
        raise ValueError("make_oboxes: exactly one of quat and matrix must be given")
    b = np.zeros(len(centre), OBOX)
    b["centre"] = centre
    b["half"] = half
    b["quat"] = matrix_to_quat(matrix) if quat is None else quat
    return b


def make_capsules(a: np.ndarray, b: np.ndarray, radius) -> np.ndarray:
    """A CAPSULE array (capsule queries: IpuScene.capsule_touches / count_capsule_overlaps / list_capsule_overlaps) from [N, 3] ends a
    and b and a radius (a number or [N]). A ball of that radius moving straight from p0 to p1 is the capsule (p0, p1, radius)."""
    a, b = np.asarray(a, np.float32).reshape(-1, 3), np.asarray(b, np.float32).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError("make_capsules: a and b must have the same shape [N, 3]")
    radius = np.asarray(radius, np.float32)
    if radius.ndim > 1 or (radius.ndim == 1 and radius.size != len(a)):
        raise ValueError("make_capsules: radius must be a number or an array of length N")
    c = np.zeros(len(a), CAPSULE)
    c["a"] = a
    c["b"] = b
    c["radius"] = radius
    return c


def camera_view_proj(eye, forward, up, fovy: float, aspect: float, near: float, far: float = np.inf, depth: str = "zo") -> np.ndarray:
    """The [4, 4] float64 view-projection matrix, acting on column vectors, of a perspective camera at `eye` looking along `forward`
    with `up` roughly upward, a vertical field of view of `fovy` RADIANS and width : height = `aspect`: right = forward x up,
    clip w = the depth along forward, clip x = right.(p - eye) / (aspect tan(fovy / 2)), clip y = up'.(p - eye) / tan(fovy / 2), and
    clip z / w running from 0 ("zo") or -1 ("no") at `near` to 1 at `far` (far = inf: the limit). What make_frusta(eye=...) makes
    its planes from."""
    if depth not in ("zo", "no"):
        raise ValueError('camera_view_proj: depth must be "zo" or "no"')
    eye, f, u = (np.asarray(v, np.float64).reshape(3) for v in (eye, forward, up))
    f = f / np.linalg.norm(f)
    r = np.cross(f, u)
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    t = np.tan(0.5 * float(fovy))
    n, fa = float(near), float(far)
    view = np.zeros((4, 4))
    view[0, :3], view[1, :3], view[2, :3] = r, u, f
    view[:3, 3] = -view[:3, :3] @ eye
    view[3, 3] = 1.0
    proj = np.zeros((4, 4))
    proj[0, 0], proj[1, 1], proj[3, 2] = 1.0 / (float(aspect) * t), 1.0 / t, 1.0
    if depth == "zo":
        proj[2, 2], proj[2, 3] = (1.0, -n) if np.isinf(fa) else (fa / (fa - n), -fa * n / (fa - n))
    else:
        proj[2, 2], proj[2, 3] = (1.0, -2.0 * n) if np.isinf(fa) else ((fa + n) / (fa - n), -2.0 * fa * n / (fa - n))
    return proj @ view


def make_frusta(planes: np.ndarray | None = None, *, view_proj: np.ndarray | None = None, depth: str = "zo", eye=None, forward=None, up=None,
                fovy: float | None = None, aspect: float = 1.0, near: float | None = None, far: float = np.inf, tiles=None) -> np.ndarray:
    """A FRUSTUM array (frustum queries: IpuScene.frustum_touches / count_frustum_overlaps / list_frustum_overlaps), from one of
      planes=[n, 6, 4]: the planes nx, ny, nz, d themselves - normals inward, not necessarily unit, a plane of four zeros absent;
      view_proj=[4, 4] or [n, 4, 4]: view-projection matrices acting on column vectors. With rows r0..r3 the planes are, in this
        order, r3 + r0, r3 - r0, r3 + r1, r3 - r1 (the sides), near - r2 for depth="zo" (clip z in [0, w]), r3 + r2 for "no" (clip z
        in [-w, w]) - and far, r3 - r2; computed in float64, not normalised, rounded once;
      eye=, forward=, up=, fovy= (radians), aspect=, near=, far=: one camera, through camera_view_proj; far=inf makes the far plane
        absent.
    tiles=(tx, ty) splits each frustum of the last two forms into tx ty sub-frusta, those of frustum i at [i tx ty, (i + 1) tx ty) in
    row-major order - tile (column c, row r) at r tx + c, rows from clip y = -w upward, columns from clip x = -w: its sides are
    r0 - x0 r3, x1 r3 - r0, r1 - y0 r3, y1 r3 - r1 with x0 = -1 + 2 c / tx, x1 = -1 + 2 (c + 1) / tx and y likewise. Neighbouring
    tiles share their plane bit for bit up to the sign, and the outer tiles' outer planes are the parent's."""
    if planes is not None:
        if view_proj is not None or eye is not None or tiles is not None:
            raise ValueError("make_frusta: planes= stands alone")
        pl = np.asarray(planes, np.float32)
        if pl.ndim == 2:
            pl = pl[None]
        if pl.ndim != 3 or pl.shape[1:] != (6, 4):
            raise ValueError("make_frusta: planes must be [n, 6, 4]")
        out = np.zeros(len(pl), FRUSTUM)
        out["planes"] = pl
        return out
    if depth not in ("zo", "no"):
        raise ValueError('make_frusta: depth must be "zo" or "no"')
    no_far = False
    if view_proj is None:
        if eye is None or forward is None or up is None or fovy is None or near is None:
            raise ValueError("make_frusta: give planes=, view_proj= or eye=, forward=, up=, fovy=, near=")
        view_proj = camera_view_proj(eye, forward, up, fovy, aspect, near, far, depth)
        no_far = bool(np.isinf(far))
    elif eye is not None:
        raise ValueError("make_frusta: view_proj= and eye= exclude each other")
    m = np.asarray(view_proj, np.float64)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[1:] != (4, 4):
        raise ValueError("make_frusta: view_proj must be [4, 4] or [n, 4, 4]")
    r0, r1, r2, r3 = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    near_plane = r2 if depth == "zo" else r3 + r2
    far_plane = np.zeros_like(r2) if no_far else r3 - r2
    if tiles is None:
        pl = np.stack([r3 + r0, r3 - r0, r3 + r1, r3 - r1, near_plane, far_plane], axis=1)
    else:
        tx, ty = (int(t) for t in tiles)
        if tx < 1 or ty < 1:
            raise ValueError("make_frusta: tiles must be two positive counts")
        col, row = np.tile(np.arange(tx), ty), np.repeat(np.arange(ty), tx)                 # row-major: tile r tx + c
        x0, x1 = -1.0 + 2.0 * col / tx, -1.0 + 2.0 * (col + 1) / tx
        y0, y1 = -1.0 + 2.0 * row / ty, -1.0 + 2.0 * (row + 1) / ty
        a = lambda v: v[:, None, :]                                                         # noqa: E731  [n, 1, 4] against [1, tiles, 1]
        b = lambda v: v[None, :, None]                                                      # noqa: E731
        k = tx * ty
        sides = [a(r0) - b(x0) * a(r3), b(x1) * a(r3) - a(r0), a(r1) - b(y0) * a(r3), b(y1) * a(r3) - a(r1)]
        rest = [np.broadcast_to(a(near_plane), (len(m), k, 4)), np.broadcast_to(a(far_plane), (len(m), k, 4))]
        pl = np.stack(sides + rest, axis=2).reshape(len(m) * k, 6, 4)
    out = np.zeros(len(pl), FRUSTUM)
    out["planes"] = pl.astype(np.float32)
    return out


def make_poses(n: int, quat: np.ndarray | None = None, translation: np.ndarray | None = None, scale=None, matrix: np.ndarray | None = None) -> np.ndarray:
    """A POSE array of n poses (rigid poses: IpuScene.set_poses) from [n, 4] quaternions x, y, z, w (they need not be unit) OR [n, 3, 3]
    rotation matrices (converted by matrix_to_quat, as make_oboxes does), [n, 3] translations and a scale (a number or [n]). Missing
    parts are the identity's: quaternion (0, 0, 0, 1), translation 0, scale 1."""
    if quat is not None and matrix is not None:
        raise ValueError("make_poses: at most one of quat and matrix may be given")
    p = np.zeros(n, POSE)
    p["quat"] = (0.0, 0.0, 0.0, 1.0)
    p["scale"] = 1.0
    if matrix is not None:
        p["quat"] = matrix_to_quat(matrix)
    elif quat is not None:
        p["quat"] = quat
    if translation is not None:
        p["translation"] = translation
    if scale is not None:
        p["scale"] = scale
    return p


def primary_rays(host_scene) -> np.ndarray:
    """The scene's camera rays (initPerspectiveRayStream without jitter, mi_init_ray_stream) as RAY records."""
    s = host_scene.init_ray_stream()
    return make_rays(_vec(s["h"]["r"], "origin"), _vec(s["h"]["r"], "direction"))


def offset_origin(p: np.ndarray, d: np.ndarray, n: np.ndarray) -> np.ndarray:
    """Render.hpp:29-33 (ray_math.h offset_origin) in binary32."""
    m = (np.float32(1) + np.abs(p).min(axis=1)) * RAY_EPSILON * np.copysign(np.float32(1), (n * d).sum(axis=1, dtype=np.float32))
    return (p + n * m[:, None].astype(np.float32)).astype(np.float32)


def hit_points(rays: np.ndarray, hits: np.ndarray):
    """(mask of rays that hit, hit points, normals facing the incoming ray) from a closest-hit query's QUERY_HIT results."""
    hit = hits["primID"] != INVALID_PRIM
    o, d = _vec(rays, "origin")[hit], _vec(rays, "direction")[hit]
    p = (o + d * hits["t"][hit][:, None]).astype(np.float32)
    n = _vec(hits, "normal")[hit]
    n = np.where(((n * d).sum(axis=1) > 0)[:, None], -n, n).astype(np.float32)
    return hit, p, n


def bounce_rays(rays: np.ndarray, hits: np.ndarray, per_hit: int = 1, seed: int = 0) -> np.ndarray:
    """Cosine-distributed diffuse bounce rays, `per_hit` per hit, leaving the hit points offset as offset_origin does."""
    _, p, n = hit_points(rays, hits)
    p, n = np.repeat(p, per_hit, 0), np.repeat(n, per_hit, 0)
    rng = np.random.default_rng(seed)
    u1, u2 = rng.random(len(p), np.float32), rng.random(len(p), np.float32)
    r, phi = np.sqrt(u1), np.float32(2 * np.pi) * u2
    local = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(0, 1 - u1))], 1).astype(np.float32)
    # an orthonormal frame around n
    a = np.where((np.abs(n[:, 0]) > 0.9)[:, None], np.array([0, 1, 0], np.float32), np.array([1, 0, 0], np.float32))
    t = np.cross(a, n); t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    d = (t * local[:, :1] + b * local[:, 1:2] + n * local[:, 2:3]).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return make_rays(offset_origin(p, d, n), d)


def shadow_rays(rays: np.ndarray, hits: np.ndarray, light=LIGHT) -> np.ndarray:
    """Any-hit rays from the hit points to a point light (Render.hpp:37-72): t_max = the distance to the light."""
    _, p, n = hit_points(rays, hits)
    off = (np.asarray(light, np.float32)[None, :] - p).astype(np.float32)
    dist = np.sqrt((off * off).sum(axis=1)).astype(np.float32)
    d = (off / dist[:, None]).astype(np.float32)
    return make_rays(offset_origin(p, d, n), d, 0.0, dist)
