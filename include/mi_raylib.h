/*
 * mi_raylib.h — C ABI of the MI355X (gfx950) ray/path-trace hot path.
 *
 * This is the drop-in boundary for the device renderer of markp-gc/ipu_ray_lib:
 * what the reference reaches through `IpuScene` + `ipu_utils::GraphManager().run()`
 * (reference include/IpuScene.hpp:33-56, caller trace.cpp:270-336) is reached here
 * through five plain-C entry points. Plain pointers and sizes only; no C++ types,
 * no torch types, no exceptions cross this boundary. Every function returns an
 * int status (MI_OK == 0) and leaves a message retrievable with mi_last_error().
 *
 * POD layouts are those of the reference (probe sizes in SURVEY.md §8a):
 *   mi_trace_result == embree_utils::TraceResult   (84 B, include/embree_utils/geometry.hpp:253-259)
 *   mi_hit_record   == embree_utils::HitRecord     (64 B, geometry.hpp:226-251)
 *   mi_ray          == embree_utils::Ray           (32 B, geometry.hpp:212-224)
 *   mi_bvh_node     == CompactBVH2Node             (24 B, include/CompactBVH2Node.hpp:52-85)
 *   mi_material     == Material                    (36 B, include/Material.hpp:8-35)
 *   mi_mesh_info    == MeshInfo                    (16 B, include/Mesh.hpp:15-20)
 *   mi_geom_ref     == GeomRef                     (4 B,  include/Scene.hpp:29-34)
 * Spheres and discs cross the boundary as vptr-free PODs (the reference's host
 * Sphere/Disc objects carry vtable pointers, include/Primitives.hpp:36-82).
 */
#ifndef MI_RAYLIB_H
#define MI_RAYLIB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
enum {
  MI_OK = 0,
  MI_ERR_INVALID_ARG = 1,   /* null pointer, bad size, inconsistent scene arrays */
  MI_ERR_DEVICE = 2,        /* HIP runtime error (message in mi_last_error)      */
  MI_ERR_NO_NIF = 3,        /* NIF entry point used before weights were loaded   */
  MI_ERR_IO = 4             /* file could not be read / parsed                   */
};

/* ---- POD types (layout == reference) ------------------------------------ */
typedef struct { float x, y, z; } mi_vec3;                      /* Vec3fa, 12 B, align 4 */

typedef struct {
  mi_vec3 origin; float t_min; mi_vec3 direction; float t_max;
} mi_ray;                                                        /* 32 B */

typedef struct {
  mi_ray r;
  uint32_t prim_id;          /* 0xFFFFFFFF = invalid */
  mi_vec3 normal;
  mi_vec3 throughput;
  uint16_t geom_id;          /* 0xFFFF = invalid */
  uint16_t flags;            /* MI_FLAG_ERROR | MI_FLAG_ESCAPED */
} mi_hit_record;                                                 /* 64 B */

typedef struct {
  mi_vec3 rgb;               /* path-trace: SUM over samples (caller divides by spp) */
  float u, v;                /* PixelCoord: u = image ROW, v = image COLUMN (src/app_utils.cpp:43) */
  mi_hit_record h;
} mi_trace_result;                                               /* 84 B */

#define MI_FLAG_ERROR   ((uint16_t)1)
#define MI_FLAG_ESCAPED ((uint16_t)2)
#define MI_INVALID_GEOM ((uint16_t)0xFFFF)
#define MI_INVALID_PRIM ((uint32_t)0xFFFFFFFFu)

/* Result of a closest-hit ray query (mi_query / mi_query_device). No reference POD: the fields are what
 * CompactBvh::intersect (CompactBvh.hpp:80-139) determines for one ray. */
typedef struct {
  float    t;          /* hit distance; == ray.t_max on a miss                                          */
  uint32_t prim_id;    /* reference primID (as mi_hit_record.prim_id); MI_INVALID_PRIM on a miss          */
  uint16_t geom_id;    /* MI_INVALID_GEOM on a miss                                                     */
  uint16_t flags;      /* MI_FLAG_ESCAPED on a miss, else 0                                             */
  mi_vec3  normal;     /* Primitive::normal at origin + t*dir (Mesh.hpp:107-121, Primitives.hpp); 0 on a miss */
  float    b1, b2;     /* barycentrics of a triangle hit as intersectTriangle computes them; 0 otherwise  */
} mi_query_hit;                                                  /* 32 B */

enum { MI_QUERY_CLOSEST = 0, MI_QUERY_ANY = 1 };

/* A point query (mi_point_query / mi_point_query_device) and its MI_POINT_CLOSEST result. No reference POD: Embree's
 * rtcPointQuery asks the same of its BVH. */
typedef struct { float x, y, z, radius; } mi_point;            /* 16 B */
typedef struct {
  float    dist;       /* sqrtf of the winning squared distance; == radius as given when nothing was found              */
  uint32_t prim_id;    /* as mi_query_hit; MI_INVALID_PRIM when nothing was found                                        */
  uint16_t geom_id;    /* MI_INVALID_GEOM when nothing was found                                                         */
  uint16_t flags;      /* MI_FLAG_ESCAPED when nothing was found, else 0                                                 */
  mi_vec3  point;      /* the closest point on the primitive; 0 when nothing was found                                   */
  float    b1, b2;     /* triangle: barycentrics v, w of `point` (point = a + ab v + ac w); 0 otherwise                  */
} mi_point_hit;                                                  /* 32 B */

enum { MI_POINT_CLOSEST = 0, MI_POINT_WITHIN = 1 };

typedef struct {
  float min_x, min_y, min_z;
  uint32_t prim_or_second_child;   /* leaf: primID; interior: index of second child (first child = this+1) */
  uint16_t dx, dy, dz;             /* IEEE binary16 bit patterns of the box extents, rounded up */
  uint16_t geom_id;                /* 0xFFFF => interior node */
} mi_bvh_node;                                                   /* 24 B, align 8 in the reference */

typedef struct {
  mi_vec3 albedo; float ior; mi_vec3 emission;
  int32_t type;                    /* 0 Diffuse, 1 Specular, 2 Refractive (Material::Type) */
  uint8_t emissive; uint8_t pad[3];
} mi_material;                                                   /* 36 B */

typedef struct {
  uint32_t first_index, first_vertex, num_triangles, num_vertices;
} mi_mesh_info;                                                  /* 16 B */

typedef struct { uint16_t index; uint8_t type; uint8_t pad; } mi_geom_ref;   /* type: 0 mesh, 1 sphere, 2 disc */

typedef struct { float x, y, z, radius; } mi_sphere;             /* radius2 = radius*radius is derived */
typedef struct { float nx, ny, nz, r, cx, cy, cz; } mi_disc;     /* r2 = r*r is derived */

/* ---- scene description: SceneRef + sphere/disc arrays + RuntimeConfig ---- */
/* Mirrors reference include/Scene.hpp:50-74 (SceneRef) field for field, plus the
 * two primitive arrays the IpuScene ctor takes separately (IpuScene.hpp:33-38).
 * All pointers are HOST pointers owned by the caller; mi_scene_create copies
 * what it needs to the device, so they may be freed after it returns.        */
typedef struct {
  const mi_geom_ref*  geometry;      uint32_t num_geometry;
  const mi_mesh_info* mesh_info;     uint32_t num_meshes;
  const uint16_t*     mesh_tris;     uint32_t num_tris;      /* 3 x u16 per triangle (Triangle, Primitives.hpp:21-25) */
  const mi_vec3*      mesh_verts;    uint32_t num_verts;
  const mi_vec3*      mesh_normals;  uint32_t num_normals;   /* 0, or == num_verts (--load-normals) */
  const uint32_t*     mat_ids;       uint32_t num_mat_ids;   /* one per geometry */
  const mi_material*  materials;     uint32_t num_materials;
  const mi_bvh_node*  bvh_nodes;     uint32_t num_nodes;
  uint32_t            max_leaf_depth;                        /* levels, root == 1 */
  const mi_sphere*    spheres;       uint32_t num_spheres;
  const mi_disc*      discs;         uint32_t num_discs;

  float    image_width, image_height;      /* FULL image size, also when a crop window is rendered */
  float    fov_radians;
  float    anti_alias_scale;
  uint32_t max_path_length;
  uint32_t roulette_start_depth;
  uint32_t samples_per_pixel;
  uint64_t rng_seed;
  int32_t  window_w, window_h, window_c, window_r;           /* CropWindow (Scene.hpp:22-27) */
  int32_t  path_trace;                                       /* bool */
  int32_t  device;                                           /* HIP device ordinal (RuntimeConfig analogue) */
} mi_scene_desc;

typedef struct mi_scene mi_scene;   /* opaque */

/* Render modes: the two trace vertices of codelets/TraceCodelets.cpp:170-316 */
enum { MI_MODE_SHADOW_TRACE = 0, MI_MODE_PATH_TRACE = 1 };

/* Replaces: IpuScene::IpuScene(...) + setRuntimeConfig (src/IpuScene.cpp:24-62, trace.cpp:297-309) */
int mi_scene_create(const mi_scene_desc* desc, mi_scene** out);

/* Same, from the reference's serialised scene: `blob` is the byte stream Serialiser<16> produced for the
 * SceneRef (IpuScene's `serialiser.bytes`, src/IpuScene.cpp:51-53; format in csrc/scene_blob.hpp), i.e.
 * what the reference broadcasts to every tile (src/IpuScene.cpp:200-216, 422-426). The eight arrays and
 * maxLeafDepth..samplesPerPixel are taken from the blob; spheres/discs, rng_seed, the crop window,
 * path_trace and device from `extras` (whose array fields are ignored). The bytes are validated like any
 * other scene and copied; no alignment requirement. */
int mi_scene_create_from_blob(const uint8_t* blob, size_t size, const mi_scene_desc* extras, mi_scene** out);

/* Replaces: IpuScene::~IpuScene */
void mi_scene_destroy(mi_scene* scene);

/* Replaces: GraphManager().run(ipuScene) -> IpuScene::build + execute (src/IpuScene.cpp:346-733),
 * host-buffer form. `rays` (n TraceResult, HOST memory) is read and overwritten in place exactly
 * as the reference overwrites the caller's ray stream (src/IpuScene.cpp:716-732). In path-trace
 * mode only rays[i].u/.v matter on input (camera rays are regenerated per sample on the device,
 * codelets/TraceCodelets.cpp:142-164); rgb comes back as the sum over samples_per_pixel samples.
 * In shadow-trace mode the given rays are traced as they are (Render.hpp:37-72).
 * `cb` (may be NULL) mirrors IpuScene::RayCallbackFn: it is called once per completed batch (see
 * mi_scene_set_ray_batch) with (user, batch_index, first_ray, ray_count), in batch order, on the calling
 * thread, while later batches are still being traced. The timed region (mi_trace_time_secs) here includes the
 * batch copies, which the pipeline overlaps with tracing. */
typedef void (*mi_ray_callback)(void* user, size_t batch_index, const mi_trace_result* rays, size_t count);
int mi_render(mi_scene* scene, int mode, mi_trace_result* rays, size_t n, mi_ray_callback cb, void* user);

/* Same operation on a DEVICE-resident ray stream (hipMalloc'ed / torch tensor memory), enqueued
 * on `hip_stream` (a hipStream_t passed as void*; NULL = the null stream). Asynchronous: returns
 * after enqueue. This is the entry bench.py times (inputs already resident in HBM).
 * Threading: a scene is thread-compatible (calls on ONE scene must not overlap in time on the host; different
 * scenes are independent). Launches of one scene enqueued on different streams own separate work counters and
 * partial-sum buffers and may execute concurrently; renders with a NIF environment share the scene's slot scratch
 * and are chained with an event, so they execute one after the other whatever streams they were enqueued on. */
int mi_render_device(mi_scene* scene, int mode, void* d_rays, size_t n, void* hip_stream);

/* Ray queries: CompactBvh::intersect (MI_QUERY_CLOSEST) / CompactBvh::occluded (MI_QUERY_ANY), CompactBvh.hpp:33-139, for each
 * of n caller-supplied rays with its own t_min / t_max - the reference's CPU path does the same with Embree's rtcIntersect1M /
 * rtcOccluded1M. Same visit order, same acceptance (t > t_min && t < closest), same NaN and infinite-inverse behaviour; no shading.
 * Device entry: d_rays = n mi_ray, d_out = n mi_query_hit (CLOSEST) or n uint8_t, 1 = occluded (ANY), DEVICE memory. Asynchronous
 * on hip_stream (a hipStream_t as void*; NULL = the null stream); the scene waits for it when destroyed.
 * Host entry: the same on HOST buffers, synchronous (copies + the device entry), in batches of mi_scene_set_ray_batch rays.
 * n == 0 is a no-op. MI_ERR_INVALID_ARG, before any device work: a null scene or buffer, an unknown kind, a buffer that is not
 * 16-byte aligned, or more rays in one launch (mi_query: in one batch) than the 32-bit work index allows (0xFFBFFFFF).
 * Counters (mi_get_counters): casts += n; nodes visited and leaf tests too under option full_stats. Options: query_kernel,
 * query_tune, and the arithmetic options double_fallback and fast, as for renders. */
int mi_query_device(mi_scene* scene, int kind, const void* d_rays, void* d_out, size_t n, void* hip_stream);
int mi_query(mi_scene* scene, int kind, const mi_ray* rays, void* out, size_t n);

/* Point queries: for each of n caller-supplied points with its own radius, the primitive of the scene's CURRENT BVH nearest to the
 * point and strictly within the radius, how far away it is and where on it (MI_POINT_CLOSEST, Embree's rtcPointQuery), or only
 * whether there is one (MI_POINT_WITHIN). Distances are to the SURFACE, as rays hit surfaces: a point inside a sphere is its
 * distance from the shell away.
 * Device entry: d_points = n mi_point, d_out = n mi_point_hit (CLOSEST) or n uint8_t, 1 = a primitive lies strictly within the
 * radius (WITHIN), DEVICE memory. Asynchronous on hip_stream (a hipStream_t as void*; NULL = the null stream); the scene waits for
 * it when destroyed, and mi_scene_update*, mi_scene_rebuild and mi_scene_set_geometry* wait for it before they overwrite a record:
 * a point query enqueued before one of them sees the old geometry.
 * Host entry: the same on HOST buffers, synchronous (copies + the device entry), in batches of mi_scene_set_ray_batch points.
 * n == 0 is a no-op. MI_ERR_INVALID_ARG, before any device work: a null scene or buffer, an unknown kind, a points buffer or a
 * CLOSEST out buffer that is not 16-byte aligned (the bytes of WITHIN need no alignment), or more points in one launch
 * (mi_point_query: in one batch) than the 32-bit work index allows (0xFFBFFFFF).
 * Arithmetic: binary32, one rounding per operation in the order written below, no contraction, correctly rounded divide and sqrt;
 * a dot product is (x x' + y y') + z z'. One definition (ipu_ray_lib_amd/csrc/point_math.hpp) serves the kernel and the host twin
 * mi_point_query_host (mi_scene_host.h), which returns the same bytes.
 * The walk is the stackless preorder walk of the ray kernels - first child first, whatever the point - with a distance test in place
 * of the slab test. best = radius * radius. At node nd: ex = fmaxf(fmaxf(nd.min.x - p.x, p.x - nd.max.x), 0), ey and ez alike,
 * db = (ex ex + ey ey) + ez ez; the node is entered when db < best, else passed. At a leaf so reached the primitive's closest
 * point q is evaluated, d2 = dot(p - q, p - q), and the leaf is accepted when d2 < best: strictly, so of equal distances the first
 * leaf in preorder wins and a NaN d2 is never accepted. CLOSEST sets best = d2 and walks on; WITHIN stops at the first accept.
 * Written without a walk, as "nothing found": a point with a coordinate that is not finite, a radius that is NaN or negative, an
 * empty scene. radius = +inf is legal (a box or primitive whose squared distance overflows to +inf is then never reached).
 * Triangle (a, b, c): Ericson, Real-Time Collision Detection 5.1.5. ab = b - a, ac = c - a; d1 = ab.(p - a), d2 = ac.(p - a),
 * d3 = ab.(p - b), d4 = ac.(p - b), d5 = ab.(p - c), d6 = ac.(p - c); vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.
 * Regions in this order, with the barycentrics (v, w): A: d1 <= 0 && d2 <= 0: (0, 0). B: d3 >= 0 && d4 <= d3: (1, 0).
 * AB: vc <= 0 && d1 >= 0 && d3 <= 0: (d1 / (d1 - d3), 0). C: d6 >= 0 && d5 <= d6: (0, 1). AC: vb <= 0 && d2 >= 0 && d6 <= 0:
 * (0, d2 / (d2 - d6)). BC: va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0: w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), (1 - w, w).
 * Face otherwise: den = 1 / ((va + vb) + vc), (vb den, vc den). q = (a + ab v) + ac w. A triangle collapsed to a point falls in
 * region A; nothing is special-cased.
 * Sphere (centre c): v = p - c, len = sqrtf(v.v); len > 0: q = c + v (radius / len), otherwise q = (c.x + radius, c.y, c.z).
 * Disc (centre c, normal n as given, as the ray test takes it, r2 = r r, r' = sqrtf(r2)): v = p - c, h = v.n, q0 = p - n h,
 * u = q0 - c, uu = u.u; uu <= r2: q = q0, otherwise q = c + u (r' / sqrtf(uu)).
 * Counters (mi_get_counters): nothing is added to casts or paths; under option full_stats the box tests are added to "nodes
 * visited" and the primitive evaluations to "leaf tests". Options: double_fallback, fast, query_kernel and query_tune do NOT apply
 * (there is one kernel and one arithmetic). Groups: call it on a replica's scene (mi_group_scene), as for ray queries. */
int mi_point_query_device(mi_scene* scene, int kind, const void* d_points, void* d_out, size_t n, void* hip_stream);
int mi_point_query(mi_scene* scene, int kind, const mi_point* points, void* out, size_t n);

/* Neighbour lists: EVERY primitive of the scene's CURRENT BVH strictly within the radius of each of n caller-supplied points, nearest
 * first (PCL's radiusSearch / nearestKSearch, Open3D's search_radius_vector_3d / search_knn_vector_3d, trimesh's nearby_faces) -
 * which mi_point_query (the nearest one, or whether there is one) cannot say. Two steps, as for the crossing lists (mi_list_*
 * below): the offsets of the points' segments, then the fill of a buffer the caller sized from them.
 * The record: dist2 = the SQUARED distance as the walk compares it (sqrtf is monotone but not injective: a list sorted by dist2 and
 * stored as distances would hide its own tie order), the ids as mi_point_hit carries them, flags = 0, point = the index of the query
 * the record belongs to. The empty record is {+inf, MI_INVALID_PRIM, MI_INVALID_GEOM, MI_FLAG_ESCAPED, point}. The closest point
 * itself is not in the record.
 * Acceptance: the walk, the box distance db, the closest point q of a primitive and d2 = dot(p - q, p - q) are mi_point_query's,
 * in its arithmetic (ipu_ray_lib_amd/csrc/point_math.hpp); r2 = radius * radius. A primitive is a neighbour exactly when its leaf
 * is reached and d2 < r2: strictly - a primitive exactly at the radius is not listed -, and a NaN d2 never qualifies. A query
 * mi_point_query does not walk (a coordinate that is not finite, a NaN or negative radius) and an empty scene have no neighbours;
 * radius = +inf is legal.
 * Order: by a key of the neighbour itself - dist2 as a float; then geom_id; then prim_id -, NOT by visit order: a list is the same
 * bytes after a refit, a rebuild or mi_scene_set_geometry of the same contents. MI_POINT_CLOSEST breaks ties by preorder instead, so
 * on an exact tie of distances its answer and a list's first record can name different primitives (at the same distance).
 * mi_near_offsets_device: d_points = n mi_point, d_offsets = n + 1 uint64_t, DEVICE memory. d_offsets[0] = 0, d_offsets[i + 1] -
 *   d_offsets[i] = the number of neighbours of point i, d_offsets[n] = their total (64 bit). The count walk runs over the FIXED
 *   bound: a node is entered when db < r2, so the set of neighbours is a function of the point and the geometry alone. Form: the
 *   count walk, then the crossing lists' prefix sum in place (their scratch per stream).
 * mi_near_fill_device: d_offsets = n + 1 uint64_t, d_hits = `capacity` mi_neighbour, DEVICE memory. Point i owns the records
 *   [d_offsets[i], d_offsets[i + 1]) cut at capacity; len = that length, 0 for a decreasing pair or a start at or past capacity,
 *   exactly as in mi_list_fill_device. NO record at an index >= capacity is ever written and none outside the segment, whatever the
 *   offsets hold. A point with len == 0 is not walked. Otherwise one thread per point walks with held = 0 records in its segment:
 *     a node is entered when db < r2 while held < len; once held == len, when db < r2 && db <= seg[len - 1].dist2 (<=: an
 *     equal-distance primitive with smaller ids must still displace the last record);
 *     an accepted neighbour (d2 < r2) is inserted at its sorted place in seg[0 .. held): appended while held < len; once held ==
 *     len it is dropped when it does not sort before seg[len - 1], and otherwise displaces that record;
 *   and what the walk leaves unused is padded with the empty record. The contract is THIS walk; mi_near_fill_host runs it
 *   statement for statement. With offsets from mi_near_offsets* a segment is full only once the point's last neighbour is placed,
 *   so the fill gives exactly the fixed-radius walk's list: every neighbour, sorted (the boxes it passes from then on hold no
 *   neighbour; under full_stats it counts no more visits than the offsets' walk). With d_offsets[i] = K i it is a K-nearest query within the radius, padded; with
 *   radius = +inf the K nearest primitives, at a cost that shrinks with the bound instead of a walk of the whole tree.
 *   Mathematically the pruned result is the len smallest of the unpruned list; that is stated as a property, not as the definition,
 *   because a box distance db and the distance d2 of a primitive inside the box are each rounded, and db <= d2 is not guaranteed to
 *   the last ulp in binary32. Overlapping segments of different points give unspecified records inside them.
 * Host entries: the same on HOST buffers, synchronous, in batches of mi_scene_set_ray_batch points; offsets and the `point` field
 *   are global across batches (`point` is the index modulo 2^32). They share mi_list_fill's device staging.
 * Ordering, destruction, groups, batches and stream rules: those of mi_point_query_device / mi_point_query. n == 0 is a no-op.
 * MI_ERR_INVALID_ARG, before any device work and without reading the scene: a null scene or buffer, points or hits that are not
 * 16-byte aligned, offsets that are not 8-byte aligned, or more points in one launch (host entries: in one batch) than the 32-bit
 * work index allows (0xFFBFFFFF).
 * Options: none apply (one kernel, one arithmetic, as for point queries). Counters: nothing is added to casts or paths; under
 * full_stats the box tests are added to "nodes visited" and the primitive evaluations to "leaf tests". */
typedef struct { float dist2; uint32_t primID; uint16_t geomID; uint16_t flags; uint32_t point; } mi_neighbour;   /* 16 B */
int mi_near_offsets_device(mi_scene* scene, const void* d_points, uint64_t* d_offsets /* n + 1 */, size_t n, void* hip_stream);
int mi_near_fill_device(mi_scene* scene, const void* d_points, const uint64_t* d_offsets, mi_neighbour* d_hits, size_t capacity, size_t n, void* hip_stream);
int mi_near_offsets(mi_scene* scene, const mi_point* points, uint64_t* offsets /* n + 1 */, size_t n);
int mi_near_fill(mi_scene* scene, const mi_point* points, const uint64_t* offsets, mi_neighbour* hits, size_t capacity, size_t n);

/* Crossing counts: for each of n caller-supplied rays, how many surfaces of the scene's CURRENT BVH it crosses with t_min < t < t_max
 * (Open3D's count_intersections). A closest-hit cast prunes what lies behind its hit and cannot say this; callers of mi_query would
 * need one round trip per surface layer.
 * Device entry: d_rays = n mi_ray, d_counts = n uint32_t, DEVICE memory. Asynchronous on hip_stream (a hipStream_t as void*; NULL =
 * the null stream); ordering, destruction, groups and batches are those of mi_query_device / mi_query: the scene waits for it when
 * destroyed, updates, rebuilds and set-geometry wait for it before they overwrite a record, and on a group it is called on a
 * replica's scene (mi_group_scene).
 * Host entry: the same on HOST buffers, synchronous (copies + the device entry), in batches of mi_scene_set_ray_batch rays.
 * n == 0 is a no-op; an empty scene gives zeros. MI_ERR_INVALID_ARG, before any device work and without reading the scene: a null
 * scene or buffer, rays that are not 16-byte aligned, counts that are not 4-byte aligned, or more rays in one launch
 * (mi_count_query: in one batch) than the 32-bit work index allows (0xFFBFFFFF).
 * The walk is the stackless preorder walk of the ray queries with their box test (CompactBVH2Node.cpp:5-22, the literal per-axis
 * sequence) over the FIXED interval [t_min, t_max]: it never shrinks, so the leaves visited are a function of the ray and the nodes
 * alone, and the count - a sum over them - does not depend on the visit order. A visited leaf adds
 *   triangle, disc: 1 when the ray query's primitive test accepts it against t_max: t > t_min && t < t_max (and t > 0 && t < inf for
 *     a triangle, Mesh.hpp:93);
 *   sphere (centre c, radius2 = radius radius): 0, 1 or 2, both roots - the reference's sphere test returns one t per sphere and
 *     misses when the centre lies behind the origin, even for an origin inside the sphere. In binary32, one rounding per operation,
 *     a dot product (x x' + y y') + z z' (ipu_ray_lib_amd/csrc/cross_math.hpp; mi_sphere_crossings_host in mi_scene_host.h runs it
 *     on the host): f = c - o; dd = d.d; tca = (f.d) / dd; l = f - d tca; l2 = l.l; !(l2 <= radius2): 0; otherwise
 *     td = sqrtf((radius2 - l2) / dd), t0 = tca - td, t1 = tca + td, and the count is (t0 > t_min && t0 < t_max) + (t1 > t_min &&
 *     t1 < t_max). No tca < 0 early-out; right for any length of d; a tangent ray (td == 0) adds 0 or 2, so a parity survives it; a
 *     NaN never counts.
 * On a scene without spheres count > 0 holds exactly when MI_QUERY_ANY answers 1 for the same ray (same boxes visited until the
 * first accept, same acceptance).
 * Options: double_fallback applies, with its triangle test (it matters most exactly here, where an edge function is zero); fast,
 * query_kernel and query_tune do NOT apply (one kernel, the exact arithmetic). Counters (mi_get_counters): casts += n; under
 * full_stats the box tests and primitive tests are added as for ray queries (double_fallback has no instrumented build and takes
 * precedence, as for ray queries). */
int mi_count_query_device(mi_scene* scene, const void* d_rays, uint32_t* d_counts, size_t n, void* hip_stream);
int mi_count_query(mi_scene* scene, const mi_ray* rays, uint32_t* counts, size_t n);

/* Inside tests and signed distance: whether each of n caller-supplied points lies inside the scene's surfaces (MI_SIGN_INSIDE,
 * Open3D's compute_occupancy, trimesh's contains) and its distance from them with that sign (MI_SIGN_DISTANCE, Open3D's
 * compute_signed_distance).
 * A point is inside when the crossing count (above) of the ray origin = the point, direction = dir, t_min = 0, t_max = +inf is odd:
 * the walk and the arithmetic of mi_count_query, option double_fallback likewise.
 * dir: a HOST pointer to three floats, read before the call returns; NULL = {1.0f, 0.70710678f, 0.57735027f}. A component that is
 * zero, NaN or infinite is refused: the reference's triangle test shears by the SMALLEST signed direction component
 * (Primitives.cpp:5-22), so an axis direction such as (1, 0, 0) divides by zero there and misses every triangle. The default's
 * components are 1, 1/sqrt 2 and 1/sqrt 3: rays from grid points do not run through the edges and face diagonals of axis-aligned boxes,
 * as those of a direction such as (1, 0.618034, 0.381966), whose components sum to 1, do. A caller who wants a majority vote calls three times with three directions.
 * MI_SIGN_INSIDE: d_out = n uint8_t, 1 = inside. The radius is ignored. A point with a coordinate that is not finite is not walked
 * and gets 0.
 * MI_SIGN_DISTANCE: d_out = n mi_point_hit, 16-byte aligned: byte for byte what MI_POINT_CLOSEST writes for the same point and
 * radius, except where the point is inside: there the sign bit of dist is set and flags |= MI_FLAG_INSIDE. When nothing lies within
 * the radius dist is the radius as given with MI_FLAG_ESCAPED, and still negative with MI_FLAG_INSIDE for a point inside: a
 * narrow-band caller gets -radius. A query a point query does not walk (a coordinate that is not finite, a NaN or negative radius)
 * is not walked for crossings either: its record is MI_POINT_CLOSEST's "nothing found", unchanged.
 * Meaning: only closed surfaces have an inside. A disc or an open mesh counts as one crossing and means what the caller makes of
 * it; a point closer to a surface than the triangle test's own error bound (t <= deltaT, Mesh.cpp) can fall on either side.
 * Form: MI_SIGN_DISTANCE is two launches on hip_stream - the point query, then the crossing walk, which changes the records in
 * place -; MI_SIGN_INSIDE is the walk alone. Ordering, destruction, groups, batches and the argument rules are those of
 * mi_point_query_device / mi_point_query (an unknown kind: "unknown sign kind"; the bytes of MI_SIGN_INSIDE need no alignment); a
 * refused dir is MI_ERR_INVALID_ARG before any device work, too.
 * Counters: the point query counts as mi_point_query does; the walk adds the points it walked to casts and, under full_stats, its
 * box tests and primitive tests to "nodes visited" and "leaf tests". */
#define MI_FLAG_INSIDE ((uint16_t)4)
enum { MI_SIGN_INSIDE = 0, MI_SIGN_DISTANCE = 1 };
int mi_point_sign_device(mi_scene* scene, int kind, const void* d_points, void* d_out, const float dir[3], size_t n, void* hip_stream);
int mi_point_sign(mi_scene* scene, int kind, const mi_point* points, void* out, const float dir[3], size_t n);

/* Crossing lists: EVERY crossing of each of n caller-supplied rays with t_min < t < t_max, sorted along the ray (Open3D's
 * list_intersections) - where a ray enters and leaves things, which mi_query (the first crossing) and mi_count_query (their number)
 * cannot say. Two steps: the offsets of the rays' segments, then the fill of a buffer the caller sized from them.
 * The record: t, the ids as mi_query_hit carries them, flags = 0 or MI_CROSS_FAR (a sphere's far root t1; its near root t0 carries
 * 0), ray = the index of the ray the record belongs to. The empty record is {+inf, MI_INVALID_PRIM, MI_INVALID_GEOM,
 * MI_FLAG_ESCAPED, ray}.
 * Acceptance: a crossing is listed exactly when mi_count_query counts it - the same walk over the FIXED interval, the same box
 * test, primitive test and double_fallback behaviour; a sphere gives both roots of the formula above with their t (sphere_roots in
 * ipu_ray_lib_amd/csrc/cross_math.hpp, mi_sphere_roots_host in mi_scene_host.h). The set of crossings is therefore a function of
 * the ray and the geometry alone, and the order is by a key of the crossing itself - t; then geom_id; then prim_id; then a sphere's
 * near root before its far root (t compares as a float: -0 == +0) -, so a list is the same bytes after a refit, a rebuild or
 * mi_scene_set_geometry of the same contents.
 * mi_list_offsets_device: d_rays = n mi_ray, d_offsets = n + 1 uint64_t, DEVICE memory. d_offsets[0] = 0, d_offsets[i + 1] -
 *   d_offsets[i] = the crossing count of ray i (mi_count_query's), d_offsets[n] = their total. 64 bit: no total overflows. Form: the
 *   count walk, then a prefix sum in place (three small launches; scratch per stream, grown on demand, kept by the scene).
 * mi_list_fill_device: d_offsets = n + 1 uint64_t, d_hits = `capacity` mi_crossing, DEVICE memory. Ray i owns the records
 *   [d_offsets[i], d_offsets[i + 1]); len = that length, 0 for a decreasing pair. The segment receives the ray's crossings in
 *   ascending order of the key; when the ray has more than len, the len smallest; when it has fewer, the rest is filled with the
 *   empty record. NO record at an index >= capacity is ever written, whatever the offsets hold: a segment is cut at capacity (it
 *   then holds the smallest crossings that fit). The offsets may come from mi_list_offsets_device - every crossing - or from the
 *   caller: d_offsets[i] = K i gives the first K crossings of every ray, padded. Offsets made for one state of the scene and
 *   filled against another are legal: truncated or padded segments. Offsets that make segments of different rays overlap give
 *   unspecified records inside those segments, and still no write outside them.
 *   Form: one thread per ray inserts each crossing at its sorted place in the ray's own segment: O(crossings x len) record moves.
 * Host entries: the same on HOST buffers, synchronous, in batches of mi_scene_set_ray_batch rays; offsets and the `ray` field are
 *   global across batches (`ray` is the index modulo 2^32). The device staging of the hits grows on demand and goes with the scene.
 * Ordering, destruction and groups: those of mi_count_query_device. n == 0 is a no-op; an empty scene gives zero offsets and padded
 * segments. MI_ERR_INVALID_ARG, before any device work and without reading the scene: a null scene or buffer, rays or hits that
 * are not 16-byte aligned, offsets that are not 8-byte aligned, or more rays in one launch (host entries: in one batch) than the
 * 32-bit work index allows (0xFFBFFFFF).
 * Options: double_fallback applies; fast, query_kernel and query_tune do NOT. Counters: each of the four calls adds n to casts and,
 * under full_stats, its box tests and primitive tests (the fill's equal the offsets' and mi_count_query's for the same rays). */
typedef struct { float t; uint32_t primID; uint16_t geomID; uint16_t flags; uint32_t ray; } mi_crossing;   /* 16 B */
#define MI_CROSS_FAR ((uint16_t)8)   /* a sphere's far root t1 */
int mi_list_offsets_device(mi_scene* scene, const void* d_rays, uint64_t* d_offsets /* n + 1 */, size_t n, void* hip_stream);
int mi_list_fill_device(mi_scene* scene, const void* d_rays, const uint64_t* d_offsets, mi_crossing* d_hits, size_t capacity, size_t n, void* hip_stream);
int mi_list_offsets(mi_scene* scene, const mi_ray* rays, uint64_t* offsets /* n + 1 */, size_t n);
int mi_list_fill(mi_scene* scene, const mi_ray* rays, const uint64_t* offsets, mi_crossing* hits, size_t capacity, size_t n);

/* Box queries: the primitives of the scene's CURRENT BVH that TOUCH each of n caller-supplied axis-aligned boxes [lo, hi] - a voxel
 * (Open3D's VoxelGrid.create_from_triangle_mesh, trimesh's voxelize), a culling or selection cell, a broad-phase cell or a moving
 * body's bounds (PCL's boxSearch, a physics engine's overlap-box). Every other query here is a ray or a ball; a caller with a box had
 * to ask mi_near_* about the circumscribed ball and filter. Whether there is one (MI_BOX_ANY), how many (MI_BOX_COUNT), or which:
 * two steps as for the neighbour lists - the offsets of the boxes' segments, then the fill of a buffer the caller sized from them.
 * Touching is CLOSED everywhere: contact counts. Queries see SURFACES, as everywhere in this library: a box wholly inside a sphere,
 * away from its shell, does not touch it.
 * The box: lo[3] and hi[3]; reserved0 and reserved1 are not read. The record: the ids as mi_point_hit carries them, flags = 0 or
 * MI_OVERLAP_CONTAINED (the primitive's own bounds, as defined below, lie inside the box, faces included), box = the index of the
 * query the record belongs to, reserved = 0. The empty record is {MI_INVALID_PRIM, MI_INVALID_GEOM, MI_FLAG_ESCAPED, box, 0}.
 * Arithmetic: binary32, one rounding per operation in the order written below, no contraction, correctly rounded divide and sqrt;
 * a dot product is (x x' + y y') + z z'; min and max are compare / select pairs (a < b ? a : b, a > b ? a : b). One definition
 * (ipu_ray_lib_amd/csrc/box_math.hpp) serves the kernels and the host twins (mi_scene_host.h), which return the same bytes.
 * Validity: a box with a coordinate that is NaN or infinite, or with lo > hi on an axis, is not walked and finds nothing; so does
 * an empty scene. lo == hi on an axis is legal: a plane, a line, a point.
 * The walk is the stackless preorder walk of the point queries - first child first, whatever the box. A node nd is entered when
 * nd.min <= hi && nd.max >= lo on all three axes (compares, no arithmetic), else passed. At a leaf so reached the primitive is
 * tested; MI_BOX_ANY stops at the first one that touches.
 * Every primitive test starts with the primitive's OWN bounds [mn, mx] against the box, in the same compares: not touching unless
 * mn <= hi && mx >= lo on all axes; CONTAINED exactly when mn >= lo && mx <= hi on all axes.
 * Triangle (a, b, c): mn, mx = the per-axis min and max of the vertices (no arithmetic: the bounds test and CONTAINED are exact).
 *   Touching at once when a vertex v has lo <= v <= hi on all axes. Otherwise Akenine-Moller's separating-axis test in centre /
 *   half-extent form: cb = 0.5 lo + 0.5 hi, h = 0.5 hi - 0.5 lo, v0 = a - cb, v1 = b - cb, v2 = c - cb, e0 = v1 - v0, e1 = v2 - v1,
 *   e2 = v0 - v2. For e = e0, e1, e2 in turn, with p_i over the three moved vertices:
 *     p_i = e.y v_i.z - e.z v_i.y, r = h.y |e.z| + h.z |e.y|;   p_i = e.z v_i.x - e.x v_i.z, r = h.x |e.z| + h.z |e.x|;
 *     p_i = e.x v_i.y - e.y v_i.x, r = h.x |e.y| + h.y |e.x|;
 *   then the plane: nrm = cross(e0, e1), p = nrm.v0 (for all three), r = (h.x |nrm.x| + h.y |nrm.y|) + h.z |nrm.z|. An axis separates
 *   when min p_i > r || max p_i < -r, evaluated as (p_0 > r && p_1 > r && p_2 > r) || (p_0 < -r && p_1 < -r && p_2 < -r): a NaN
 *   never separates, so a box so large that its products overflow errs towards listing. The triangle touches when no axis separates
 *   (the box's own three axes were the bounds test). A collapsed triangle needs no special case: zero axes separate nothing.
 * Sphere (centre c, radius, r2 = radius radius as the scene holds it): mn = c - radius, mx = c + radius (one rounded operation
 *   each). dmin2 = mi_point_query's box distance db of c from [lo, hi]; per axis f = max(|c - lo|, |hi - c|), dmax2 = (fx fx + fy fy)
 *   + fz fz, the squared distance of the farthest corner. Touching when !(dmin2 > r2) && !(dmax2 < r2): the shell is reached from
 *   outside and from inside.
 * Disc (centre c, normal n as given, r2 = r r as the scene holds it): CONSERVATIVE - three necessary conditions that must all hold.
 *   r' = sqrtf(r2), nn = n.n, per axis t = 1 - n_i n_i / nn, t = t > 0 ? t : 0, half extent r' sqrtf(t): mn = c - ext, mx = c + ext,
 *   the disc's tight bounds, which the box must meet (and which decide CONTAINED). The box meets the disc's plane: s = n.(cb - c),
 *   rr = (h.x |n.x| + h.y |n.y|) + h.z |n.z|, !(|s| > rr). The box meets the ball of radius r about c: !(db of c > r2). No touching
 *   disc is missed, up to the rounding of these operations; a box that passes the disc's rim within its own size may list it without
 *   touching it. An exact disc test is not offered.
 * Order: records are sorted by the key (geom_id, prim_id), ascending; keys are unique within a box. This IS the definition - there is
 * no distance bound to round -: a segment shorter than the box's count holds the len smallest keys, and a list is the same bytes
 * after a refit, a rebuild or mi_scene_set_geometry of the same contents.
 * mi_box_query_device: d_boxes = n mi_box, d_out = n uint8_t, 1 = a primitive touches the box (MI_BOX_ANY; the bytes need no
 *   alignment) or n uint32_t counts (MI_BOX_COUNT), DEVICE memory.
 * mi_box_offsets_device: d_offsets = n + 1 uint64_t: d_offsets[0] = 0, d_offsets[i + 1] - d_offsets[i] = the count of box i,
 *   d_offsets[n] = their total (64 bit). Form: the count walk, then the crossing lists' prefix sum in place (their scratch per stream).
 * mi_box_fill_device: d_offsets = n + 1 uint64_t, d_hits = `capacity` mi_overlap, DEVICE memory. Box i owns the records
 *   [d_offsets[i], d_offsets[i + 1]) cut at capacity; len = that length, 0 for a decreasing pair or a start at or past capacity,
 *   exactly as in mi_near_fill_device. NO record at an index >= capacity is ever written and none outside the segment, whatever the
 *   offsets hold. A box with len == 0 is not walked. Otherwise the segment receives the len smallest keys of the box's touching
 *   primitives, ascending, and what they leave unused is the empty record. The key has no spatial bound, so the fill walks exactly
 *   what the count walk walks: under full_stats its visits equal mi_box_offsets' over the boxes whose segment is not empty.
 *   Caller-made offsets are legal: d_offsets[i] = K i gives the K smallest keys of every box, padded. Overlapping segments of
 *   different boxes give unspecified records inside them.
 *   Form: one thread per box keeps the len smallest keys as a binary max-heap inside the segment - O(count log len) record moves,
 *   where an insertion sort would move O(count len) - and heap-sorts it in place.
 * Host entries: the same on HOST buffers, synchronous, in batches of mi_scene_set_ray_batch boxes; offsets and the `box` field are
 *   global across batches (`box` is the index modulo 2^32). The fill shares mi_list_fill's device staging.
 * Asynchrony, ordering against update / rebuild / set-geometry, destruction, groups, batches and stream rules: those of
 * mi_point_query_device / mi_point_query and mi_near_*. n == 0 is a no-op. MI_ERR_INVALID_ARG, before any device work and without
 * reading the scene: a null scene or buffer, an unknown kind ("unknown box kind"), boxes or hits that are not 16-byte aligned, counts
 * that are not 4-byte aligned, offsets that are not 8-byte aligned, or more boxes in one launch (host entries: in one batch) than the
 * 32-bit work index allows (0xFFBFFFFF).
 * Options: none apply (one kernel, one arithmetic). Counters: nothing is added to casts or paths; under full_stats the box tests are
 * added to "nodes visited" and the primitive tests to "leaf tests". */
typedef struct { float lo[3]; uint32_t reserved0; float hi[3]; uint32_t reserved1; } mi_box;      /* 32 B, 16-byte aligned loads */
typedef struct { uint32_t primID; uint16_t geomID; uint16_t flags; uint32_t box; uint32_t reserved; } mi_overlap;   /* 16 B */
#define MI_OVERLAP_CONTAINED ((uint16_t)16)   /* the primitive's own bounds lie inside the box (closed) */
enum { MI_BOX_ANY = 0, MI_BOX_COUNT = 1 };
int mi_box_query_device(mi_scene* scene, int kind, const void* d_boxes, void* d_out, size_t n, void* hip_stream);
int mi_box_query(mi_scene* scene, int kind, const mi_box* boxes, void* out, size_t n);
int mi_box_offsets_device(mi_scene* scene, const void* d_boxes, uint64_t* d_offsets /* n + 1 */, size_t n, void* hip_stream);
int mi_box_fill_device(mi_scene* scene, const void* d_boxes, const uint64_t* d_offsets, mi_overlap* d_hits, size_t capacity, size_t n, void* hip_stream);
int mi_box_offsets(mi_scene* scene, const mi_box* boxes, uint64_t* offsets /* n + 1 */, size_t n);
int mi_box_fill(mi_scene* scene, const mi_box* boxes, const uint64_t* offsets, mi_overlap* hits, size_t capacity, size_t n);

/* Triangle queries: the primitives of the scene's CURRENT BVH that TOUCH each of n caller-supplied triangles (q0, q1, q2) - a face of
 * another mesh (Embree's rtcCollide, trimesh / FCL's collision manager, libigl's intersection tests), a facet of a cutting surface.
 * A caller with a triangle had to ask mi_box_* about its bounding box and filter with a triangle-triangle test of their own; a
 * diagonal triangle's box lists many times what the triangle touches. Whether there is one (MI_TRI_ANY), how many (MI_TRI_COUNT), or
 * which: two steps as for the box lists - the offsets of the triangles' segments, then the fill of a buffer the caller sized from them.
 * Touching is CLOSED everywhere: contact counts. Queries see SURFACES, as everywhere in this library: a triangle wholly inside a
 * sphere, away from its shell, touches nothing.
 * The triangle: a[3], b[3], c[3] = q0, q1, q2, 36 bytes at a 4-byte aligned address: a float32 [n, 3, 3] array (vertices[faces]) IS a
 * batch. The record has the layout of mi_overlap: the ids as mi_point_hit carries them, flags = 0, tri = the index of the query the
 * record belongs to, reserved = 0. The empty record is {MI_INVALID_PRIM, MI_INVALID_GEOM, MI_FLAG_ESCAPED, tri, 0}.
 * Arithmetic: binary32, one rounding per operation in the order written below, no contraction, correctly rounded divide and sqrt;
 * a dot product is (x x' + y y') + z z', cross(a, v) = (a.y v.z - a.z v.y, a.z v.x - a.x v.z, a.x v.y - a.y v.x); min and max are
 * compare / select pairs (a < b ? a : b, a > b ? a : b). Every separation is a strict compare that a NaN fails: a NaN never separates,
 * and a query so large that its products overflow errs towards listing. One definition (ipu_ray_lib_amd/csrc/contact_math.hpp) serves
 * the kernels and the host twins (mi_scene_host.h), which return the same bytes.
 * Validity: a triangle with a coordinate that is NaN or infinite is not walked and finds nothing; so does an empty scene. A collapsed
 * query (a segment, a point) is legal.
 * The walk is the stackless preorder walk of the box queries. qmn, qmx = the per-axis select-min and select-max of the query's
 * vertices ((q0 ? q1) ? q2). A node nd is entered when nd.min <= qmx && nd.max >= qmn on all three axes (compares, no arithmetic),
 * else passed: the visited set is a function of the query's bounds alone (no plane test at the nodes). At a leaf so reached the
 * primitive is tested; MI_TRI_ANY stops at the first one that touches.
 * Every primitive test starts with the primitive's OWN bounds [mn, mx] - those mi_box_* defines for that kind of primitive - against
 * [qmn, qmx], in the same compares: not touching unless mn <= qmx && mx >= qmn on all axes.
 * Scene triangle (a, b, c): a separating-axis test of 17 axes, relative to q0. u0 = a - q0, u1 = b - q0, u2 = c - q0; v0 = (0, 0, 0),
 *   v1 = q1 - q0, v2 = q2 - q0. e0 = u1 - u0, e1 = u2 - u1, e2 = u0 - u2; f0 = v1, f1 = v2 - v1, f2 = -v2. nT = cross(e0, e1),
 *   nQ = cross(f0, f1). The axes, in this order: nQ; nT; cross(e_i, f_j) for i = 0..2 (outer), j = 0..2 (inner); cross(nT, e_i) for
 *   i = 0..2; cross(nQ, f_j) for j = 0..2. For an axis x: pT_i = dot(x, u_i), pQ_0 = 0.f, pQ_j = dot(x, v_j); x separates exactly
 *   when pT_i > pQ_j for all nine pairs or pT_i < pQ_j for all nine pairs. The triangles touch when no axis separates. The last six
 *   axes are what decides coplanar pairs. A zero axis has all projections 0 and separates nothing, so a collapsed triangle errs
 *   towards listing: nothing is special-cased.
 * Sphere (centre c, radius, r2 = radius radius as the scene holds it): dmin2 = dot(d, d), d = c - q, q = mi_point_query's closest
 *   point of the triangle (q0, q1, q2) to c; dmax2 = the select-max ((d_0 ? d_1) ? d_2) of d_i = dot(q_i - c, q_i - c). Touching when
 *   !(dmin2 > r2) && !(dmax2 < r2): the shell is reached from outside and from inside.
 * Disc (centre c, normal n as given, r2): CONSERVATIVE, as for boxes - three necessary conditions that must all hold. The disc's
 *   tight bounds (mi_box_*'s) meet [qmn, qmx]. The triangle meets the plane: s_i = dot(n, q_i - c), not all three > 0 and not all
 *   three < 0. The triangle meets the ball: !(dmin2 of c > r2). No touching disc is missed, up to the rounding of these operations; a
 *   triangle that passes the rim may be listed without touching it. An exact disc test is not offered.
 * Order: records are sorted by the key (geom_id, prim_id), ascending; keys are unique within a query. This IS the definition: a
 * segment shorter than the triangle's count holds the len smallest keys, and a list is the same bytes after a refit, a rebuild or
 * mi_scene_set_geometry of the same contents.
 * mi_tri_query_device: d_tris = n mi_tri, d_out = n uint8_t, 1 = a primitive touches the triangle (MI_TRI_ANY; the bytes need no
 *   alignment) or n uint32_t counts (MI_TRI_COUNT), DEVICE memory.
 * mi_tri_offsets_device / mi_tri_fill_device: offsets, segments, the cut at capacity (NO record at an index >= capacity is ever
 *   written and none outside the segment), a decreasing pair = an empty segment, which is not walked, caller-made offsets (K i = the K
 *   smallest keys of every triangle, padded), overlapping segments (unspecified records inside them) and the form (a max-heap inside
 *   the segment, heap-sorted in place) are mi_box_offsets_device's and mi_box_fill_device's, with d_hits = `capacity` mi_contact.
 * Host entries: the same on HOST buffers, synchronous, in batches of mi_scene_set_ray_batch triangles; offsets and the `tri` field are
 *   global across batches (`tri` is the index modulo 2^32). The fill shares mi_list_fill's device staging.
 * Asynchrony, ordering against update / rebuild / set-geometry, destruction, groups, batches and stream rules: those of mi_box_*.
 * n == 0 is a no-op. MI_ERR_INVALID_ARG, before any device work and without reading the scene: a null scene or buffer, an unknown kind
 * ("unknown triangle kind"), triangles that are not 4-byte aligned ("triangles must be 4-byte aligned"), counts that are not 4-byte
 * aligned, offsets that are not 8-byte aligned, hits that are not 16-byte aligned, or more triangles in one launch (host entries: in
 * one batch) than the 32-bit work index allows (0xFFBFFFFF).
 * Options: none apply (one kernel, one arithmetic). Counters: nothing is added to casts or paths; under full_stats the box tests are
 * added to "nodes visited" and the primitive tests to "leaf tests". */
typedef struct { float a[3], b[3], c[3]; } mi_tri;   /* 36 B, 4-byte aligned: a float32 [n,3,3] array IS a batch */
typedef struct { uint32_t primID; uint16_t geomID; uint16_t flags; uint32_t tri; uint32_t reserved; } mi_contact;  /* 16 B, layout of mi_overlap */
enum { MI_TRI_ANY = 0, MI_TRI_COUNT = 1 };
int mi_tri_query_device(mi_scene* scene, int kind, const void* d_tris, void* d_out, size_t n, void* hip_stream);
int mi_tri_query(mi_scene* scene, int kind, const mi_tri* tris, void* out, size_t n);
int mi_tri_offsets_device(mi_scene* scene, const void* d_tris, uint64_t* d_offsets /* n + 1 */, size_t n, void* hip_stream);
int mi_tri_fill_device(mi_scene* scene, const void* d_tris, const uint64_t* d_offsets, mi_contact* d_hits, size_t capacity, size_t n, void* hip_stream);
int mi_tri_offsets(mi_scene* scene, const mi_tri* tris, uint64_t* offsets /* n + 1 */, size_t n);
int mi_tri_fill(mi_scene* scene, const mi_tri* tris, const uint64_t* offsets, mi_contact* hits, size_t capacity, size_t n);

/* Oriented-box queries: the primitives of the scene's CURRENT BVH that TOUCH each of n caller-supplied ROTATED boxes - a rigid body's
 * bounding box, a robot link, a beam, a selection volume, a voxel of a rotated grid, a portal (FCL's and Bullet's OBB, Open3D's
 * OrientedBoundingBox). A caller with such a box had to ask mi_box_* about its world bounds and filter; a long box on a diagonal
 * lists many times what it touches. Whether there is one (MI_OBOX_ANY), how many (MI_OBOX_COUNT), or which: two steps as for the box
 * lists - the offsets of the boxes' segments, then the fill of a buffer the caller sized from them.
 * Touching is CLOSED everywhere: contact counts. Queries see SURFACES, as everywhere in this library.
 * The oriented box: centre[3], half[3] (the half extents along the box's own axes) and quat[4] = x, y, z, w, the rotation that turns
 * an axis-aligned box into this one (U, V, W below are the box's axes in world coordinates); reserved0 and reserved1 are not read. The quaternion NEED NOT BE UNIT: the frame below is orthogonal
 * for any non-zero quaternion, which is why the orientation is a quaternion and not nine floats a caller could get wrong. The record
 * is mi_overlap: the ids as mi_point_hit carries them, flags = 0 or MI_OVERLAP_CONTAINED, box = the index of the query the record
 * belongs to, reserved = 0. The empty record is {MI_INVALID_PRIM, MI_INVALID_GEOM, MI_FLAG_ESCAPED, box, 0}.
 * Arithmetic: binary32, one rounding per operation in the order written below, no contraction, correctly rounded divide (and sqrt,
 * in the disc's bounds); dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z. Every separation is a strict compare that a NaN fails: a NaN
 * never separates, and a query so large that its products overflow errs towards listing. One definition
 * (ipu_ray_lib_amd/csrc/obox_math.hpp, over box_math.hpp) serves the kernels and the host twins (mi_scene_host.h), which return the
 * same bytes.
 * Validity: a query is valid when all ten floats are finite, half >= 0 on every axis, qq = ((x x + y y) + z z) + w w > 0 and
 *   s = 2.f / qq is finite. Any other query is not walked and finds nothing; so does an empty scene. A zero half extent is legal: a
 *   rectangle, a segment, a point. The two ends of the quaternion's range are not alike: a norm below about 1e-19 makes s overflow and
 *   the query invalid, but a finite quaternion whose SQUARED NORM overflows (a norm above about 1.8e19) gives qq = +inf and s = 0, which
 *   is finite: the query is valid, every product of the frame is 0 and the frame is the IDENTITY, whatever rotation the quaternion
 *   stood for. Nothing is rescaled. A caller whose quaternions can be that large scales them down first (any positive scale keeps the
 *   rotation).
 * The frame: xs = x s, ys = y s, zs = z s; wx = w xs, wy = w ys, wz = w zs; xx = x xs, xy = x ys, xz = x zs, yy = y ys, yz = y zs,
 *   zz = z zs; U = (1 - (yy + zz), xy + wz, xz - wy), V = (xy - wz, 1 - (xx + zz), yz + wx), W = (xz + wy, yz - wx, 1 - (xx + yy)).
 *   A point p has the local coordinates (dot(U, d), dot(V, d), dot(W, d)), d = p - centre; a direction rotates the same way without
 *   the subtraction.
 * The query's world bounds: ext.x = (|U.x| half.x + |V.x| half.y) + |W.x| half.z, likewise y and z; qmn = centre - ext,
 *   qmx = centre + ext.
 * The bounds test obox_meets_bounds(mn, mx), used at every node and, unchanged, as the first step at every leaf on the primitive's
 *   own bounds: first the six closed compares of mi_box_* against [qmn, qmx] (mn <= qmx && mx >= qmn on all axes). Then
 *   dl = mn - centre, dh = mx - centre, and for each axis A of U, V, W with its half extent hA: up = (t0 + t1) + t2 with
 *   t_k = A_k > 0 ? A_k dh_k : A_k dl_k; dn the same with dl and dh exchanged; the axis separates when dn > hA || up < -hA. The
 *   bounds are met when the six compares hold and no axis separates. The test has no other arithmetic.
 * The walk is the stackless preorder walk of the box queries. A node is entered when obox_meets_bounds of its box holds, else passed.
 * At a leaf so reached the primitive is tested; MI_OBOX_ANY stops at the first one that touches.
 * Primitive test, two steps. 1: obox_meets_bounds on the primitive's OWN bounds - those mi_box_* defines for that kind of primitive.
 *   2: mi_box_*'s test of that kind, exactly as it stands, in the box's frame with lo = -half, hi = half: a triangle's three vertices,
 *   a sphere's centre, a disc's centre and normal are moved into the frame first (radius and r2 are kept). There cb is an exact zero
 *   and h is exactly half. MI_OVERLAP_CONTAINED is what that test reports: for a triangle it is exact - all three moved vertices lie
 *   in the box, faces included -, for a sphere and a disc it is decided by their bounds about the moved centre; the disc stays
 *   conservative as everywhere else. A flat or collapsed box errs towards listing; mi_tri_* is the exact answer for flat queries.
 * Order: records are sorted by the key (geom_id, prim_id), ascending; keys are unique within a query. This IS the definition: a
 * segment shorter than the box's count holds the len smallest keys, and a list is the same bytes after a refit, a rebuild or
 * mi_scene_set_geometry of the same contents. The node test has arithmetic, so this needs an argument: fl(a - c), fl(x a) for a fixed
 * x and fl(a + b) are monotone in a and b, so for bounds A that contain bounds B every t_k of up is no smaller and every t_k of dn no
 * larger for A than for B, and so are the sums as computed: up(A) >= up(B), dn(A) <= dn(B). Whatever B does not separate, A does not,
 * and the six compares nest likewise. A node's device box contains its primitives' bounds as those functions compute them - the fact
 * the box family rests on -, so a primitive whose own bounds pass has every ancestor's box pass, whatever tree is walked.
 * mi_obox_query_device: d_oboxes = n mi_obox, d_out = n uint8_t, 1 = a primitive touches the box (MI_OBOX_ANY; the bytes need no
 *   alignment) or n uint32_t counts (MI_OBOX_COUNT), DEVICE memory.
 * mi_obox_offsets_device / mi_obox_fill_device: offsets, segments, the cut at capacity (NO record at an index >= capacity is ever
 *   written and none outside the segment), a decreasing pair = an empty segment, which is not walked, caller-made offsets (K i = the K
 *   smallest keys of every box, padded), overlapping segments (unspecified records inside them) and the form (a max-heap inside the
 *   segment, heap-sorted in place) are mi_box_offsets_device's and mi_box_fill_device's, with d_hits = `capacity` mi_overlap.
 * Host entries: the same on HOST buffers, synchronous, in batches of mi_scene_set_ray_batch oriented boxes; offsets and the `box` field
 *   are global across batches (`box` is the index modulo 2^32). The fill shares mi_list_fill's device staging.
 * Asynchrony, ordering against update / rebuild / set-geometry, destruction, groups, batches and stream rules: those of mi_box_*.
 * n == 0 is a no-op. MI_ERR_INVALID_ARG, before any device work and without reading the scene: a null scene or buffer, an unknown kind
 * ("unknown oriented-box kind"), oriented boxes or hits that are not 16-byte aligned, counts that are not 4-byte aligned, offsets that
 * are not 8-byte aligned, or more oriented boxes in one launch (host entries: in one batch) than the 32-bit work index allows
 * (0xFFBFFFFF).
 * Options: none apply (one kernel, one arithmetic). Counters: nothing is added to casts or paths; under full_stats the box tests are
 * added to "nodes visited" and the primitive tests to "leaf tests". */
typedef struct { float centre[3]; uint32_t reserved0; float half[3]; uint32_t reserved1; float quat[4]; } mi_obox;  /* 48 B, three 16-byte loads; quat = x, y, z, w */
enum { MI_OBOX_ANY = 0, MI_OBOX_COUNT = 1 };
int mi_obox_query_device(mi_scene* scene, int kind, const void* d_oboxes, void* d_out, size_t n, void* hip_stream);
int mi_obox_query(mi_scene* scene, int kind, const mi_obox* oboxes, void* out, size_t n);
int mi_obox_offsets_device(mi_scene* scene, const void* d_oboxes, uint64_t* d_offsets /* n + 1 */, size_t n, void* hip_stream);
int mi_obox_fill_device(mi_scene* scene, const void* d_oboxes, const uint64_t* d_offsets, mi_overlap* d_hits, size_t capacity, size_t n, void* hip_stream);
int mi_obox_offsets(mi_scene* scene, const mi_obox* oboxes, uint64_t* offsets /* n + 1 */, size_t n);
int mi_obox_fill(mi_scene* scene, const mi_obox* oboxes, const uint64_t* offsets, mi_overlap* hits, size_t capacity, size_t n);

/* Capsule queries: the primitives of the scene's CURRENT BVH within `radius` of each of n caller-supplied SEGMENTS [a, b] - a robot
 * link, a limb, a character's body (FCL's, Bullet's and PhysX's capsule, URDF's collision cylinder with rounded ends). A capsule is
 * also the volume a ball of that radius sweeps on a straight move from a to b: "does the ball hit anything on its way" is
 * MI_CAPSULE_ANY. a == b is a closed ball, radius == 0 a bare segment. Whether there is a primitive (MI_CAPSULE_ANY), how many
 * (MI_CAPSULE_COUNT), or which: two steps as for the box lists - the offsets of the capsules' segments, then the fill of a buffer
 * the caller sized from them.
 * Meaning: a primitive touches the capsule when the distance between the segment [a, b] and the primitive's SURFACE is at most
 * radius. Touching is CLOSED: contact counts. Queries see SURFACES, as everywhere in this library. `reserved` is not read. The record
 * is mi_overlap: the ids as mi_point_hit carries them, flags = 0 or MI_OVERLAP_CONTAINED, box = the index of the query the record
 * belongs to, reserved = 0. The empty record is {MI_INVALID_PRIM, MI_INVALID_GEOM, MI_FLAG_ESCAPED, box, 0}.
 * Arithmetic: binary32, one rounding per operation in the order written below, no contraction, correctly rounded divide and sqrt;
 * dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, cross(a, v) = (a.y v.z - a.z v.y, a.z v.x - a.x v.z, a.x v.y - a.y v.x),
 * dist2(p, q) = dot(p - q, p - q); sel_min(x, y) = x < y ? x : y, sel_max(x, y) = x > y ? x : y. Every rejection is a strict
 * compare that a NaN fails: a NaN never rejects, and a query so large that its products overflow errs towards listing. One
 * definition (ipu_ray_lib_amd/csrc/capsule_math.hpp, over point_math.hpp and box_math.hpp) serves the kernels and the host twins
 * (mi_scene_host.h), which return the same bytes.
 * Validity: a query is valid when all seven floats are finite and radius >= 0; -0 is legal. Any other query is not walked and finds
 *   nothing; so does an empty scene.
 * The query: d = b - a, r2 = radius radius, dd = dot(d, d); world bounds qmn_k = sel_min(a_k, b_k) - radius,
 *   qmx_k = sel_max(a_k, b_k) + radius; the lateral axes X0 = (0, d.z, -d.y), X1 = (-d.z, 0, d.x), X2 = (d.y, -d.x, 0) (cross(d, e_k)),
 *   R0 = width(d.z d.z + d.y d.y), R1 = width(d.z d.z + d.x d.x), R2 = width(d.y d.y + d.x d.x), Rd = width(dd), where
 *   width(ll) = ll >= 2^-126 ? radius sqrtf(ll) : +inf. 2^-126 is the smallest normal binary32: an axis whose squared length has
 *   underflowed (a == b, or a segment shorter than about 1e-19) separates nothing, since radius sqrtf(ll) would be 0, or short of its
 *   bits, while the products X_k dh_k below are not, and would part the ball from boxes that it reaches. Such a query is decided at
 *   the nodes by its world bounds, and errs towards listing like an overflowing one.
 * The bounds test capsule_meets_bounds(mn, mx), used at every node and, unchanged, as the first step at every leaf on the primitive's
 *   own bounds: first the six closed compares of mi_box_* against [qmn, qmx] (mn <= qmx && mx >= qmn on all axes). Then dl = mn - a,
 *   dh = mx - a. For each lateral axis X_i, over its two non-zero components k (lower index first): up = t + t' with
 *   t_k = X_k > 0 ? X_k dh_k : X_k dl_k; dn the same with dl and dh exchanged; the axis separates when dn > R_i || up < -R_i (relative
 *   to a the segment projects onto 0, the ball widens that to +-R_i). For the axis d: up = (t0 + t1) + t2 and dn likewise over the three
 *   components of d; it separates when dn > dd + Rd || up < -Rd. The bounds are met when the six compares hold and none of the four
 *   axes separates. The test has no other arithmetic. For radius == 0 these are the six axes of the complete segment-against-box
 *   separating-axis test; for a == b every width is +inf and the world bounds alone decide.
 * point_seg_dist2(p): t = dot(p - a, d); t <= 0: dist2(p, a); t >= dd: dist2(p, b); else dist2(p, a + d (t / dd)).
 * seg_seg_dist2(a, b, P, Q), Ericson, Real-Time Collision Detection 5.1.9 without its epsilon: d2 = Q - P, r = a - P, e = dot(d2, d2),
 *   f = dot(d2, r). dd <= 0 && e <= 0: dot(r, r). dd <= 0: s = 0, t = clamp(f / e). Else c = dot(d, r); e <= 0: t = 0,
 *   s = clamp(-c / dd). Else bb = dot(d, d2), denom = dd e - bb bb, s = denom != 0 ? clamp((bb f - c e) / denom) : 0,
 *   t = (bb s + f) / e; t < 0: t = 0, s = clamp(-c / dd); else t > 1: t = 1, s = clamp((bb - c) / dd). c1 = a + d s, c2 = P + d2 t,
 *   the result is dot(c1 - c2, c1 - c2). clamp(x) = x < 0 ? 0 : (x > 1 ? 1 : x): a NaN stays a NaN.
 * The walk is the stackless preorder walk of the box queries. A node is entered when capsule_meets_bounds of its box holds, else
 * passed. At a leaf so reached the primitive is tested; MI_CAPSULE_ANY stops at the first one that touches.
 * Primitive test. First capsule_meets_bounds on the primitive's OWN bounds - those mi_box_* defines for that kind of primitive. Then:
 *   Triangle (A, B, C) touches when any of these holds, tried in this order. 1, an end is near it: !(tri_point_dist2(A, B, C, a) > r2),
 *     then the same for b - the closest point of the triangle as mi_point_query finds it, q, and dist2(p, q). 2, the segment is near an
 *     edge: !(seg_seg_dist2(a, b, P, Q) > r2) for the edges AB, BC, CA in this order. 3, the segment pierces the face:
 *     n = cross(B - A, C - A), sa = dot(n, a - A), sb = dot(n, b - A), !(sa > 0 && sb > 0) && !(sa < 0 && sb < 0) && !(sa == 0 && sb == 0),
 *     and with u0 = A - a, u1 = B - a, u2 = C - a, w0 = dot(d, cross(u0, u1)), w1 = dot(d, cross(u1, u2)), w2 = dot(d, cross(u2, u0)): all
 *     three >= 0 or all three <= 0. A coplanar segment has w0 = w1 = w2 = 0; the both-in-plane exclusion keeps one far from the triangle
 *     from being listed, and coplanar pairs are decided by 1 and 2. MI_OVERLAP_CONTAINED: point_seg_dist2(V) <= r2 for all three
 *     vertices; the capsule is convex, so this is exact.
 *   Sphere (centre c, radius R): dmin2 = point_seg_dist2(c), dmax2 = sel_max(dist2(a, c), dist2(b, c)), s = R + radius, m = R - radius;
 *     it touches when !(dmin2 > s s) && !(m > 0 && dmax2 < m m): the shell is reached from outside and from inside; a capsule wholly
 *     inside the ball, away from the shell, touches nothing. CONTAINED: sqrtf(dmin2) + R <= radius.
 *   Disc (normal n as given, centre c, r2' the squared radius as the scene holds it, r' = sqrtf(r2')): CONSERVATIVE as everywhere - three
 *     necessary conditions. Its tight bounds pass the bounds test (the common first step); the segment reaches the plane's slab:
 *     sa = dot(n, a - c), sb = dot(n, b - c), rn = radius sqrtf(dot(n, n)), !(sa > rn && sb > rn) && !(sa < -rn && sb < -rn); the capsule
 *     reaches the ball: s = r' + radius, !(point_seg_dist2(c) > s s). No touching disc is missed, up to rounding; one whose rim the
 *     capsule passes may be listed although it is not touched. CONTAINED is the sufficient sqrtf(dmin2) + r' <= radius: never set
 *     wrongly, possibly absent for a thin disc.
 * Order: records are sorted by the key (geom_id, prim_id), ascending; keys are unique within a query. This IS the definition: a
 * segment shorter than the capsule's count holds the len smallest keys, and a list is the same bytes after a refit, a rebuild or
 * mi_scene_set_geometry of the same contents. The node test has arithmetic, so this needs an argument: fl(a - c), fl(x a) for a fixed
 * x and fl(a + b) are monotone in a and b, so for bounds A that contain bounds B every t_k of up is no smaller and every t_k of dn no
 * larger for A than for B, and so are the sums as computed: up(A) >= up(B), dn(A) <= dn(B) on each of the four axes; R_i, Rd and
 * dd + Rd do not depend on the bounds. Whatever B does not separate, A does not, and the six compares nest likewise. A node's device
 * box contains its primitives' bounds as those functions compute them - the fact the box family rests on -, so a primitive whose own
 * bounds pass has every ancestor's box pass, whatever tree is walked: what is listed is decided by the primitive and the query alone.
 * mi_capsule_query_device: d_capsules = n mi_capsule, d_out = n uint8_t, 1 = a primitive touches the capsule (MI_CAPSULE_ANY; the
 *   bytes need no alignment) or n uint32_t counts (MI_CAPSULE_COUNT), DEVICE memory.
 * mi_capsule_offsets_device / mi_capsule_fill_device: offsets, segments, the cut at capacity (NO record at an index >= capacity is ever
 *   written and none outside the segment), a decreasing pair = an empty segment, which is not walked, caller-made offsets (K i = the K
 *   smallest keys of every capsule, padded), overlapping segments (unspecified records inside them) and the form (a max-heap inside the
 *   segment, heap-sorted in place) are mi_box_offsets_device's and mi_box_fill_device's, with d_hits = `capacity` mi_overlap.
 * Host entries: the same on HOST buffers, synchronous, in batches of mi_scene_set_ray_batch capsules; offsets and the `box` field
 *   are global across batches (`box` is the index modulo 2^32). The fill shares mi_list_fill's device staging.
 * Asynchrony, ordering against update / rebuild / set-geometry / set-poses, destruction, groups, batches and stream rules: those of
 *   mi_box_*.
 * n == 0 is a no-op. MI_ERR_INVALID_ARG, before any device work and without reading the scene: a null scene or buffer, an unknown kind
 * ("unknown capsule kind"), capsules or hits that are not 16-byte aligned ("capsules must be 16-byte aligned"), counts that are not
 * 4-byte aligned, offsets that are not 8-byte aligned, or more capsules in one launch (host entries: in one batch) than the 32-bit work
 * index allows (0xFFBFFFFF).
 * Options: none apply (one kernel, one arithmetic). Counters: nothing is added to casts or paths; under full_stats the box tests are
 * added to "nodes visited" and the primitive tests to "leaf tests". */
typedef struct { float a[3]; float radius; float b[3]; uint32_t reserved; } mi_capsule;   /* 32 B, two 16-byte loads */
enum { MI_CAPSULE_ANY = 0, MI_CAPSULE_COUNT = 1 };
int mi_capsule_query_device(mi_scene* scene, int kind, const void* d_capsules, void* d_out, size_t n, void* hip_stream);
int mi_capsule_query(mi_scene* scene, int kind, const mi_capsule* capsules, void* out, size_t n);
int mi_capsule_offsets_device(mi_scene* scene, const void* d_capsules, uint64_t* d_offsets /* n + 1 */, size_t n, void* hip_stream);
int mi_capsule_fill_device(mi_scene* scene, const void* d_capsules, const uint64_t* d_offsets, mi_overlap* d_hits, size_t capacity, size_t n, void* hip_stream);
int mi_capsule_offsets(mi_scene* scene, const mi_capsule* capsules, uint64_t* offsets /* n + 1 */, size_t n);
int mi_capsule_fill(mi_scene* scene, const mi_capsule* capsules, const uint64_t* offsets, mi_overlap* hits, size_t capacity, size_t n);

/* Frustum queries: the primitives of the scene's CURRENT BVH inside or touching each of n caller-supplied REGIONS BOUNDED BY SIX
 * PLANES - a camera's view volume, a screen tile's sub-frustum (tiled or clustered light lists), a marquee selection, a shadow
 * cascade, a portal, a half-space, a slab. Whether there is a primitive (MI_FRUSTUM_ANY), how many (MI_FRUSTUM_COUNT), or which: two
 * steps as for the box lists - the offsets of the frusta's segments, then the fill of a buffer the caller sized from them.
 * Layout: mi_frustum is six planes nx, ny, nz, d: 96 bytes, six 16-byte loads, 16-byte aligned.
 * Region: a point p is in the region when n_k.p + d_k >= 0 for all six planes. Normals point INWARD and need not be unit; the
 *   region is whatever convex set the six half-spaces leave. The order of the planes means nothing.
 * Absent planes: a plane of four zeros is absent: it holds everywhere. This gives half-spaces, slabs, wedges and a frustum without
 *   a far plane; six absent planes list the whole scene.
 * Validity and emptiness: an item is valid when its 24 floats are finite. Any other item is not walked and finds nothing; so does
 *   an empty scene. A zero normal with d < 0 and contradictory planes are valid: the first lists nothing, the second no triangle -
 *   that falls out of the arithmetic below and is not a special case (a zero normal with d = -0 is an absent plane). A sphere or a
 *   disc wider than the gap between two contradictory planes is listed all the same: see their conservative test.
 * Meaning: a primitive is listed when its SURFACE and the region share a point. Touching is CLOSED: contact counts. The record is
 * mi_overlap: the ids as mi_point_hit carries them, flags = 0 or MI_OVERLAP_CONTAINED, box = the index of the query the record
 * belongs to, reserved = 0. The empty record is {MI_INVALID_PRIM, MI_INVALID_GEOM, MI_FLAG_ESCAPED, box, 0}.
 * Arithmetic: binary32, one rounding per operation in the order written below, no contraction, correctly rounded divide and sqrt;
 * dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z, cross(a, v) = (a.y v.z - a.z v.y, a.z v.x - a.x v.z, a.x v.y - a.y v.x),
 * at(k, p) = dot(n_k, p) + d_k, sel_min(x, y) = x < y ? x : y, sel_max(x, y) = x > y ? x : y. One definition
 * (ipu_ray_lib_amd/csrc/frustum_math.hpp, over box_math.hpp) serves the kernels and the host twins (mi_scene_host.h), which return
 * the same bytes.
 * The bounds test frustum_meets_bounds(mn, mx), used at every node and, unchanged, as the first step at every leaf on the primitive's
 *   own bounds, runs per plane on the corner of the bounds farthest along n: t_k = n_k > 0 ? n_k mx_k : n_k mn_k over the three axes,
 *   up = ((t0 + t1) + t2) + d; the plane separates when up < 0, and the bounds are met when no plane separates. A NaN separates
 *   nothing. The test has no other arithmetic: the region has no finite world bounds, so the planes are all there is. A box that
 *   misses the region only past one of its edges or corners is entered.
 * The walk is the stackless preorder walk of the box queries. A node is entered when frustum_meets_bounds of its box holds, else
 * passed. At a leaf so reached the primitive is tested; MI_FRUSTUM_ANY stops at the first one that touches.
 * Primitive test. First frustum_meets_bounds on the primitive's OWN bounds - those mi_box_* defines for that kind of primitive. Then:
 *   Triangle (A, B, C): EXACT, three stages tried in this order over s[v][k] = at(k, V_v), 18 values.
 *     1, a vertex in the region: some v has s[v][k] >= 0 for all k. MI_OVERLAP_CONTAINED when all three vertices have; the region is
 *     convex, so this is exact.
 *     2, an edge through the region: for AB, BC, CA in this order, [t0, t1] = [0, 1] is cut by the six planes in order from the
 *     values sP, sQ of the edge's two ends: both < 0, the edge misses; else sP < 0: t0 = sel_max(t0, sP / (sP - sQ)); else sQ < 0:
 *     t1 = sel_min(t1, sP / (sP - sQ)). The edge touches when it was not missed and t0 <= t1.
 *     3, the region through the face (the floor under the camera): no vertex lies in the region and no edge meets it, so the
 *     region's cross-section with the triangle's plane lies wholly inside the triangle or wholly outside; if not empty it is bounded
 *     and has a corner where two of the planes meet the triangle's plane. m = cross(B - A, C - A), mA = dot(m, A); for the 15 pairs
 *     i < j in order: c = cross(n_i, n_j), det = dot(c, m), the pair is skipped unless det != 0; u = cross(n_j, m), w = cross(m, n_i),
 *     x_a = (((-d_i) u_a - d_j w_a) + mA c_a) / det on each axis a; the triangle touches when at(k, x) >= 0 for the other four planes
 *     and dot(m, cross(B - A, x - A)) >= 0, dot(m, cross(C - B, x - B)) >= 0, dot(m, cross(A - C, x - C)) >= 0. A triangle with
 *     m = 0 (a segment, a point) ends at stage 2, which is exact for it.
 *   Sphere (centre c, radius R), CONSERVATIVE: with s = at(k, c), nn = dot(n_k, n_k), R2 = R R it is rejected only when some plane has
 *     the whole ball behind it: s < 0 && s s > R2 nn. CONTAINED: s >= 0 && s s >= R2 nn for all six planes (exact for the ball).
 *   Disc (normal n as given, centre c, r2 the squared radius as the scene holds it), CONSERVATIVE: its tight bounds pass the bounds
 *     test (the common first step), then the sphere's test on the ball (c, R2 = r2); CONTAINED likewise (sufficient, never wrong).
 *   Neither is ever missed, up to rounding. Each may be listed although it is not touched in two situations: it lies just outside
 *   an edge or a corner of the region - no single plane has all of it behind it -, or the region lies strictly inside a sphere,
 *   away from its shell.
 * Order: records are sorted by the key (geom_id, prim_id), ascending; keys are unique within a query. This IS the definition: a
 * segment shorter than the frustum's count holds the len smallest keys, and a list is the same bytes after a refit, a rebuild or
 * mi_scene_set_geometry of the same contents. The node test has arithmetic, so this needs an argument: fl(x a) for a fixed x and
 * fl(a + b) are monotone in a and b, so for bounds A that contain bounds B every t_k is no smaller for A than for B - n_k > 0 takes
 * mx_k, which is no smaller, any other n_k takes mn_k, which is no larger, times a factor that is not positive -, and so is up as
 * computed. Whatever plane does not separate B does not separate A. A node's device box contains its primitives' bounds as those
 * functions compute them - the fact the box family rests on -, so a primitive whose own bounds pass has every ancestor's box pass,
 * whatever tree is walked: what is listed is decided by the primitive and the query alone.
 * mi_frustum_query_device: d_frusta = n mi_frustum, d_out = n uint8_t, 1 = a primitive touches the region (MI_FRUSTUM_ANY; the
 *   bytes need no alignment) or n uint32_t counts (MI_FRUSTUM_COUNT), DEVICE memory.
 * mi_frustum_offsets_device / mi_frustum_fill_device: offsets, segments, the cut at capacity (NO record at an index >= capacity is ever
 *   written and none outside the segment), a decreasing pair = an empty segment, which is not walked, caller-made offsets (K i = the K
 *   smallest keys of every frustum, padded), overlapping segments (unspecified records inside them) and the form (a max-heap inside the
 *   segment, heap-sorted in place) are mi_box_offsets_device's and mi_box_fill_device's, with d_hits = `capacity` mi_overlap.
 * Host entries: the same on HOST buffers, synchronous, in batches of mi_scene_set_ray_batch frusta; offsets and the `box` field
 *   are global across batches (`box` is the index modulo 2^32). The fill shares mi_list_fill's device staging.
 * Asynchrony, ordering against update / rebuild / set-geometry / set-poses, destruction, groups, batches and stream rules: those of
 *   mi_box_*.
 * n == 0 is a no-op. MI_ERR_INVALID_ARG, before any device work and without reading the scene: a null scene or buffer, an unknown kind
 * ("unknown frustum kind"), frusta or hits that are not 16-byte aligned ("frusta must be 16-byte aligned"), counts that are not
 * 4-byte aligned, offsets that are not 8-byte aligned, or more frusta in one launch (host entries: in one batch) than the 32-bit work
 * index allows (0xFFBFFFFF).
 * Options: none apply (one kernel, one arithmetic). Counters: nothing is added to casts or paths; under full_stats the box tests are
 * added to "nodes visited" and the primitive tests to "leaf tests". */
typedef struct { float planes[6][4]; } mi_frustum;   /* 96 B, six 16-byte loads: nx, ny, nz, d per plane */
enum { MI_FRUSTUM_ANY = 0, MI_FRUSTUM_COUNT = 1 };
int mi_frustum_query_device(mi_scene* scene, int kind, const void* d_frusta, void* d_out, size_t n, void* hip_stream);
int mi_frustum_query(mi_scene* scene, int kind, const mi_frustum* frusta, void* out, size_t n);
int mi_frustum_offsets_device(mi_scene* scene, const void* d_frusta, uint64_t* d_offsets /* n + 1 */, size_t n, void* hip_stream);
int mi_frustum_fill_device(mi_scene* scene, const void* d_frusta, const uint64_t* d_offsets, mi_overlap* d_hits, size_t capacity, size_t n, void* hip_stream);
int mi_frustum_offsets(mi_scene* scene, const mi_frustum* frusta, uint64_t* offsets /* n + 1 */, size_t n);
int mi_frustum_fill(mi_scene* scene, const mi_frustum* frusta, const uint64_t* offsets, mi_overlap* hits, size_t capacity, size_t n);

/* Geometry updates: new positions for the primitives of a live scene, the topology kept - triangles, geometry list, materials and
 * the BVH's shape - and every BVH box recomputed on the device (a refit: Embree's RTC_BUILD_QUALITY_REFIT commit, OptiX's
 * OPTIX_BUILD_OPERATION_UPDATE). Any pointer may be NULL = keep; a non-NULL array must have exactly the scene's count (a NULL array
 * must come with count 0). mesh_normals only for scenes created with normals.
 * Result. The nodes are those mi_refit_compact_bvh (mi_scene_host.h) computes from the moved arrays, byte for byte, and every render
 * and query afterwards equals that of a scene freshly created from the moved arrays and those nodes, bit for bit. A refit keeps the
 * old topology, so under large motion boxes overlap more and traces slow down; mi_scene_rebuild (below) gives the scene a new one.
 * Ordering. The update waits for all work already enqueued on the scene, on any stream (renders and queries), before it overwrites a
 * device record: a render or query enqueued before the update sees the old geometry, whatever its stream.
 * Synchronous return. The update returns once the new geometry is in place; work enqueued after it returns sees it. It reads back
 * one small record (the refusal flag and the root box). mi_scene_update_device takes DEVICE arrays and does its kernels and copies on
 * hip_stream (a hipStream_t as void*; NULL = the null stream), then waits for that stream only; mi_scene_update takes HOST arrays.
 * Refusal. MI_ERR_INVALID_ARG leaves the scene unchanged - every record, node and later result: a null scene or update, a count
 * that differs from the scene's (or a count without its array), normals for a scene without normals, a resulting node box that
 * is not finite, an extent above 65504 - exactly when mi_scene_create from the moved arrays and the refit nodes would fail.
 * Counters, options and the NIF environment are untouched; a scene made by mi_scene_create_from_blob updates the same way.
 * The first update builds the refit's device tables (about 100 bytes per node); a scene never updated allocates nothing for them.
 * mi_scene_get_bvh copies the scene's current compact nodes to `out` (HOST memory, capacity nodes); *num_nodes = the node count
 * (out == NULL: only the count). */
typedef struct {
  const mi_vec3*   mesh_verts;   uint32_t num_verts;
  const mi_vec3*   mesh_normals; uint32_t num_normals;   /* only for scenes created with normals */
  const mi_sphere* spheres;      uint32_t num_spheres;
  const mi_disc*   discs;        uint32_t num_discs;
} mi_geometry_update;

int mi_scene_update(mi_scene* scene, const mi_geometry_update* host_arrays);                            /* host memory */
int mi_scene_update_device(mi_scene* scene, const mi_geometry_update* device_arrays, void* hip_stream); /* device memory */
int mi_scene_get_bvh(mi_scene* scene, mi_bvh_node* out, uint32_t capacity, uint32_t* num_nodes);       /* current compact nodes, host out */
/* Measurement only (tools/bench_refit.py): the last update's pass times in milliseconds from HIP events on its stream,
 * out = {leaf boxes, interior boxes, record rewrite and copies}; zeros unless scene option "refit_timing" is 1. */
int mi_get_refit_timing(mi_scene* scene, double out[3]);

/* Rigid poses: move whole geometries of a live scene by one transform each - a rotation (a quaternion that need not be unit), a
 * uniform scale and a translation - and refit (Embree's and OptiX's per-instance transform; this library has one BVH over all
 * primitives, so the geometry is posed on the device and the BVH refitted: every later render and query works unchanged on the posed
 * scene). 32 bytes per geometry cross the bus, not 12 per vertex.
 * Poses and the geometry list. One pose per entry of the scene's geometry list, in its order; num_geometry must equal the scene's
 * geometry count.
 * Rest geometry. Poses are ABSOLUTE: each is applied to the rest geometry, never to the previous pose's result - "pose A, then pose
 * B" gives the bytes of "pose B" alone, nothing drifts. The rest geometry is the scene's current geometry - vertices, vertex normals,
 * spheres, discs - at the first pose call after mi_scene_create*, mi_scene_update*, mi_scene_set_geometry* or mi_scene_bake_poses:
 * those calls invalidate the snapshot and reset the stored poses to the identity. A rebuild, an automatic one included, changes
 * topology only and keeps both. A scene that is never posed allocates nothing (a posed one keeps a rest copy, a scratch copy and a
 * uint16_t owner per vertex: 26 bytes per vertex, 50 with normals).
 * Arithmetic. Binary32, one rounding per operation, nothing contracted. U, V, W = obox_frame(x, y, z, w), the function mi_obox uses
 * (ipu_ray_lib_amd/csrc/obox_math.hpp): qq = ((x x + y y) + z z) + w w, s = 2 / qq, xs = x s, ys = y s, zs = z s,
 * U = (1 - (y ys + z zs), x ys + w zs, x zs - w ys), V = (x ys - w zs, 1 - (x xs + z zs), y zs + w xs),
 * W = (x zs + w ys, y zs - w xs, 1 - (x xs + y ys)) - the columns of the rotation's matrix, so a body and its mi_obox turn alike.
 * A point p becomes p'_k = fl(fl(scale r_k) + t_k) with r_k = fl(fl(fl(U_k p.x) + fl(V_k p.y)) + fl(W_k p.z)); a direction becomes
 * r_k: no scale, no translation, not renormalised.
 * What is moved. Mesh vertices are points, vertex normals directions; a sphere's centre is a point and radius' = fl(scale radius); a
 * disc's centre is a point, its normal a direction and r' = fl(scale r).
 * Identity. A pose is the identity when it compares equal to (0, 0, 0, 1; 0, 0, 0; 1) - float compares, -0 counts as zero. Such a
 * pose copies the geometry's rest bytes: a -0 coordinate stays -0.
 * Valid pose. Eight finite floats, qq > 0, a finite 2 / qq (mi_obox's rule) and scale > 0.
 * Ownership. A vertex belongs to the geometry whose mesh's range [first_vertex, first_vertex + num_vertices) contains it; vertices in
 * no referenced mesh's range, and spheres and discs no geometry references, keep their rest bytes. The call is refused when two
 * meshes' vertex ranges intersect or when one mesh, sphere or disc is referenced by two geometry entries (the message names the
 * pair); checked once per rest snapshot, on the host.
 * Result. mi_pose_geometry_host (mi_scene_host.h) computes the posed arrays; after the call the scene is, bit for bit, what
 * mi_scene_update with those arrays leaves: nodes, records, later renders and queries, "auto_rebuild" decisions and the counts of
 * mi_get_live_stats.
 * Ordering. The call waits for all work already enqueued on the scene, on any stream (renders and queries), before it overwrites a
 * device record: a render or query enqueued before it sees the old geometry, whatever its stream.
 * Synchronous return. The call returns once the new geometry is in place; work enqueued after it returns sees it. It reads back one
 * small record more than an update does (whether every pose is valid). mi_scene_set_poses_device takes DEVICE poses (16-byte aligned)
 * and does its kernels and copies on hip_stream (a hipStream_t as void*; NULL = the null stream), then waits for that stream only;
 * mi_scene_set_poses takes HOST poses.
 * Refusal. MI_ERR_INVALID_ARG leaves the scene unchanged - the scene, the stored poses and the rest snapshot: a null scene or a null
 * array, a wrong num_geometry, an invalid pose (for the device entry decided on the device, before anything changes), an ownership
 * conflict, a resulting node box that is not finite, an extent above 65504. The message names the entry.
 * Zero geometries. num_geometry == 0 on a scene of zero geometries is a no-op that reads no pointer.
 * mi_scene_get_poses copies the current poses to `out` (HOST memory, capacity poses); *num_geometry = the geometry count (out == NULL:
 * only the count). mi_scene_bake_poses: the current geometry becomes the rest geometry and every pose the identity; it moves no byte
 * of the scene. */
typedef struct { float quat[4]; float translation[3]; float scale; } mi_pose;   /* 32 B, two 16-byte loads; quat = x, y, z, w */

int mi_scene_set_poses(mi_scene* scene, const mi_pose* poses, uint32_t num_geometry);                                  /* host memory */
int mi_scene_set_poses_device(mi_scene* scene, const void* d_poses, uint32_t num_geometry, void* hip_stream);          /* device memory */
int mi_scene_get_poses(mi_scene* scene, mi_pose* out, uint32_t capacity, uint32_t* num_geometry);                      /* current poses, host out */
int mi_scene_bake_poses(mi_scene* scene);
/* Measurement only (tools/bench_pose.py): the last pose call's times in milliseconds from HIP events on its stream, out = {the
 * pose pass (frames and posed arrays), everything after it (the read-back, the refit, the copies)}; zeros unless scene option
 * "refit_timing" is 1. */
int mi_get_pose_timing(mi_scene* scene, double out[2]);

/* Rebuild the BVH topology of a live scene from its CURRENT geometry, on the device (Embree's RTC_BUILD_QUALITY_LOW rebuild next
 * to its refit, OptiX's BUILD next to UPDATE): a linear BVH - Morton keys of the primitive centroids, a radix sort, Karras' 2012
 * hierarchy - over the primitives in canonical order (geometry 0 .. G - 1, inside a mesh triangle 0 .. T - 1). The node count
 * stays 2 P - 1 (one primitive per leaf); everything attached to the scene stays: NIF weights, options, counters, launch slots.
 * Result. The nodes are those mi_build_lbvh_compact (mi_scene_host.h) computes from the scene's current arrays, byte for byte,
 * whatever topology or history the scene had (rebuilding twice is the identity); *max_leaf_depth (may be NULL) is the twin's depth;
 * every render and query afterwards equals that of a scene freshly created from the current arrays and those nodes, bit for bit.
 * An LBVH costs more box tests per cast than the host builder's tree: the rebuild is for a scene whose refitted
 * tree has degraded, not a better tree for a static one.
 * Ordering. The rebuild waits for all work already enqueued on the scene, on any stream (renders and queries), before it overwrites
 * a device record: a render or query enqueued before the rebuild sees the old tree, whatever its stream.
 * Synchronous return. The rebuild returns once the new tree is in place; work enqueued after it returns sees it. It reads back two
 * small records (where the tree's depths start; the refusal flag and the root box). Its kernels run on hip_stream (a hipStream_t as
 * void*; NULL = the null stream), and it waits for that stream only.
 * Refusal. MI_ERR_INVALID_ARG leaves the scene unchanged - every record, node and later result: a null scene, a scene whose BVH does
 * not hold every primitive in exactly one leaf, a resulting node box that is not finite, an extent above 65504 - exactly when
 * mi_scene_create from the current arrays and the twin's nodes would fail. (Geometry that came in through mi_scene_update* has
 * passed the same checks; a scene created with nodes that do not bound its geometry can be refused.)
 * A scene of 0 nodes is a no-op (depth 0), one primitive keeps its single leaf root (depth 1). Counters, options and the NIF
 * environment are untouched; a scene made by mi_scene_create_from_blob rebuilds the same way. mi_scene_get_bvh returns the rebuilt
 * nodes. The first rebuild builds the canonical primitive table and the passes' scratch (about 135 bytes per primitive, plus the
 * update's tables); a scene never rebuilt allocates nothing for them. The rebuild leaves the refit's tables of the new topology
 * ready on the device (what every node's box is computed from, the nodes bucketed by height, where the heights start: device passes
 * of the rebuild, read back with its second record): the first mi_scene_update* after a rebuild costs what any other does. Only a
 * scene's very first update derives its tables on the host, from the nodes the scene was created with; a scene whose first call is
 * a rebuild never does (mi_get_live_stats counts the derivations). */
int mi_scene_rebuild(mi_scene* scene, void* hip_stream, uint32_t* max_leaf_depth /* may be NULL */);
/* Measurement only (tools/bench_rebuild.py): the last rebuild's pass times in milliseconds from HIP events on its stream, out =
 * {primitive boxes + scene box + keys, key sort, hierarchy + depths + depth sort (with the first read-back), level boxes,
 * preorder indices, refit tables (height sort, height starts, with the second read-back) + scatter + copies}; zeros unless scene
 * option "rebuild_timing" is 1. */
int mi_get_rebuild_timing(mi_scene* scene, double out[6]);

/* Replace the CONTENTS of a live scene: new geometry list, meshes, triangle lists, vertices, normals, spheres, discs, material ids
 * and materials - every count may differ from the scene's, vertex normals may appear or disappear - and its BVH built on the device
 * (Embree's rtcCommitScene after attaching or detaching geometry, an OptiX BUILD into a live pipeline). The scene stays: the render
 * parameters of its desc (image, fov, spp, seed, window, path length), the NIF environment, every option, the counters (they go
 * on counting), the launch slots and their scratch, its place in a group. An empty scene (mi_scene_create with no geometry and no
 * nodes) that takes this call is a scene made without a host-built BVH.
 * Arrays. The control plane - geometry, mesh_info, mat_ids, materials - is always HOST memory. The data plane - mesh_tris,
 * mesh_verts, mesh_normals, spheres, discs - is HOST memory for mi_scene_set_geometry and DEVICE memory for
 * mi_scene_set_geometry_device. All of them are copied: they may be freed when the call returns.
 * Result. The scene's contents are exactly the given arrays and its BVH is their LBVH: mi_scene_get_bvh returns what
 * mi_build_lbvh_compact (mi_scene_host.h) computes from the same arrays, byte for byte; *max_leaf_depth (may be NULL) is the twin's
 * depth; every render and query afterwards equals that of a scene freshly created from the arrays and the twin's nodes, bit for
 * bit. No primitives: an empty scene (0 nodes, depth 0). One primitive: a single leaf root (depth 1).
 * How. The new contents are built aside and swapped in: new geometry buffers, device records and refit tables are allocated, the
 * canonical primitive table is written by a kernel (one thread per primitive, a binary search over the geometries' prefix sums),
 * the passes of mi_scene_rebuild run into the new buffers, the decision is read back, and only then the scene's pointers are
 * swapped and the old buffers freed. The rebuild's scratch is reused where it is large enough. Peak device memory is the old scene
 * plus the new one plus the scratch (about 135 bytes per primitive).
 * Ordering and return. Work enqueued on the scene before the call, on any stream, sees the old contents. The call returns once
 * the new contents are in place. Its kernels and copies run on hip_stream (a hipStream_t as void*; NULL = the null stream;
 * mi_scene_set_geometry uses the null stream) and it waits for that stream only - and, before it frees anything old, for the
 * work the scene had enqueued before (the launch slots' events).
 * Refusal. MI_ERR_INVALID_ARG leaves the scene unchanged - every record, node and later result. Refused is exactly what
 * mi_scene_create from the same arrays and the twin's nodes would refuse, with its words where the check is the same one: a null
 * array that comes with a count, a geometry type, geometry index, material index or mesh range out of bounds, normals neither
 * absent nor one per vertex, more than 65535 geometries, more than 2^25 primitives, a triangle's vertex index not below its mesh's
 * num_vertices, a node box that is not finite, an extent above 65504. The last three are found on the device (the error word
 * the passes share); the others on the host before any device work. A null scene or struct is refused before a device is touched.
 * Afterwards the scene is in the state of one just rebuilt: the refit's tables are device-made and ready (no host derivation, the
 * first mi_scene_update* costs what any other does, and its count checks use the new counts), mi_scene_rebuild is the identity,
 * mi_get_live_stats counts the call and carries the new depth, and option "auto_rebuild" takes the new tree's estimate as its
 * baseline (off: the baseline is dropped, a later enable measures the new tree). */
typedef struct {
  /* control plane: always HOST memory (at most 65535 geometries) */
  const mi_geom_ref*  geometry;   uint32_t num_geometry;
  const mi_mesh_info* mesh_info;  uint32_t num_meshes;
  const uint32_t*     mat_ids;    uint32_t num_mat_ids;
  const mi_material*  materials;  uint32_t num_materials;
  /* data plane: HOST memory for mi_scene_set_geometry, DEVICE memory for mi_scene_set_geometry_device */
  const uint16_t*  mesh_tris;    uint32_t num_tris;
  const mi_vec3*   mesh_verts;   uint32_t num_verts;
  const mi_vec3*   mesh_normals; uint32_t num_normals;   /* 0, or == num_verts */
  const mi_sphere* spheres;      uint32_t num_spheres;
  const mi_disc*   discs;        uint32_t num_discs;
} mi_scene_geometry;

int mi_scene_set_geometry(mi_scene* scene, const mi_scene_geometry* host_arrays, uint32_t* max_leaf_depth /* may be NULL */);
int mi_scene_set_geometry_device(mi_scene* scene, const mi_scene_geometry* arrays, void* hip_stream, uint32_t* max_leaf_depth /* may be NULL */);

/* The surface-area cost of the scene's CURRENT BVH - the nodes mi_scene_get_bvh would return -, summed on the device: the figure a
 * caller (and option "auto_rebuild") decides between refit and rebuild by. out = {sum_all, sum_leaf, a_root}: a node's term is
 * a = (ex * ey + ey * ez) + ez * ex in binary64 from its three binary16 extents; sum_all sums it over all nodes (every visited node
 * costs a box test, leaves included), sum_leaf over the leaves (a primitive test each), a_root is the root's term. sum_all / a_root
 * is the expected number of box tests of a random line through the root box, sum_leaf / a_root that of primitive tests. The raw
 * sums come back and the caller divides: an empty scene gives zeros, and a_root == 0 (a root box without area) is legal.
 * Bit-reproducible: the sums are formed in a fixed shape (blocks of 256 consecutive nodes through a fixed binary tree, then the
 * partial sums the same way, level by level; no atomics), so the result is the same run to run and on every replica of a group, and
 * equals the host twin mi_bvh_cost_compact (mi_scene_host.h) of the same nodes bit for bit.
 * Its kernels run on hip_stream (a hipStream_t as void*; NULL = the null stream) and it waits for that stream only; one read-back of
 * 32 bytes. It changes nothing of the scene, the counters included. A scene that was never updated or rebuilt still has its nodes on
 * the host only: the twin then runs there (the same bits) and nothing is allocated. MI_ERR_INVALID_ARG: a null scene or out. */
int mi_scene_bvh_cost(mi_scene* scene, void* hip_stream, double out[3]);

/* What updates and rebuilds have done to this scene so far: out = {updates applied, updates refused for their geometry (a node box
 * not finite or too large; argument errors are not counted), explicit rebuilds (mi_scene_rebuild calls that succeeded), automatic
 * rebuilds (option "auto_rebuild"), host derivations of the refit's tables (1 after the first update of a scene that was not rebuilt
 * before or given new contents, else 0: never more), cost evaluations (mi_scene_bvh_cost calls and the policy's own), the current
 * max_leaf_depth (the scene's at create, the rebuilt or newly built tree's afterwards), mi_scene_set_geometry* calls that
 * succeeded}. Touches no device. */
int mi_get_live_stats(mi_scene* scene, uint64_t out[8]);

/* Replaces: IpuScene::getTraceTimeSecs (IpuScene.hpp:55). Wall time of the last mi_render. */
double mi_trace_time_secs(const mi_scene* scene);

/* Counters accumulated by render calls since scene creation / last reset: number of
 * CompactBvh::intersect + ::occluded casts, BVH nodes visited, primitive (leaf) tests.
 * Synchronises the device. counts[0]=casts, [1]=nodes visited, [2]=leaf tests, [3]=paths. */
int mi_get_counters(mi_scene* scene, uint64_t counts[4]);
int mi_reset_counters(mi_scene* scene);

/* Diagnostics of the phase-scheduled path-trace kernel (only filled when the instrumented kernel
 * variant is selected with MI_RAYLIB_FULL_STATS=1): for each phase NODE, LEAF, SHADE, GEN the number
 * of wave-level executions and the sum of lanes active in them:
 * stats[0..7] = {node_iters, node_lanes, leaf_iters, leaf_lanes, shade_iters, shade_lanes, gen_iters, gen_lanes},
 * stats[8..11] = shader cycles summed over waves spent in {traversal loop, SHADE, GEN, whole kernel loop}.
 * No reference counterpart (the IPU has no SIMT lanes); used by DESIGN.md's occupancy table. */
int mi_get_phase_stats(mi_scene* scene, uint64_t stats[12]);
/* Scheduler bookkeeping of the path-pool kernel (kernel 3, instrumented build only): {loop iterations, refill turns,
 * lanes refilled, idle iterations, lost ring claims, traversal bursts, lanes walking at burst start, cycles in refill}. */
int mi_get_pool_stats(mi_scene* scene, uint64_t stats[8]);
/* What the instrumented build (option full_stats) counted of plain renders that walked the private, hot-first copy (option hot_nodes):
 * {box-test steps that ran from LDS, the lanes in them, box-test steps of runs that ran from global memory, the lanes in them, box tests
 * of nodes inside the staged prefix}. Zeros while no such render has run. */
int mi_get_hot_stats(mi_scene* scene, uint64_t stats[5]);
/* Measurement only: enqueues, on a stream of the scene's own, ONE wave that samples the work counter of `hip_stream`'s persistent
 * launches n times, period_ticks (100-MHz ticks) apart, into d_samples (device memory, 2 n words: {s_memrealtime, counter}). Call it
 * right before mi_render_device on `hip_stream`; read the samples after a device synchronise (tools/launch_progress.py: the rate at which
 * a launch hands its work units out over its life). No reference counterpart. */
int mi_debug_launch_progress(mi_scene* scene, void* hip_stream, uint64_t* d_samples, uint32_t n, uint32_t period_ticks);
/* Diagnostics of NIF renders (only filled while the scene option "nif_timing" is 1): HIP events bracket every launch of
 * the MLP kernel on the render's stream. out[0] = milliseconds spent in MLP launches since the last call, out[1] = number
 * of launches. Synchronises the device and clears the record. tools/bench_config5.py reports the MLP's share of a frame
 * from it. No reference counterpart. */
int mi_get_nif_timing(mi_scene* scene, double out[2]);
/* The shader clock the last launch of the register-resident MLP kernel (K3a, csrc/nif_asm_kernel.hpp) ran at: out[0] = shader
 * cycles (s_memtime), out[1] = ticks of the constant 100-MHz counter (s_memrealtime) that the first wave of its first workgroup -
 * which lives as long as the launch - spent in the kernel; clock in GHz = out[0] / out[1] / 10. Both 0 when the scene's network
 * runs nif_mlp_kernel (no such record). Synchronises the device. An MFMA-dense kernel runs at the clock the chip's power
 * management leaves it, which differs from box to box: bench.py quotes this beside the kernel's time. No reference counterpart. */
int mi_get_nif_clock(mi_scene* scene, uint64_t out[2]);

/* Replaces: IpuScene::loadNifModel (src/IpuScene.cpp:174-187) with the weights handed over as
 * arrays (the file side — nif_metadata.txt + Keras-H5 — is mi_host_nif_load in mi_scene_host.h).
 * Dense layer i has kernel[i] of shape [rows[i] x cols[i]] row-major (Keras kernel:0 layout,
 * y = x·W + b) and bias[i] of cols[i] floats (NULL = no bias); relu[i] != 0 applies ReLU.
 * Where a layer's rows != current activation width, the Fourier features are re-concatenated
 * to the activations first (NifModel.cpp:306-309). Decode: y*max + mean, then exp if
 * log_tonemap (NifModel.cpp:222-246); `mean` must already have eps folded in
 * (NifMetaData.cpp:48-53). Output channels are BGR (codelets/TraceCodelets.cpp:376). */
int mi_scene_set_nif(mi_scene* scene, uint32_t num_layers,
                     const float* const* kernels, const float* const* biases,
                     const uint32_t* rows, const uint32_t* cols, const uint8_t* relu,
                     uint32_t embedding_dimension, float max_value, const float mean[3],
                     int32_t log_tonemap);

/* Replaces: IpuScene::setHdriRotation (degrees) / setMaxNifBatchSize (src/IpuScene.cpp:334-344). */
int mi_scene_set_hdri_rotation(mi_scene* scene, float degrees);
int mi_scene_set_max_nif_batch(mi_scene* scene, size_t rays_per_batch);

/* Replaces: the `raysPerWorker` constructor argument / --rays-per-worker (src/IpuScene.cpp:360-361, 110-172):
 * mi_render cuts the host ray stream into batches of this many rays (the reference: 1440 tiles x 6 workers x
 * raysPerWorker), pipelines their upload / trace / download on two HIP streams and calls the ray callback once
 * per finished batch, in batch order. 0 (default) = one batch. Results do not depend on the batch size. */
int mi_scene_set_ray_batch(mi_scene* scene, size_t rays_per_batch);

/* Kernel selection / tuning of ONE scene (no reference counterpart; the nearest is the reference's per-run
 * RuntimeConfig + codelet build flags, trace.cpp:297-309). Every scene carries its own copy: defaults, overridden
 * by the MI_RAYLIB_* environment variables as they stand when the scene is created, then by this call. Keys and the
 * values each accepts (anything else: MI_ERR_INVALID_ARG, the option keeps its value):
 *   "kernel"        0 | 1 | 2 | 3   nested-loop / phase-scheduled (default) / phase-scheduled + LDS-staged nodes / path pool
 *   "waves"         4 | 5 | 6 | 7   waves per SIMD the default kernel is built for (6: the 80-VGPR build, the default; 5 - the 96-VGPR build -,
 *                                   4 and 7 - 72 VGPRs, 21 words of LDS per lane, measured 1 % slower - only in the variants build)
 *   "merge"         0 | 1           kernel 1: SHADE and GEN served by one turn (1, the default) or by two, at five waves per SIMD - the
 *                                   default kernel up to round 3 (0: variants build only)
 *   "spec"          0 | 1           kernel 1: lanes walk on past ONE pending primitive test
 *   "full_stats"    0 | 1           instrumented kernels: node / leaf-test counters, phase occupancy
 *   "tune"          "leafAt,shadeAt,genAt[,burst,keep8,dbl,maxExtra(<=7),leafThenNode,prio,leafP,probe]"   scheduling weights of kernel 1
 *   "pool_waves"    4 | 8 | 16      kernel 3: waves per workgroup
 *   "pool_tune"     "leafAt,burst,retireAt,refillMin,shadeW,genW[,dbl,maxExtra,leafThenNode,prio]"
 *   "tiles"         0 | 1           walk row-structured streams in 8x8 pixel tiles
 *   "seg_budget_kb" N >= 1          partial-sum buffer budget per launch
 *   "nif_spl"       0..1024         NIF samples per launch, rounded up to whole segments (0 = default: 512, memory permitting - 48 B of
 *                                   slots per sample and pixel; a launch is never shorter than its longest work unit: 128 samples per launch cost
 *                                   config 5 5 % of its frame)
 *   "nif_shape"     auto | a8 | b4 | w6 | t6 | t4    which NIF MLP kernel runs (b4 = K3a's dataflow with four waves of 64 rays: 3 % slower): auto (default) = a8 where its generated body covers the network
 *                                   (the reference's 6 x 320 shape), w6 otherwise; a8 = K3a, the hand-scheduled register-resident kernel
 *                                   (csrc/nif_asm_kernel.hpp); w6 | t6 | t4 = workgroup shapes of nif_mlp_kernel; the variants build also takes
 *                                   r8 | r8s = K3r (csrc/nif_regs_kernel.hpp: measured slower; refused by the shipped library)
 *   "nif_generations" 1..4096       nif_mlp_kernel: workgroups launched per resident slot (measurement knob; default 64)
 *   "root_start"    0 | 1           a cast whose origin lies strictly inside the root's box starts at node 1 (default 1; exact either way)
 *   "say_grid"      0 | 1           print every persistent launch's grid to stderr
 *   "pin"           0 | 1           page-lock the caller's stream for the duration of mi_render
 *   "nif_overlap"   auto | 0 | 1    NIF renders trace sample batch b + 1 beside the MLP of batch b (two slot sets, a second stream). auto (the
 *                                   default) = only beside nif_mlp_kernel: K3a / K3b hold every register of their compute unit, nothing runs
 *                                   beside them, and one slot set leaves the memory for longer launches
 *   "nif_split"     0..1024         with the overlap: compute units the trace launches of batches 1.. get for themselves (two CU-masked
 *                                   streams, hipExtStreamCreateWithCUMask; the MLP and accumulate passes keep the rest). 0 = off, the default:
 *                                   the MLP is power-limited and loses as much as the hidden launch was worth (-2 ... +5 % by box)
 *   "nif_first_test" 0 | 1          NIF renders: a cast's first box test runs in the turn that sets the cast up instead of in a NODE turn
 *                                   (default 0: measured neutral)
 *   "nif_trace_wgs" 0..16           with nif_overlap: workgroups per compute unit of a trace launch that runs beside the previous batch's MLP
 *                                   (0 = all that stay resident, the default)
 *   "nif_timing"    0 | 1           bracket every MLP launch of a NIF render with HIP events (mi_get_nif_timing)
 *   "refit_timing"  0 | 1           bracket the passes of mi_scene_update* with HIP events (mi_get_refit_timing)
 *   "rebuild_timing" 0 | 1          bracket the passes of mi_scene_rebuild with HIP events (mi_get_rebuild_timing)
 *   "leaf_rot"      0 | 1           scenes without vertex normals: the default kernel reads primitive records pre-rotated for the cast's shear axis (default 1)
 *   "lean_hit"      0 | 1           scenes without vertex normals run the build of the default kernel that carries no barycentrics (default 1)
 *   "leaf_frame"    0 | 1           scenes without vertex normals: the default kernel loads the tangent frame of a diffuse bounce off a triangle or disc from a
 *                                   per-leaf record instead of computing it per hit (default 1; every byte the same either way)
 *   "hot_nodes"     auto | 0..65535 plain renders of the default kernel walk a private, hot-first copy of the BVH arrays and run the box-test runs whose lanes
 *                                   all stand in its first nodes from LDS: that many nodes, clamped to the tree and to what fits beside the kernel's other LDS
 *                                   (316 on an MI355X). 0 = off: the shared arrays and the launch of before. auto (the default): on, with as many as fit, where
 *                                   those nodes take 0.9 of the tree's expected box tests (surface-area model, decided at create). Every result byte is the same
 *                                   either way. NIF renders, renders under double_fallback or fast, and a scene whose geometry has been updated, rebuilt
 *                                   or replaced (mi_scene_update*, mi_scene_rebuild, mi_scene_set_geometry*) run on the shared arrays whatever the option says.
 *                                   The un-instrumented builds walk a copy from which the interior nodes whose box test cannot change a result have been
 *                                   taken (both children's stored boxes inside the node's own, and the node more than half its nearest surviving ancestor's
 *                                   half-area: csrc/hot_order.hpp), casts on the literal box test (a zero or denormal direction component, a non-finite
 *                                   origin) start in a region of every node behind it; the instrumented build (full_stats) walks a copy of every node and
 *                                   counts the reference's visits.
 *                                   The copies are made at create, whatever the option says then (it may be set later): about 750 bytes of device memory per
 *                                   BVH node beside the shared arrays' own, given back by the first update, rebuild or replacement of the geometry
 *   "coords"        0 | 1           (pixel, segment) work units read the pixel's (u, v) from a compact copy of the stream gathered once
 *                                   per launch, not from the 84-byte record (default 1: a third of the HBM traffic)
 *   "cus"           0..4096         compute units the launch grids are sized for (0 = what the device reports; grids are
 *                                   units x workgroups resident per unit, asked of the runtime per kernel)
 *   "query_kernel"  0 | 1           ray queries (mi_query*): one thread per ray (0, the default: measured faster) or K4, the
 *                                   persistent phase-scheduled query kernel (1)
 *   "query_tune"    "leafAt,dbl,maxExtra,burst,keep8"   scheduling weights of K4 (csrc/query_kernels.hpp QueryTune)
 *   "auto_rebuild"  0 | R > 1       0 (default) = off. A decimal ratio R above 1: mi_scene_update* runs the rebuild itself, before it returns, when
 *                                   the refitted tree has degraded. Set through this call only (no environment variable, as for the arithmetic
 *                                   options). The figure compared is est = (26 * sum_all + 224 * sum_leaf) / a_root of mi_scene_bvh_cost - 26
 *                                   and 224 are the static instruction counts of the box-test and the triangle-test step.
 *                                   Baseline: est of the tree right after the scene's last rebuild made with the option on; before that, est of
 *                                   the tree as it stood before the first update that found the option on and had no baseline (evaluated once).
 *                                   Decision: after an update has been APPLIED (a refused one never triggers it), est of the refitted tree is
 *                                   computed on the update's stream; if a_root > 0 and est > R * baseline (binary64), mi_scene_rebuild's work
 *                                   runs on the same stream under the same ordering rules, and the baseline becomes the rebuilt tree's est.
 *                                   An LBVH is a dearer tree than the host builder's (28.87 against 19.75 box tests per cast on the box scene,
 *                                   DESIGN.md §17), so a small R can fire once on a healthy tree; the scene then settles on the LBVH's
 *                                   baseline. mi_get_live_stats tells whether a rebuild happened. Renders and queries equal those of a fresh
 *                                   scene made from the current arrays and mi_scene_get_bvh's nodes either way.
 * None of them changes a result bit (auto_rebuild changes the tree, not what a cast returns beyond what mi_scene_rebuild itself documents). Two further keys select ARITHMETIC:
 *   "double_fallback" 0 | 1         the reference built with -DALLOW_DOUBLE_FALLBACK=1 (CMakeLists.txt:13,34-41; src/Mesh.cpp:38-51):
 *                                   edge functions that are exactly zero in binary32 are recomputed in binary64. Results are those
 *                                   of the reference's CPU path built the same way, bit for bit (default 0 = the reference default)
 *   "fast"            0 | 1         tolerance tier for plain path-trace renders of the default kernel and for ray queries: box test as FMAs, triangle
 *                                   test contracted, v_rcp_f32 in the cast set-up. NOT bit-exact: first hits name the same primitive
 *                                   with distance / point within 1e-6; see tests/test_gpu_parity.py (test_fast_tier_...) for the
 *                                   stated tolerance. Never the default. */
int mi_scene_set_option(mi_scene* scene, const char* key, const char* value);

/* The NIF environment evaluated stand-alone on device arrays: for i<n, bgr[i*3..] =
 * decode(MLP(fourier(u[i], v[i]))). Replaces NifModel::buildInference's execModel
 * (NifModel.cpp:249-356). d_u, d_v, d_bgr are DEVICE pointers. */
int mi_nif_infer_device(mi_scene* scene, const float* d_u, const float* d_v, float* d_bgr,
                        size_t n, void* hip_stream);

/* ---- several GPUs in one process -------------------------------------------------------
 * Replaces: the replicas of an IpuScene (RuntimeConfig.numIpus / numReplicas, trace.cpp:297-309; scene replicated per
 * device src/IpuScene.cpp:473-483; replicas pull disjoint ray batches round-robin from the one stream :676-684; every
 * batch is written back into the caller's stream :699-732 and handed to the callback, src/RayCallback.cpp:8-24).
 * mi_group_create builds one mi_scene per entry of `devices` (HIP ordinals; an ordinal may repeat - several replicas
 * then share that GPU, which is how the path is rehearsed on a one-GPU box). mi_group_render cuts the host stream into
 * ray batches (mi_group_set_ray_batch; default: one batch = the whole stream) and, for each batch: deals it in bands
 * (8 rows of the render window per band, band b to replica b % R: ipu_ray_lib_amd/csrc/ray_shard.hpp, also exported as
 * mi_shard_* by libmi_scene_host.so), uploads every replica's bands with one strided copy, traces every share on its
 * own HIP stream with no exchange while it renders, moves the finished shares to the first replica's device with ONE
 * RCCL group call (ncclSend / ncclRecv over xGMI), and copies them from there straight into their places in `rays`
 * (strided copies: no de-interleave pass, no second frame buffer). The callback is called once per batch, in batch
 * order, on the calling thread, as soon as that batch is home and while the next one is being traced. Every pixel owns
 * its RNG streams, so the result is bit-identical for any number of replicas and any batch size.
 * `transport`: 0 = RCCL as soon as more than one device takes part (peer copies otherwise), 1 = RCCL always, 2 = peer
 * copies only. RCCL is loaded with dlopen when the first group needs it.
 * mi_group_scene hands out a replica's scene for the per-scene setters (mi_scene_set_nif, mi_scene_set_option, ...),
 * which must be applied to every replica alike. The same holds for geometry updates: mi_scene_update / mi_scene_update_device on
 * every replica's scene, with the same arrays (there is no group-level update entry), and for mi_scene_rebuild: call it on every
 * replica's scene (the result is a function of the geometry alone, so the replicas stay alike). Option "auto_rebuild" likewise: set it
 * on every replica's scene, with the same ratio. The decision is a function of the geometry alone - the cost pass is bit-reproducible
 * and the compare is binary64 -, so replicas fed the same arrays rebuild in the same update and stay alike. New contents go the
 * same way: mi_scene_set_geometry / mi_scene_set_geometry_device on every replica's scene, with the same arrays (there is no
 * group-level entry; the result is a function of the arrays alone, and the replica keeps its place in the group). */
typedef struct mi_group mi_group;
int mi_group_create(const mi_scene_desc* desc, const int32_t* devices, uint32_t num_replicas, int32_t transport, mi_group** out);
void mi_group_destroy(mi_group* group);
uint32_t mi_group_size(const mi_group* group);
mi_scene* mi_group_scene(mi_group* group, uint32_t replica);
int mi_group_set_ray_batch(mi_group* group, size_t rays_per_batch);
int mi_group_render(mi_group* group, int mode, mi_trace_result* rays, size_t n, mi_ray_callback cb, void* user);
/* The stages of mi_group_render one by one, for callers that keep the shares RESIDENT on the devices (the reference
 * keeps a batch in remote buffers between executions the same way, src/IpuScene.cpp:399-409): upload deals and copies
 * the whole stream (one batch); trace renders every share where it lies and gathers the shares on the first replica's
 * device (rgb keeps accumulating from call to call, as with mi_render_device); download copies the gathered shares into
 * `rays` (n must be the uploaded count). bench.py --gpus N times mi_group_trace: inputs resident in HBM, the RCCL
 * gather inside the timed region. mi_group_gathered_device exposes the gathered buffer (shares replica after replica;
 * offsets[r] = first record of replica r's share, up to num_offsets entries) for device-side consumers. */
int mi_group_upload(mi_group* group, const mi_trace_result* rays, size_t n);
int mi_group_trace(mi_group* group, int mode);
int mi_group_download(mi_group* group, mi_trace_result* rays, size_t n);
int mi_group_gathered_device(mi_group* group, void** d_gathered, uint64_t* offsets, uint32_t num_offsets);
double mi_group_trace_time_secs(const mi_group* group);               /* wall time of the last mi_group_render / mi_group_trace */
int mi_group_get_counters(mi_group* group, uint64_t counts[4]);       /* summed over the replicas */
int mi_group_reset_counters(mi_group* group);
/* What the last mi_group_render (or stage call) moved: info[0] = RCCL send/recv pairs, info[1] = peer copies,
 * info[2] = bands dealt, info[3] = host->device copies issued, info[4] = device->host copies issued. */
int mi_group_last_transfer(const mi_group* group, uint64_t info[5]);
/* How long the last batch's gather took on the first replica's device, in milliseconds (HIP events on its stream: from
 * "its own share is traced" to "the last share has arrived" - a slower peer's remaining trace time included). Waits for
 * that gather. And the communicator the group built: `*distinct` = number of distinct devices (= RCCL ranks when the
 * transport is RCCL), the ordinals themselves in devices[0..capacity), root first. A multi-GPU record that reports
 * distinct == 1 was a one-GPU rehearsal (src/IpuScene.cpp:676-684 spreads the batches over real replicas). */
int mi_group_last_gather_ms(mi_group* group, double* ms);
int mi_group_devices(const mi_group* group, int32_t* devices, uint32_t capacity, uint32_t* distinct);

/* Thread-local message for the last failing call on this thread. Never NULL. */
const char* mi_last_error(void);

/* Library / build identification, e.g. "mi_raylib 0.1 gfx950 contract=off". */
const char* mi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MI_RAYLIB_H */
