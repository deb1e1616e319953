/*
 * mi_scene_host.h — C ABI of the host-side scene plumbing (CPU only, no GPU needed).
 *
 * These entry points reproduce the INPUTS the reference hands to its renderers — they are
 * the callers' side of the hot path, not the hot path itself:
 *   buildSceneDescription / makeCornellBoxScene / makePrimitiveScene  (src/app_utils.cpp:252-283,
 *                                                                      src/scene_utils.cpp:319-597)
 *   buildSceneData (array packing + BVH build driver)                 (src/app_utils.cpp:291-371)
 *   BvhBuilder::build + buildCompactBvh (node FORMAT is contractual,  (include/embree_utils/bvh.hpp:37-77,
 *     the Embree builder is not: tree topology is "parity unpinned")   src/CompactBvhBuild.cpp:5-56)
 *   initPerspectiveRayStream (no-jitter form) + zeroRgb               (src/app_utils.cpp:19-53)
 * The arrays they produce are what mi_scene_create (mi_raylib.h) and the CPU oracle consume.
 */
#ifndef MI_SCENE_HOST_H
#define MI_SCENE_HOST_H

#include "mi_raylib.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_host_scene mi_host_scene;   /* opaque; owns every array a desc points into */

/* Built-in scenes of the reference CLI (--scene box-simple | box | spheres, trace.cpp:357),
 * plus "monkey": the monkey bust alone in an open environment (BASELINE config 5).
 * `mesh_file` is the glTF-binary mesh placed on the short block for "box"
 * (assets/monkey_bust.glb in the reference, src/app_utils.cpp:264); ignored otherwise. */
int mi_host_scene_builtin(const char* scene_name, const char* mesh_file, mi_host_scene** out);

/* importScene(filename, loadNormals) (src/scene_utils.cpp:152-317, --mesh-file/--load-normals): a
 * complete scene with camera and materials from a Collada (.dae) file, camera moved to the origin,
 * materials re-interpreted with the reference's heuristics. */
int mi_host_scene_import(const char* file, int load_normals, mi_host_scene** out);

/* Build a scene from caller-provided arrays (same array contract as mi_scene_desc, but
 * bvh_nodes/max_leaf_depth are ignored and rebuilt). Used by tests with synthetic geometry.
 * A geometry is one mesh, sphere or disc; its geomID is 16 bit with 0xFFFF kept for "interior node"
 * (mi_bvh_node::geom_id) and mi_geom_ref::index is 16 bit. So num_meshes + num_spheres + num_discs above
 * 65535 is refused before anything is built, with MI_ERR_INVALID_ARG and mi_scene_create's words,
 * "more than 65535 geometries (geomID is 16 bit)"; that bound also keeps every mesh, sphere and disc index
 * inside mi_geom_ref::index. mi_host_scene_import refuses a file with more geometries the same way, and
 * the host twins below and mi_refit_compact_bvh refuse a desc whose num_geometry exceeds 65535. */
int mi_host_scene_from_arrays(const mi_scene_desc* geometry_only, mi_host_scene** out);

/* Fill `desc` with pointers into the host scene's storage and the reference CLI's default
 * render parameters (trace.cpp:343-366: 768x432, aa .25, path length 10, roulette depth 3,
 * 256 spp, seed 1442; fov from the scene's camera). The desc stays valid until destroy. */
int mi_host_scene_fill_desc(const mi_host_scene* scene, mi_scene_desc* desc);

void mi_host_scene_destroy(mi_host_scene* scene);

/* SAH BVH2 over axis-aligned boxes, one primitive per leaf, flattened depth-first with the
 * first child adjacent to its parent (CompactBVH2Node.hpp:60-63). lower/upper: 3 floats per
 * primitive. `nodes` must hold 2*n-1 entries. */
int mi_build_compact_bvh(const float* lower, const float* upper, const uint16_t* geom_ids,
                         const uint32_t* prim_ids, uint32_t n,
                         mi_bvh_node* nodes, uint32_t* num_nodes, uint32_t* max_leaf_depth);

/* Refit: the topology of desc->bvh_nodes (desc->num_nodes nodes: links, geomIDs, primIDs) kept, every box recomputed from desc's
 * geometry arrays - a leaf's the box of its primitive (a triangle's three vertices grown from an empty box, a sphere's or disc's
 * centre +- radius), an interior node's the union of its two children's - and encoded as mi_build_compact_bvh encodes it.
 * Writes desc->num_nodes nodes to `out` (which may alias desc->bvh_nodes). Fails with the builder's message ("Cannot compress BVH
 * bounds into fp16 (half)", MI_ERR_IO) on an extent above 65504, and with MI_ERR_INVALID_ARG on a node box that is not finite
 * (what mi_scene_create refuses) or an index out of range; `out` is then partly written. The reference the device refit
 * (mi_scene_update, mi_raylib.h) is checked against, and the way to build the fresh scene an updated one must equal. */
int mi_refit_compact_bvh(const mi_scene_desc* desc, mi_bvh_node* out);

/* Rebuild: a linear BVH (LBVH) over desc's primitives from desc's geometry arrays; desc's own bvh_nodes are ignored. The primitives
 * are taken in canonical order - geometry 0 .. num_geometry - 1, inside a mesh triangle 0 .. T - 1 -, keyed by the 63-bit Morton code
 * of their box centroid (lo + hi) * .5f quantised to 21 bits per axis inside the scene box, sorted by (key, canonical index), hung
 * into Karras' 2012 hierarchy (equal keys split by sorted position: coincident primitives give a balanced subtree), boxed bottom-up
 * as mi_refit_compact_bvh boxes them, each pair of children ordered by the builder's rule (box centre nearer the origin first, the
 * lower-key child on a tie) and laid out depth-first. `out` must hold 2 P - 1 nodes for P primitives (what the scene's own BVH
 * holds); *num_nodes = 2 P - 1 (0 for an empty scene) and *max_leaf_depth = the deepest leaf with the root at 1, at most
 * 63 + 32 + 1. Fails as mi_refit_compact_bvh fails, with the same messages: "Cannot compress BVH bounds into fp16 (half)"
 * (MI_ERR_IO) on an extent above 65504, MI_ERR_INVALID_ARG on a node box that is not finite or an index out of range. The twin
 * of the device rebuild (mi_scene_rebuild, mi_raylib.h), whose nodes equal these byte for byte, and the way to build the fresh
 * scene a rebuilt one must equal. */
int mi_build_lbvh_compact(const mi_scene_desc* desc, mi_bvh_node* out, uint32_t* num_nodes, uint32_t* max_leaf_depth);

/* The canonical primitive table of desc's geometry arrays: its primitives in canonical order (geometry 0 .. num_geometry - 1, inside
 * a mesh triangle 0 .. T - 1), 32 bytes each - eight uint32: {a, b, c, kind, geomID, primID, triBase, matIndex}; kind 0 = a triangle
 * (a, b, c = its absolute vertex indices, triBase = the index of its first uint16 in mesh_tris), 1 = a sphere, 2 = a disc (a = its
 * index in spheres / discs). It is what the LBVH builds sort, so it fixes the tree. The twin of the kernel that writes the table
 * for mi_scene_set_geometry* (mi_raylib.h), through the same code: the exclusive prefix of the geometries' primitive counts, then
 * per canonical index a binary search for its geometry (geometries without triangles are stepped over) and the record. desc's
 * nodes and render parameters are ignored. *count = the primitive count; `out` must hold it (out == NULL with capacity 0: only
 * the count). MI_ERR_INVALID_ARG with mi_scene_create's words for what it refuses of these arrays: null arrays that come with
 * counts, a geometry type, geometry index, material index or mesh range out of bounds, normals neither absent nor one per vertex,
 * more than 65535 geometries, too many primitives, a triangle's vertex index not below its mesh's num_vertices. */
int mi_canonical_prims(const mi_scene_desc* desc, void* out /* 32 B each */, uint32_t capacity, uint32_t* count);

/* The surface-area cost of a tree of n compact nodes, out = {sum_all, sum_leaf, a_root}: a node's term is
 * a = (ex * ey + ey * ez) + ez * ex in binary64 from its three binary16 extents (decoded exactly, every operation rounded once in
 * that order); sum_all sums it over all nodes (every visited node costs a box test), sum_leaf over the leaves (a primitive test
 * each), a_root is node 0's term. sum_all / a_root is the expected number of box tests of a random line through the root box,
 * sum_leaf / a_root that of primitive tests; the entry returns the raw sums (zeros for n == 0, and a_root == 0 is legal) and the
 * caller divides. The sums are formed in a fixed shape - blocks of 256 consecutive entries through a fixed binary tree, level by
 * level (ipu_ray_lib_amd/csrc/ray_math.h, cost_block_reduce) - which the device pass mi_scene_bvh_cost (mi_raylib.h) runs too:
 * the twin returns the same three doubles as the device, bit for bit. mi_bvh_cost_compact_block is the same with another block
 * width (a power of two, at least 2: tests reach three levels with 65 nodes and a width of 4). mi_bvh_cost_estimate is the
 * figure the auto-rebuild policy compares (mi_raylib.h, option "auto_rebuild"): (26 * sum_all + 224 * sum_leaf) / a_root. */
int mi_bvh_cost_compact(const mi_bvh_node* nodes, uint32_t n, double out[3]);
int mi_bvh_cost_compact_block(const mi_bvh_node* nodes, uint32_t n, uint32_t block, double out[3]);
double mi_bvh_cost_estimate(const double cost[3]);

/* Point queries on the host: the twin of mi_point_query / mi_point_query_device (mi_raylib.h, where the contract is written), for
 * the same `kind`, points and out (n mi_point_hit for MI_POINT_CLOSEST, n uint8_t for MI_POINT_WITHIN; no alignment asked). It walks
 * desc->bvh_nodes - compact nodes: max = min + (float)extent, one rounded add; first child first - in the device's order, resolves
 * every leaf's primitive from desc's arrays as mi_scene_create resolves it, and evaluates boxes and primitives through the code the
 * kernel runs (ipu_ray_lib_amd/csrc/point_math.hpp): it returns the bytes the device returns. visits (may be NULL) receives
 * {box tests, primitive evaluations} summed over the n points: what the device adds to "nodes visited" and "leaf tests" under option
 * full_stats. MI_ERR_INVALID_ARG: a null desc, an unknown kind, a null buffer with n > 0, nodes that are not a depth-first BVH2, a
 * leaf whose geometry, primitive or vertex index is out of range. */
int mi_point_query_host(const mi_scene_desc* desc, int kind, const mi_point* points, void* out, size_t n, uint64_t visits[2]);

/* Neighbour lists on the host: the twins of mi_near_offsets* / mi_near_fill* (mi_raylib.h, where the contract is written), over
 * desc->bvh_nodes and desc's arrays as mi_point_query_host reads them and through the same code (point_math.hpp). offsets: n + 1
 * uint64_t, written by mi_near_offsets_host (0, then the running total of the points' neighbour counts, the count walk over the
 * fixed bound) and read by mi_near_fill_host, which runs the fill's walk - the bound lowered to the last record's dist2 once a
 * segment is full - statement for statement and writes `hits` as the device writes it: nothing at or past `capacity`, nothing
 * outside a segment, a point with an empty segment not walked. No alignment asked. They return the bytes the device returns;
 * visits (may be NULL) receives {box tests, primitive evaluations} summed over the n points, what the device adds to "nodes visited"
 * and "leaf tests" under option full_stats. MI_ERR_INVALID_ARG, with the function's name in mi_host_last_error: a null desc, a null
 * buffer with n > 0, nodes that are not a depth-first BVH2, a leaf whose geometry, primitive or vertex index is out of range. */
int mi_near_offsets_host(const mi_scene_desc* desc, const mi_point* points, uint64_t* offsets /* n + 1 */, size_t n, uint64_t visits[2]);
int mi_near_fill_host(const mi_scene_desc* desc, const mi_point* points, const uint64_t* offsets, mi_neighbour* hits, size_t capacity,
                      size_t n, uint64_t visits[2]);

/* Box queries on the host: the twins of mi_box_query* / mi_box_offsets* / mi_box_fill* (mi_raylib.h, where the contract is written),
 * over desc->bvh_nodes and desc's arrays as mi_point_query_host reads them, boxes and primitives tested through the code the kernels
 * run (ipu_ray_lib_amd/csrc/box_math.hpp). out: n uint8_t (MI_BOX_ANY) or n uint32_t (MI_BOX_COUNT); offsets: n + 1 uint64_t, written
 * by mi_box_offsets_host (0, then the running total of the boxes' counts) and read by mi_box_fill_host, which writes `hits` as the
 * device writes it - the len smallest keys (geom_id, prim_id) of each box ascending, then the empty record; nothing at or past
 * `capacity`, nothing outside a segment, a box with an empty segment not walked. No alignment asked. They return the bytes the device
 * returns; visits (may be NULL) receives {box tests, primitive tests} summed over the n boxes, what the device adds to "nodes visited"
 * and "leaf tests" under option full_stats. MI_ERR_INVALID_ARG, with the function's name in mi_host_last_error: a null desc, an
 * unknown kind, a null buffer with n > 0, nodes that are not a depth-first BVH2, a leaf whose geometry, primitive or vertex index is
 * out of range. */
int mi_box_query_host(const mi_scene_desc* desc, int kind, const mi_box* boxes, void* out, size_t n, uint64_t visits[2]);
int mi_box_offsets_host(const mi_scene_desc* desc, const mi_box* boxes, uint64_t* offsets /* n + 1 */, size_t n, uint64_t visits[2]);
int mi_box_fill_host(const mi_scene_desc* desc, const mi_box* boxes, const uint64_t* offsets, mi_overlap* hits, size_t capacity,
                     size_t n, uint64_t visits[2]);

/* Triangle queries on the host: the twins of mi_tri_query* / mi_tri_offsets* / mi_tri_fill* (mi_raylib.h, where the contract is
 * written), over desc->bvh_nodes and desc's arrays as mi_point_query_host reads them, boxes and primitives tested through the code the
 * kernels run (ipu_ray_lib_amd/csrc/contact_math.hpp). out: n uint8_t (MI_TRI_ANY) or n uint32_t (MI_TRI_COUNT); offsets: n + 1
 * uint64_t, written by mi_tri_offsets_host (0, then the running total of the triangles' counts) and read by mi_tri_fill_host, which
 * writes `hits` as the device writes it - the len smallest keys (geom_id, prim_id) of each triangle ascending, then the empty record;
 * nothing at or past `capacity`, nothing outside a segment, a triangle with an empty segment not walked. No alignment asked. They
 * return the bytes the device returns; visits (may be NULL) receives {box tests, primitive tests} summed over the n triangles, what the
 * device adds to "nodes visited" and "leaf tests" under option full_stats. MI_ERR_INVALID_ARG, with the function's name in
 * mi_host_last_error: a null desc, an unknown kind, a null buffer with n > 0, nodes that are not a depth-first BVH2, a leaf whose
 * geometry, primitive or vertex index is out of range. */
int mi_tri_query_host(const mi_scene_desc* desc, int kind, const mi_tri* tris, void* out, size_t n, uint64_t visits[2]);
int mi_tri_offsets_host(const mi_scene_desc* desc, const mi_tri* tris, uint64_t* offsets /* n + 1 */, size_t n, uint64_t visits[2]);
int mi_tri_fill_host(const mi_scene_desc* desc, const mi_tri* tris, const uint64_t* offsets, mi_contact* hits, size_t capacity,
                     size_t n, uint64_t visits[2]);

/* Oriented-box queries on the host: the twins of mi_obox_query* / mi_obox_offsets* / mi_obox_fill* (mi_raylib.h, where the contract is
 * written), over desc->bvh_nodes and desc's arrays as mi_point_query_host reads them, boxes and primitives tested through the code the
 * kernels run (ipu_ray_lib_amd/csrc/obox_math.hpp). out: n uint8_t (MI_OBOX_ANY) or n uint32_t (MI_OBOX_COUNT); offsets: n + 1
 * uint64_t, written by mi_obox_offsets_host (0, then the running total of the boxes' counts) and read by mi_obox_fill_host, which
 * writes `hits` as the device writes it - the len smallest keys (geom_id, prim_id) of each box ascending, then the empty record;
 * nothing at or past `capacity`, nothing outside a segment, a box with an empty segment not walked. No alignment asked. They return
 * the bytes the device returns; visits (may be NULL) receives {box tests, primitive tests} summed over the n boxes, what the device
 * adds to "nodes visited" and "leaf tests" under option full_stats. MI_ERR_INVALID_ARG, with the function's name in
 * mi_host_last_error: a null desc, an unknown kind, a null buffer with n > 0, nodes that are not a depth-first BVH2, a leaf whose
 * geometry, primitive or vertex index is out of range. */
int mi_obox_query_host(const mi_scene_desc* desc, int kind, const mi_obox* oboxes, void* out, size_t n, uint64_t visits[2]);
int mi_obox_offsets_host(const mi_scene_desc* desc, const mi_obox* oboxes, uint64_t* offsets /* n + 1 */, size_t n, uint64_t visits[2]);
int mi_obox_fill_host(const mi_scene_desc* desc, const mi_obox* oboxes, const uint64_t* offsets, mi_overlap* hits, size_t capacity,
                      size_t n, uint64_t visits[2]);

/* obox_meets_bounds of mi_obox_* (mi_raylib.h) on its own: 1 when the bounds [mn, mx] meet the oriented box, 0 when they do not or
 * the query is not valid, from the function the kernels and the twins run. What the tests pin the test's monotonicity with. A null
 * pointer gives 0. */
int mi_obox_meets_bounds_host(const mi_obox* obox, const float mn[3], const float mx[3]);

/* Capsule queries on the host: the twins of mi_capsule_query* / mi_capsule_offsets* / mi_capsule_fill* (mi_raylib.h, where the contract
 * is written), over desc->bvh_nodes and desc's arrays as mi_point_query_host reads them, boxes and primitives tested through the code
 * the kernels run (ipu_ray_lib_amd/csrc/capsule_math.hpp). out: n uint8_t (MI_CAPSULE_ANY) or n uint32_t (MI_CAPSULE_COUNT); offsets:
 * n + 1 uint64_t, written by mi_capsule_offsets_host (0, then the running total of the capsules' counts) and read by
 * mi_capsule_fill_host, which writes `hits` as the device writes it - the len smallest keys (geom_id, prim_id) of each capsule
 * ascending, then the empty record; nothing at or past `capacity`, nothing outside a segment, a capsule with an empty segment not
 * walked. No alignment asked. They return the bytes the device returns; visits (may be NULL) receives {box tests, primitive tests}
 * summed over the n capsules, what the device adds to "nodes visited" and "leaf tests" under option full_stats.
 * MI_ERR_INVALID_ARG, with the function's name in mi_host_last_error: a null desc, an unknown kind, a null buffer with n > 0, nodes
 * that are not a depth-first BVH2, a leaf whose geometry, primitive or vertex index is out of range. */
int mi_capsule_query_host(const mi_scene_desc* desc, int kind, const mi_capsule* capsules, void* out, size_t n, uint64_t visits[2]);
int mi_capsule_offsets_host(const mi_scene_desc* desc, const mi_capsule* capsules, uint64_t* offsets /* n + 1 */, size_t n, uint64_t visits[2]);
int mi_capsule_fill_host(const mi_scene_desc* desc, const mi_capsule* capsules, const uint64_t* offsets, mi_overlap* hits, size_t capacity,
                         size_t n, uint64_t visits[2]);

/* capsule_meets_bounds of mi_capsule_* (mi_raylib.h) on its own: 1 when the bounds [mn, mx] meet the capsule, 0 when they do not or
 * the query is not valid, from the function the kernels and the twins run. What the tests pin the test's monotonicity with. A null
 * pointer gives 0. */
int mi_capsule_meets_bounds_host(const mi_capsule* capsule, const float mn[3], const float mx[3]);

/* Frustum queries on the host: the twins of mi_frustum_query* / mi_frustum_offsets* / mi_frustum_fill* (mi_raylib.h, where the contract
 * is written), over desc->bvh_nodes and desc's arrays as mi_point_query_host reads them, boxes and primitives tested through the code
 * the kernels run (ipu_ray_lib_amd/csrc/frustum_math.hpp). out: n uint8_t (MI_FRUSTUM_ANY) or n uint32_t (MI_FRUSTUM_COUNT); offsets:
 * n + 1 uint64_t, written by mi_frustum_offsets_host (0, then the running total of the frusta's counts) and read by
 * mi_frustum_fill_host, which writes `hits` as the device writes it - the len smallest keys (geom_id, prim_id) of each frustum
 * ascending, then the empty record; nothing at or past `capacity`, nothing outside a segment, a frustum with an empty segment not
 * walked. No alignment asked. They return the bytes the device returns; visits (may be NULL) receives {box tests, primitive tests}
 * summed over the n frusta, what the device adds to "nodes visited" and "leaf tests" under option full_stats.
 * MI_ERR_INVALID_ARG, with the function's name in mi_host_last_error: a null desc, an unknown kind, a null buffer with n > 0, nodes
 * that are not a depth-first BVH2, a leaf whose geometry, primitive or vertex index is out of range. */
int mi_frustum_query_host(const mi_scene_desc* desc, int kind, const mi_frustum* frusta, void* out, size_t n, uint64_t visits[2]);
int mi_frustum_offsets_host(const mi_scene_desc* desc, const mi_frustum* frusta, uint64_t* offsets /* n + 1 */, size_t n, uint64_t visits[2]);
int mi_frustum_fill_host(const mi_scene_desc* desc, const mi_frustum* frusta, const uint64_t* offsets, mi_overlap* hits, size_t capacity,
                         size_t n, uint64_t visits[2]);

/* frustum_meets_bounds of mi_frustum_* (mi_raylib.h) on its own: 1 when the bounds [mn, mx] meet the region, 0 when they do not or
 * the query is not valid, from the function the kernels and the twins run. What the tests pin the test's monotonicity with. A null
 * pointer gives 0. */
int mi_frustum_meets_bounds_host(const mi_frustum* frustum, const float mn[3], const float mx[3]);

/* Rigid poses on the host: the twin of the pose pass of mi_scene_set_poses* (mi_raylib.h, where the contract is written). `rest`
 * holds the rest geometry - its geometry list, mesh_info, vertices, normals, spheres and discs are read, nothing else -, poses one
 * mi_pose per geometry entry. Writes the posed arrays - rest->num_verts vertices, as many normals (normals_out may be NULL when the
 * scene has none), num_spheres spheres, num_discs discs - through the code the kernel runs (ipu_ray_lib_amd/csrc/pose_math.hpp): the
 * bytes the device hands to its refit. Records no geometry owns and geometries under the identity pose keep their rest bytes.
 * MI_ERR_INVALID_ARG, with the function's name in mi_host_last_error: a null desc, null poses with num_geometry > 0, a num_geometry
 * that differs from rest's, a null output for a kind the scene has, a geometry reference or vertex range out of bounds, an invalid
 * pose, an ownership conflict (two meshes' vertex ranges intersect; one mesh, sphere or disc referenced twice): nothing is
 * written then. num_geometry == 0 on a description of zero geometries reads no pose. */
int mi_pose_geometry_host(const mi_scene_desc* rest, const mi_pose* poses, uint32_t num_geometry, mi_vec3* verts_out, mi_vec3* normals_out,
                          mi_sphere* spheres_out, mi_disc* discs_out);

/* Sphere crossings on the host: how often the ray origin + t direction, t_min < t < t_max, crosses the shell of the sphere (centre,
 * radius2 = the squared radius) - 0, 1 or 2 -, from the definition the crossing-count kernels run (mi_count_query / mi_point_sign,
 * mi_raylib.h, where the formula is written; ipu_ray_lib_amd/csrc/cross_math.hpp). The triangle and disc tests of a crossing count
 * are the reference's and are checked against the CPU oracle; this is the part with no reference counterpart. A null pointer gives 0. */
uint32_t mi_sphere_crossings_host(const float centre[3], float radius2, const float origin[3], const float direction[3],
                                  float t_min, float t_max);

/* The same crossings with their t, as a crossing list reports them (mi_list_fill, mi_raylib.h; sphere_roots of cross_math.hpp): a
 * mask of the accepted roots - bit 0: the near root, written to t[0]; bit 1: the far root (MI_CROSS_FAR), written to t[1] -, whose
 * number of set bits is mi_sphere_crossings_host of the same arguments. A line that misses the sphere leaves t as it was. A null
 * pointer gives 0. */
uint32_t mi_sphere_roots_host(const float centre[3], float radius2, const float origin[3], const float direction[3],
                              float t_min, float t_max, float t[2]);

/* The hot-first order of the private copy of the walk's arrays that plain renders may walk (scene option "hot_nodes", mi_raylib.h),
 * from the functions the device library's upload runs (ipu_ray_lib_amd/csrc/hot_order.hpp). For num_nodes compact nodes (a depth-first
 * BVH2) it writes, each num_nodes entries long: preorder - the 32-byte device nodes of the shared array (six floats min/max per axis,
 * then the two successors as byte offsets: link, hit); order - order[k] = the preorder index of the node at place k of the private
 * array (chains of first children by falling half-area of their first box, ties by preorder index, the root's chain first); hot - the
 * private node array; leaf_link - per private node, the byte offset of the node that follows a leaf (its record carries it; 0 for
 * interior nodes). MI_ERR_INVALID_ARG: a null pointer with num_nodes > 0, 2^26 nodes or more, nodes that are not a depth-first BVH2. */
int mi_hot_nodes(const mi_bvh_node* compact, uint32_t num_nodes, void* preorder, uint32_t* order, void* hot, uint32_t* leaf_link);

/* share[k - 1] = the share of a random line's box tests that falls on the first k nodes of `order`, under the surface-area model (a
 * node is tested when its parent's box is hit; probability proportional to that box's half-area): what the default of option
 * "hot_nodes" is decided from. preorder and order as mi_hot_nodes writes them. */
int mi_hot_share(const void* preorder, uint32_t num_nodes, const uint32_t* order, double* share);

/* The stackless walk of such a node array for the ray origin + t direction, t in [0, inf), with no primitive ever shortening it:
 * visits[] receives, up to capacity entries, the index of every node whose box is tested, followed - for a leaf whose box is hit -
 * by the same index with bit 31 set (the primitive test); the return value is the number of entries the walk makes. leaf_link = NULL
 * walks the shared array's protocol (preorder), otherwise the layout-free one of the private array. *status (may be NULL) becomes
 * MI_ERR_INVALID_ARG when a successor points outside the array or the walk does not end, else MI_OK. */
uint32_t mi_hot_walk(const void* nodes, uint32_t num_nodes, const uint32_t* leaf_link, const float origin[3], const float direction[3],
                     uint32_t* visits, uint32_t capacity, int* status);

/* The collapsed tree plain renders walk where the private copy is on (ipu_ray_lib_amd/csrc/hot_order.hpp): an interior node other than
 * the root is taken out of the walk when both children's stored boxes lie inside its own (all six floats) and its half-area exceeds
 * theta times that of its nearest surviving ancestor (theta < 0: the constant the device library uses); every successor that pointed
 * at it points at its first child, transitively. Writes, num_nodes entries each: preorder (as mi_hot_nodes), keep (1 = the node
 * survives); and, counts[0] = the number of survivors entries each (the buffers hold num_nodes): from - the preorder index of
 * survivor j; collapsed - the survivors as a preorder array of their own (the shared array's protocol: mi_hot_walk with
 * leaf_link = NULL); order, hot, leaf_link, share - as mi_hot_nodes and mi_hot_share give them, over the survivors. counts[1] = the
 * interior nodes the area rule alone would take out and the containment rule keeps. Errors as mi_hot_nodes. */
int mi_hot_collapse(const mi_bvh_node* compact, uint32_t num_nodes, double theta, void* preorder, uint8_t* keep, uint32_t* from, void* collapsed,
                    uint32_t* order, void* hot, uint32_t* leaf_link, double* share, uint32_t counts[2]);

/* The node array plain renders walk where the private copy is on: the collapsed tree's m nodes (hot, leaf_link of mi_hot_collapse), then all
 * n nodes (hot, leaf_link of mi_hot_nodes) with their successors moved behind them; joined and joined_link hold m + n entries. A cast on
 * the literal box test (mi_hot_cast_is_literal: a reciprocal direction component or an origin component that is not finite) starts at
 * place *exact_start = m, every other cast at place 0: for a flat box on a face of the box around it the literal test can hit the inner
 * box and miss the outer one, so such casts never walk the collapsed tree. */
int mi_hot_join(const void* thin, const uint32_t* thin_link, uint32_t m, const void* full, const uint32_t* full_link, uint32_t n, void* joined, uint32_t* joined_link,
                uint32_t* exact_start);
int mi_hot_cast_is_literal(const float origin[3], const float direction[3]);

/* mi_hot_walk from node `start` (an index) for the segment t in [0, t_max] (t_max = a cast's hit.t while the boxes are tested; INFINITY: no hit
 * yet), the far slab product scaled as the kernels' box test scales it; *box_tests (may be NULL) receives the number of box tests of the walk. */
uint32_t mi_hot_walk_count(const void* nodes, uint32_t num_nodes, const uint32_t* leaf_link, uint32_t start, const float origin[3], const float direction[3], float t_max,
                           uint32_t* visits, uint32_t capacity, uint32_t* box_tests, int* status);

/* The tangent frame a diffuse bounce builds about `normal` (ipu_ray_lib_amd/csrc/ray_math.h diffuse_frame), and the per-leaf records a
 * scene WITHOUT vertex normals keeps of it (scene option "leaf_frame", mi_raylib.h; ipu_ray_lib_amd/csrc/leaf_frame.hpp, from the function
 * the device library's upload runs): frames receives, for each of `count` places, the eight floats {xb, 0, yb, 0} of the node at[k]
 * (at = NULL: node k; count <= num_nodes then) - the frame about a triangle leaf's face normal or a disc leaf's plane normal, zeros
 * for sphere leaves and interior nodes. normals (may be NULL) receives three floats per NODE: the normal the frame was built about
 * (zeros where there is none). `at` = the "place" list of a private copy gives that copy's records. */
void mi_diffuse_frame(const float normal[3], float xb[3], float yb[3]);
int mi_leaf_frames(const mi_scene_desc* desc, const uint32_t* at, uint32_t count, float* frames, float* normals);

/* initPerspectiveRayStream(rayStream, image, data, nullptr) + zeroRgb: window_w*window_h rays in
 * row-major window order, origin 0, un-jittered pinhole directions, u=row, v=col. */
int mi_init_ray_stream(const mi_scene_desc* desc, mi_trace_result* rays, size_t capacity);

/* scaleRgb (src/app_utils.cpp:55-59) */
void mi_scale_rgb(mi_trace_result* rays, size_t n, float scale);

/* ---- serialised scene -----------------------------------------------------------
 * The byte stream the reference's Serialiser<16> writes for a SceneRef (include/serialisation/
 * serialisation.hpp:33-53, src/IpuScene.cpp:51-53) and Deserialiser<16> aliases in place
 * (deserialisation.hpp:43-59). Layout is documented in ipu_ray_lib_amd/csrc/scene_blob.hpp. The blob
 * carries the eight scene arrays and maxLeafDepth .. samplesPerPixel; spheres, discs, rng seed, crop
 * window, pathTrace and device are not part of it.
 *   mi_scene_blob_size      bytes mi_scene_serialise will write for `desc`
 *   mi_scene_serialise      writes the blob; MI-host error if capacity is too small
 *   mi_scene_deserialise    fills `desc`'s array pointers with views INTO `blob` (which must be 16-byte
 *                           aligned and outlive the desc) and the eight scalars; other fields untouched.
 *                           A truncated blob fails with "Deserialiser encountered end of byte stream." */
size_t mi_scene_blob_size(const mi_scene_desc* desc);
int mi_scene_serialise(const mi_scene_desc* desc, uint8_t* out, size_t capacity, size_t* written);
int mi_scene_deserialise(const uint8_t* blob, size_t size, mi_scene_desc* desc, size_t* consumed);
/* Padding the format inserts before an object of alignment `align` at byte offset `offset`
 * (Serialiser::calculatePadding, Serialiser.hpp:30-39). */
uint32_t mi_blob_padding(uint32_t base_align, size_t offset, uint32_t align);

/* ---- ray-band sharding -----------------------------------------------------------
 * How a ray stream is dealt to the R replicas of a multi-GPU render and put together again; replaces the
 * round-robin batch pull of the reference's replicas (src/IpuScene.cpp:676-684, src/RayCallback.cpp:8-24).
 * The stream is cut into bands of `band` consecutive rays, band b belongs to replica b % R. One definition
 * (ipu_ray_lib_amd/csrc/ray_shard.hpp) serves these functions, mi_group_render and the Python ranks of bench.py.
 *   mi_shard_band_rays     band length for a stream of n rays rendered for a window `window_w` pixels wide: 8 rows
 *                          of the window when the stream is made of full rows, else 4096 rays
 *   mi_shard_count         rays replica r renders
 *   mi_shard_stream_index  out[k] = stream position of the k-th ray of replica r's stream
 *   mi_shard_frame_index   out[i] = position of stream ray i in the gathered buffer (replica 0's stream, then
 *                          replica 1's, ...): the de-interleave map the frame is assembled with            */
size_t mi_shard_band_rays(size_t n, uint32_t window_w);
size_t mi_shard_count(size_t n, size_t band, uint32_t replicas, uint32_t r);
int mi_shard_stream_index(size_t n, size_t band, uint32_t replicas, uint32_t r, uint64_t* out, size_t capacity);
int mi_shard_frame_index(size_t n, size_t band, uint32_t replicas, uint64_t* out);

/* ---- NIF assets ----------------------------------------------------------------
 * IpuScene::loadNifModel(assetPath) (src/IpuScene.cpp:174-187) reads <assetPath>/nif_metadata.txt
 * (NifMetaData.cpp:11-71) and <assetPath>/converted.hdf5, a Keras "Functional" model whose Dense layers
 * are stored under /model_weights/<layer>/<layer>/{kernel:0,bias:0} as float16 or float32
 * (src/keras/Hdf5Model.cpp:62-133). mi_host_nif_load does the same and hands the layers back in the
 * form mi_scene_set_nif takes (binary32 arrays; binary16 weights are widened exactly). HDF5 is reached
 * through the plugin libmi_nif_h5.so next to this library; if <assetPath>/converted.hdf5 is absent,
 * <assetPath>/nif_weights.bin is read instead: u32 numLayers, then per layer u32 rows, u32 cols,
 * u8 relu, u8 hasBias, f32 kernel[rows*cols] (Keras kernel:0 order), f32 bias[cols] if hasBias. */
typedef struct mi_host_nif mi_host_nif;

typedef struct mi_nif_desc {
  uint32_t num_layers;
  const float* const* kernels;   /* [num_layers] -> rows[i]*cols[i] floats, row-major */
  const float* const* biases;    /* [num_layers] -> cols[i] floats or NULL */
  const uint32_t* rows;
  const uint32_t* cols;
  const uint8_t* relu;           /* activation "relu" -> 1, "linear" -> 0 (NifModel.cpp:75-77, 324) */
  uint32_t embedding_dimension;  /* nif_metadata.txt */
  uint32_t hidden_size;          /* argument after --layer-size in train_command (0 if absent) */
  float max_value;
  float mean[3];                 /* eps already folded in when log_tonemap (NifMetaData.cpp:48-53) */
  int32_t log_tonemap;
  int32_t weights_are_half;      /* any kernel stored as float16 */
  const char* name;
  const char* source;            /* the weights file that was read */
} mi_nif_desc;

int mi_host_nif_load(const char* asset_path, mi_host_nif** out);
int mi_host_nif_describe(const mi_host_nif* nif, mi_nif_desc* desc);   /* pointers valid until destroy */
void mi_host_nif_destroy(mi_host_nif* nif);
const char* mi_host_nif_last_error(void);

const char* mi_host_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
