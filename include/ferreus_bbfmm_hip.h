/*
 * ferreus_bbfmm_hip.h -- C ABI of the MI355X-native BBFMM evaluator.
 *
 * Drop-in boundary for the hot path of graphic-goose/ferreus_rbf_rs: the
 * `ferreus_bbfmm` matrix-vector product behind the type-erased evaluator
 * `ferreus_rbf_utils::FmmTree` (ferreus_rbf_utils/src/utils.rs:383-494).  The
 * reference has no FFI for this path; every entry point below cites the Rust
 * method it replaces (paths relative to the reference repository root).  A
 * Rust `extern "C"` shim / ctypes stub binding these symbols is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *   - all matrices are f64, column-major with an explicit leading dimension
 *     (faer::Mat layout); `pts` are N x d (column a at pts + a*ld).
 *   - one in-flight call per handle (the reference wraps the tree in a Mutex,
 *     ferreus_rbf/src/rbf.rs:87,106,124); a handle may be used from any thread.
 *   - nothing throws across the ABI; every function returns a bbfmm_status.
 *   - the library fails loudly (BBFMM_DEVICE_ERROR) when no HIP device is
 *     usable: there is no CPU fallback for the compute entry points.
 */
#ifndef FERREUS_BBFMM_HIP_H
#define FERREUS_BBFMM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Return codes.  1 and 2 mirror FmmError (ferreus_bbfmm/src/bbfmm.rs:20-27). */
typedef enum {
    BBFMM_OK = 0,
    BBFMM_POINT_OUTSIDE_TREE = 1,         /* FmmError::PointOutsideTree{point_index} */
    BBFMM_KERNEL_NO_GRADIENTS = 2,        /* FmmError::KernelDoesNotSupportGradients */
    BBFMM_BAD_ARGUMENT = 3,               /* the reference panics (e.g. bbfmm.rs:293-298) */
    BBFMM_DEVICE_ERROR = 4,               /* HIP failure or no device */
    BBFMM_UNSUPPORTED = 5,                /* valid in the reference, not built here yet */
    BBFMM_CALLBACK_FAILED = 6             /* a caller's field callback returned nonzero (bbfmm_isosurfaces_from_function_opts) */
} bbfmm_status;

/* KernelType, in registry order (ferreus_rbf_utils/src/utils.rs:558-571).
 * Ids >= 100 are extension kernels of this repository that the reference does
 * not ship (BASELINE.json configs name them); their only oracle is the dense sum. */
typedef enum {
    BBFMM_KERNEL_LINEAR_RBF = 0,
    BBFMM_KERNEL_THIN_PLATE_SPLINE_RBF = 1,
    BBFMM_KERNEL_CUBIC_RBF = 2,
    BBFMM_KERNEL_SPHEROIDAL3_RBF = 3,
    BBFMM_KERNEL_SPHEROIDAL5_RBF = 4,
    BBFMM_KERNEL_SPHEROIDAL7_RBF = 5,
    BBFMM_KERNEL_SPHEROIDAL9_RBF = 6,
    BBFMM_KERNEL_LAPLACIAN = 7,
    BBFMM_KERNEL_ONE_OVER_R2 = 8,
    BBFMM_KERNEL_ONE_OVER_R4 = 9,
    BBFMM_KERNEL_GAUSSIAN_EXT = 100,      /* exp(-(r/base_range)^2)      -- extension */
    BBFMM_KERNEL_MULTIQUADRIC_EXT = 101   /* sqrt(1+(r/base_range)^2)    -- extension */
} bbfmm_kernel_type;

/* M2LCompressionType (ferreus_bbfmm/src/bbfmm.rs:62-73). */
typedef enum {
    BBFMM_COMPRESSION_NONE = 0,
    BBFMM_COMPRESSION_SVD = 1,
    BBFMM_COMPRESSION_ACA = 2
} bbfmm_compression_type;

/* FmmParams (ferreus_bbfmm/src/bbfmm.rs:77-104). */
typedef struct {
    int64_t max_points_per_cell;   /* default 256 */
    int32_t compression_type;      /* bbfmm_compression_type, default ACA */
    double epsilon;                /* default 10^-interpolation_order */
    int64_t eval_chunk_size;       /* default 1024 (host chunking knob of the reference; kept for API parity) */
} bbfmm_params;

/* Fills FmmParams::new_defaults(interpolation_order) (bbfmm.rs:96-103). */
void bbfmm_params_defaults(int32_t interpolation_order, bbfmm_params *out);

typedef struct bbfmm_handle bbfmm_handle;

/* Creation flags. */
#define BBFMM_FLAG_HOST_ONLY 1u /* build tree/lists/operators on the host only; no device is
                                   touched and every compute call returns BBFMM_DEVICE_ERROR.
                                   Used by the CPU-side structure tests. */
#define BBFMM_FLAG_M2L_SHARED_BASIS 2u /* EXTENSION beyond the reference (off by default): the M2L stages run on
                                        * coordinates in one orthonormal basis per level (the dominant subspace of
                                        * all of the level's compressed operators, cut at params.epsilon by the
                                        * operators' own rule: rank 107 of 343 for LinearRbf at order 7, 183-259 of 729
                                        * for the thin-plate spline at order 9), with the reference's factors
                                        * projected onto it.  About a third of the M2L flops; results
                                        * differ from the default path by the projection error (a few epsilon of the
                                        * far field; tests/test_gpu_shared_basis.py).  Needs a compressed operator
                                        * type (ACA or SVD) and a device; when the basis would keep more than 60 % of
                                        * the nodes (short-range spheroidal kernels) the default stages run and
                                        * bbfmm_tree_stats.m2l_basis_len stays 0. */
#define BBFMM_FLAG_DIRECT_SMALL_W_LEAVES 4u /* EXTENSION beyond the reference (off by default): a W-list cell that is a leaf
                                        * with no more points than the expansion has nodes is treated as near field --
                                        * its points are summed directly (both ways: the transposed X-list entry goes
                                        * too) instead of through M2P / P2L, which cost `nodes` kernel evaluations per
                                        * target where the direct sum costs `points`.  Exact where the reference
                                        * approximates, so results move by the reference's own M2P / P2L error (about
                                        * epsilon); on mixed-level trees of moderate size these two passes dominate the
                                        * matvec (1M uniform points, Spheroidal3: 9 of 14 ms). */
#define BBFMM_FLAG_DETERMINISTIC 8u /* bitwise reproducible results from run to run, as the reference's fixed-order
                                    * per-target sums are.  The default one-rhs matvec accumulates through hardware f64
                                    * atomics in three places (column sums of the unordered-pair near field, L and the
                                    * potentials of the fused M2P + P2L pass, the contraction split of M2L stage 2 on
                                    * small trees) and M2P adds the chunks of a leaf's W list atomically: the last bits
                                    * of a result depend on the scheduling (differences <= 1e-12 relative; an FGMRES run
                                    * near its tolerance may take one iteration more or less).  With this flag the handle
                                    * uses the ordered-pair kernels, one M2P job per leaf and plain stores in stage 2:
                                    * every sum has a fixed order (about 1.1x slower at 10M points, 1.5x on mixed-level
                                    * trees).  Same arithmetic as the reference either way. */

/*
 * FmmTree::new (ferreus_rbf_utils/src/utils.rs:392-421 -> ferreus_bbfmm/src/bbfmm.rs:272-353).
 * Copies the points (the caller keeps its buffer), builds the Morton tree, the
 * U/V/W/X lists and the M2L operators on the host and uploads them.
 *   pts       N x d column-major, leading dimension ld (>= n)
 *   extents   NULL (computed from the data, bbfmm.rs:281-284) or 2*d values
 *             [mins..., maxs...]
 *   params    NULL -> FmmParams::new_defaults(order)
 * d must be 1, 2 or 3 (bbfmm.rs:293-298).
 */
int bbfmm_create(const double *pts, int64_t n, int32_t d, int64_t ld, int32_t interpolation_order,
                 int32_t kernel_type, double base_range, double total_sill, int32_t adaptive_tree,
                 int32_t sparse, const double *extents, const bbfmm_params *params,
                 uint32_t flags, bbfmm_handle **out);

/*
 * One handle, several devices, ONE process (round 6).  The reference keeps a single FmmTree behind a Mutex
 * (ferreus_rbf/src/rbf.rs:85-133) and its FGMRES is not an SPMD program, so the GPUs of a node are reached behind the
 * unchanged method set of ferreus_rbf_utils::FmmTree (utils.rs:392-449): a handle created on a device list owns one
 * part per list entry -- the tree on that device and one subtree partition of the matvec -- and
 * bbfmm_set_weights + bbfmm_evaluate at the sources, bbfmm_fast_matrix_vector_product (all rows) and
 * bbfmm_matvec_device run partitioned over the parts: weights to every device over its own link, own-subtree upward
 * pass, the partial coarse multipoles copied to a slot on every device (peer copies beside the near field) and added in
 * part order, restricted downward + leaf pass, the owned blocks of the potentials straight back to the host (or, for
 * device callers, to the first device).  No caller-supplied collective, no second process.  Arbitrary targets (values,
 * gradients, Leaves mode after bbfmm_set_local_coefficients) with the weights of bbfmm_set_weights are SHARDED by target rows
 * when there are at least 16384 per part (BBFMM_GROUP_SHARD_MIN): every part completes its own multipoles from its
 * device's copy of the weights and evaluates a contiguous share of the rows (bbfmm_last_evaluate_at_sources: 3).  Row subsets
 * (bbfmm_fast_matrix_vector_product with target_indices; the unchanged caller's evaluate at rows of the sources from the second
 * sighting of a set on) are dealt to the parts that own the rows.  Everything else (few targets, other weights than
 * set_weights') is served by the first device alone, with unchanged results.
 *   devices    n_devices HIP device ids; the first one holds the handle's own tree (introspection, bbfmm_stream,
 *              device-resident vectors).  An id may repeat: logical parts on one device -- the one-GPU rehearsal of the
 *              N-device path (peer copies become device copies).  One entry: a plain handle on that device.
 * bbfmm_create itself reads FERREUS_BBFMM_DEVICES ("0,1,2,3", "all", "0,0,0"; unset or empty: the current device, no
 * group) -- the reference's constructor has no argument for a device list, so the unchanged caller is switched there.
 * The calling thread's current device is restored before returning.
 */
int bbfmm_create_on_devices(const double *pts, int64_t n, int32_t d, int64_t ld, int32_t interpolation_order,
                            int32_t kernel_type, double base_range, double total_sill, int32_t adaptive_tree,
                            int32_t sparse, const double *extents, const bbfmm_params *params, uint32_t flags,
                            const int32_t *devices, int32_t n_devices, bbfmm_handle **out);
int32_t bbfmm_device_count(const bbfmm_handle *h);              /* parts of the handle (1: no group) */
int32_t bbfmm_part_device(const bbfmm_handle *h, int32_t part); /* HIP device of a part; part 0 = the handle's own device */
int bbfmm_group_bounds(const bbfmm_handle *h, int64_t *bounds_out); /* parts + 1 offsets into the sorted points (group handles) */
int bbfmm_get_part_phase_ms(bbfmm_handle *h, int32_t part, double *ms_out, int64_t *count_out); /* bbfmm_get_phase_ms of one part */

void bbfmm_destroy(bbfmm_handle *h);

/* Message of the last failure on this handle ("" if none). Owned by the handle. */
const char *bbfmm_last_error(const bbfmm_handle *h);

/* FmmTree::set_weights (utils.rs:425-429 -> bbfmm.rs:383-401): upward pass.
 * w is rows x k (rows >= N; only rows < N are read), leading dimension ldw. */
int bbfmm_set_weights(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw);

/* FmmTree::set_local_coefficients (utils.rs:433-437 -> bbfmm.rs:518-524). */
int bbfmm_set_local_coefficients(bbfmm_handle *h, const double *w, int64_t rows, int32_t k,
                                 int64_t ldw);

/* FmmTree::evaluate (utils.rs:441-449 -> bbfmm.rs:411-418): downward pass restricted
 * to the ancestors of the target leaves + leaf pass.  x is m x d (ldx), out is
 * m x k (ldo), caller allocated.  On BBFMM_POINT_OUTSIDE_TREE *bad_point_index
 * receives the smallest offending row (linear_tree.rs:505-517). */
int bbfmm_evaluate(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw,
                   const double *x, int64_t m, int64_t ldx, double *out, int64_t ldo,
                   int64_t *bad_point_index);
/* The unchanged caller of the FGMRES matvec (rbf.rs:1357-1364) calls set_weights(w) and then
 * evaluate(w, select_mat_rows(source_points, all rows)).  bbfmm_evaluate recognises that sequence without being
 * told: m == N targets that equal the handle's source points bit for bit and row for row (threaded comparison on
 * the host, run beside the M2L) are served by the resident sorted target set -- every unordered near-field pair
 * once, M2P fused with P2L, no target upload or grouping -- and weights equal to those of the preceding
 * bbfmm_set_weights are not transferred a second time.  One differing bit (a perturbed coordinate, two rows
 * swapped, -0.0 for 0.0) takes the general path.  Results of the two paths agree to summation order (1e-12).
 * The same caller's matvec_partial (rbf.rs:119-133: target_indices = Some(idx)) evaluates at
 * select_mat_rows(source_points, idx): on a handle created the way the solver creates its tree (sparse, extents NULL:
 * rbf.rs:456-467), targets that are ROWS of the sources (one rhs, N / 2048 <= m <= N / 2 rows, each
 * found bit for bit in a table over the source points that the first such call builds) are served by the cached plan
 * bbfmm_fast_matrix_vector_product(target_indices) uses -- sorted targets and restricted downward pass once per index
 * set, not once per call.  One target that is no source point takes the general path.
 * Returns which path the last bbfmm_evaluate on this handle took: 1 the resident sources, 2 the cached plan of a row
 * subset, 0 the general path.  BBFMM_EVAL_SOURCES_FAST=0 in the environment disables both detections (checker). */
int bbfmm_last_evaluate_at_sources(const bbfmm_handle *h);
/* The comparison itself (host only, also on BBFMM_FLAG_HOST_ONLY handles): 1 when x (m x d, ldx) equals the handle's
 * source points bit for bit and row for row, else 0. */
int bbfmm_debug_targets_are_sources(const bbfmm_handle *h, const double *x, int64_t m, int64_t ldx);
/* ... and the lookup of targets that are rows of the sources: 1 and rows_out[j] = a source row with the coordinates of
 * target j (rows with equal coordinates are interchangeable) when every target is a source point, else 0. */
int bbfmm_debug_rows_of_sources(bbfmm_handle *h, const double *x, int64_t m, int64_t ldx, int64_t *rows_out);

/* FmmTree::evaluate_with_gradients (utils.rs:453-461 -> bbfmm.rs:434-441).
 * grad is m x (k*d), columns [rhs0_dx, rhs0_dy, rhs0_dz, rhs1_dx, ...]. */
int bbfmm_evaluate_with_gradients(bbfmm_handle *h, const double *w, int64_t rows, int32_t k,
                                  int64_t ldw, const double *x, int64_t m, int64_t ldx,
                                  double *out, int64_t ldo, double *grad, int64_t ldg,
                                  int64_t *bad_point_index);

/* FmmTree::evaluate_leaves (utils.rs:465-473 -> bbfmm.rs:537-544): leaf pass only,
 * after bbfmm_set_local_coefficients.
 * Extension for many small batches (isosurfacing, ferreus_rmt/src/isosurface.rs:574,693): w may be
 * NULL in the two leaves-only entry points; the weights already resident on the device (those of
 * the last call that took weights, normally bbfmm_set_local_coefficients) are used and the N x k
 * host-to-device copy per call is skipped.  k must still equal the set_weights column count. */
int bbfmm_evaluate_leaves(bbfmm_handle *h, const double *w, int64_t rows, int32_t k, int64_t ldw,
                          const double *x, int64_t m, int64_t ldx, double *out, int64_t ldo,
                          int64_t *bad_point_index);

/* FmmTree::evaluate_leaves_with_gradients (utils.rs:477-485 -> bbfmm.rs:560-567). */
int bbfmm_evaluate_leaves_with_gradients(bbfmm_handle *h, const double *w, int64_t rows, int32_t k,
                                         int64_t ldw, const double *x, int64_t m, int64_t ldx,
                                         double *out, int64_t ldo, double *grad, int64_t ldg,
                                         int64_t *bad_point_index);

/* ---- Isosurfaces: dense marching tetrahedra on the RMT sampling lattice (ferreus_rmt build_isosurface with
 * ClusterMethod::None, or with the *_ex entries and BBFMM_CLUSTER_AVERAGE / BBFMM_CLUSTER_CURVATURE its
 * ClusterMethod::Average / CurvatureWeighted; the raw mesh
 * before clipping and cleaning, or with the *_opts entries and BBFMM_FINISH_CLIPPED the mesh clipped to the extents and
 * cleaned on the device, which is the reference's finished mesh for BoundaryClosure::None; its self-intersection
 * rollback is run with BBFMM_SELF_INTERSECTIONS_ROLLBACK in the options.  Boundary closure (ClosePositive /
 * CloseNegative) is not implemented; contract in DESIGN.md
 * "Isosurfaces on the RMT lattice").  extents = [min x, min y, min z, max x, max y, max z]; resolution > 0.  Lattice fields are arrays of
 * nk x nj x ni doubles (i fastest) over the bounding box of the extraction nodes E; entries off E are ignored (NaN in
 * returned fields).  Vertices are n x 3 doubles, facets m x 3 int64 vertex ids, both row-major. */
typedef struct bbfmm_isosurface_result bbfmm_isosurface_result; /* the meshes of one call, one per isovalue */

/* The reference's tables as the product holds them: EDGE_DELTAS (14 x 3), REVERSE_EDGE (14), OWNED_TET_EDGES (6 x 3),
 * TET_EDGE_PAIRS (6 x 2), MT_TABLE (16 x 7: triangle count, then up to 2 triangles of 3 tet-edge ids, -1 padded). */
int bbfmm_isosurface_tables(int32_t *edge_deltas, int32_t *reverse_edge, int32_t *owned_tet_edges,
                            int32_t *tet_edge_pairs, int32_t *mt_table);
/* Host only (any handle, also BBFMM_FLAG_HOST_ONLY; h may be NULL, then without a message).  info_out[11]: max_ijk[3],
 * number of keys, number of nodes of E, ijk of field entry 0 (3), ni, nj, nk. */
int bbfmm_isosurface_lattice(bbfmm_handle *h, const double *extents, double resolution, int64_t *info_out);
/* Meshes of the handle's field (after bbfmm_set_local_coefficients with one column; d = 3) at n_isovalues isovalues
 * that share one evaluation of the field, on the handle's stream (a device group: on its primary part).  drift: NULL or
 * [a, b0, b1, b2], a + b . x added to the field.  d_field_out: NULL or a device array of nk x nj x ni doubles that
 * receives the field.  batch_bytes: device memory for one batch of k-planes (<= 0: a default).  A node outside the tree:
 * BBFMM_POINT_OUTSIDE_TREE before any work.  *out is set on success (free with bbfmm_isosurface_destroy). */
int bbfmm_build_isosurfaces(bbfmm_handle *h, const double *extents, double resolution, const double *isovalues,
                            int32_t n_isovalues, const double *drift, double *d_field_out, int64_t batch_bytes,
                            bbfmm_isosurface_result **out);
/* The same from a caller's host field (nk x nj x ni doubles).  h NULL: the current device and a stream of the call's
 * own; the message of a failure is then in *out (bbfmm_isosurface_error), which is set whenever out is not NULL. */
int bbfmm_isosurfaces_from_values(bbfmm_handle *h, const double *values, const double *extents, double resolution,
                                  const double *isovalues, int32_t n_isovalues, int64_t batch_bytes,
                                  bbfmm_isosurface_result **out);
/* Vertex clustering.  BBFMM_CLUSTER_NONE: one vertex per crossed lattice edge (the entries above).
 * BBFMM_CLUSTER_AVERAGE: the intersections near a sample point are merged into their mean where the topology tests of
 * ferreus_rmt allow it (topology.rs:232-314), then clusters that give a mesh edge more than 2 faces are split again
 * (isosurface.rs:798-930); the self-intersection rollback of the reference (isosurface.rs:932-1007) is run by the *_opts
 * entries with self_intersections = BBFMM_SELF_INTERSECTIONS_ROLLBACK and not otherwise.  The whole lattice field then
 * stays on the device (40 bytes per node of the nk x nj x ni box); a lattice that does not fit is refused before any
 * work with BBFMM_BAD_ARGUMENT.  The meshes do not depend on batch_bytes. */
#define BBFMM_CLUSTER_NONE 0
#define BBFMM_CLUSTER_AVERAGE 1
/* BBFMM_CLUSTER_CURVATURE: ClusterMethod::CurvatureWeighted, the method the reference's interpolator always uses
 * (rbf.rs:1054-1064).  Clusters, facets and the counts above are those of BBFMM_CLUSTER_AVERAGE; the point of every
 * cluster, those of one edge too, is the sum of w * p over its intersections in ascending edge order times 1 / sum of w
 * (curvature_weighting.rs:242-276), w the curvature weight of the crossed edge (curvature_weighting.rs:48-234) from the
 * field at the 14 neighbours of the edge's owner, 1 where that stencil is incomplete (a neighbour outside the extraction
 * nodes, not evaluated or not finite) or degenerate; a sum of w of 1e-12 or less gives the point of
 * BBFMM_CLUSTER_AVERAGE.  The weights are computed on the device once per isovalue.  The device's trigonometric functions
 * differ from a host's in their last bits, so vertices agree with a host computation to some 1e-13 of the resolution, not
 * bit for bit; facets are exact.  48 bytes per node of the box and 8 per crossed edge stay on the device. */
#define BBFMM_CLUSTER_CURVATURE 2
int bbfmm_build_isosurfaces_ex(bbfmm_handle *h, const double *extents, double resolution, const double *isovalues,
                               int32_t n_isovalues, const double *drift, double *d_field_out, int64_t batch_bytes,
                               int32_t cluster_method, bbfmm_isosurface_result **out);
int bbfmm_isosurfaces_from_values_ex(bbfmm_handle *h, const double *values, const double *extents, double resolution,
                                     const double *isovalues, int32_t n_isovalues, int64_t batch_bytes,
                                     int32_t cluster_method, bbfmm_isosurface_result **out);
/* The clustering counts of mesh i, stats_out[16] (all 0 with BBFMM_CLUSTER_NONE): sample points per topology case
 * [closed, multi-hole, flat-hole, multi-surface, simple, incomplete (a neighbour outside the extraction nodes: not
 * clustered)]; [6] mesh edges with more than 2 faces before pass A, [7] clusters pass A split; [8..12) sample points
 * rolled back in rounds 1..4 of pass B, [12..16) mesh edges with more than 2 faces those rounds found. */
int bbfmm_isosurface_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out);
/* The counts of BBFMM_CLUSTER_CURVATURE for mesh i, stats_out[4] (all 0 with the other methods): crossed edges weighted,
 * of those the edges with the fallback weight 1, clusters placed (the vertices before the clip), of those the clusters
 * whose weights summed to 1e-12 or less. */
int bbfmm_isosurface_curvature_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out);
/* Finishing.  BBFMM_FINISH_RAW: the marching-tetrahedra mesh as it is (the entries above): it reaches two lattice cells
 * past the extents and ends in open triangles there.  BBFMM_FINISH_CLIPPED: clip_mesh_to_aabb (aabb_clipping.rs:55-105)
 * and clean_mesh (mesh_cleanup.rs:32-96) of ferreus_rmt run on the device before the one download, with
 * eps = 1e-10 * max(|hi - lo|, 1): every facet clipped against the six planes of the extents and fanned, then vertices
 * within eps welded (the representative of a group is its lowest-index vertex), collapsed, zero-area, repeated and
 * lone facets dropped, and vertices renumbered in order of first use.  A mesh of more than 2^26 facets is refused
 * before any work (ids are packed in 32 bits).  BBFMM_FINISH_CLOSE_POSITIVE / BBFMM_FINISH_CLOSE_NEGATIVE: the clipped
 * mesh closed on the six faces of the extents (the reference's BoundaryClosure::ClosePositive / CloseNegative,
 * boundary_closure.rs; contract: DESIGN.md "Boundary closure"): its facets first (reversed for NEGATIVE), then per face
 * the cap facets wound outward, on a grid of the call's resolution; the new vertices follow the mesh's in order of first
 * use.  POSITIVE keeps the part of the faces where the field outside the extents counts as above the isovalue, NEGATIVE
 * the rest.  A mesh without open edges is returned as it is; one with an open edge off the faces is refused. */
#define BBFMM_FINISH_RAW 0
#define BBFMM_FINISH_CLIPPED 1
#define BBFMM_FINISH_CLOSE_POSITIVE 2
#define BBFMM_FINISH_CLOSE_NEGATIVE 3
/* Self-intersections.  BBFMM_SELF_INTERSECTIONS_IGNORE: the clustered mesh as the two passes above leave it (averaging can
 * pull two sheets of a complex surface through each other).  BBFMM_SELF_INTERSECTIONS_ROLLBACK, with
 * BBFMM_CLUSTER_AVERAGE or BBFMM_CLUSTER_CURVATURE (nothing is done with BBFMM_CLUSTER_NONE: the mesh and the counts are those without it): after
 * pass B and before the clip, one round of the reference's third guard.  The triangles on true self-intersections
 * (is_true_self_intersection, mesh_intersections.rs:125-159) among the facets with every corner inside the extents are
 * found on the device, by a uniform grid over the facets' bounding boxes instead of an R-tree; their vertices that are
 * clusters of several lattice edges send the sample points that own them back to one vertex per edge, and the mesh is
 * marched again.  Nothing found: the mesh is bit for bit the one without the option.  A mesh of more than 2^26 facets is
 * refused. */
#define BBFMM_SELF_INTERSECTIONS_IGNORE 0
#define BBFMM_SELF_INTERSECTIONS_ROLLBACK 1
/* Where the field is evaluated.  BBFMM_FOLLOW_DENSE: at every node of E (the entries above).  BBFMM_FOLLOW_SURFACE: only
 * in the bricks of B x B x B lattice nodes (B from the environment variable BBFMM_ISO_BRICK: 4, 8 or 16, default 8, read
 * per call) that a wavefront reaches from the seeds, as ferreus_rmt follows the surface from its seed points
 * (seed_projection.rs:29-130, isosurface.rs:551-697): seeds are clamped to the extents, kept one per lattice cell and,
 * with a handle's field, moved onto the level set by at most 30 Newton steps (gradients from the leaf pass, or central
 * differences for a kernel without them, or with BBFMM_ISO_SEED_GRADIENTS=differences in the environment); the bricks
 * that hold the 8 corners of their cells are evaluated, and every lattice edge with both ends
 * known and on opposite sides of the isovalue sends the wavefront into every brick within (4, 2, 2) nodes in (i, j, k) of
 * its ends, until nothing new is reached.  The mesh of an isovalue is the dense extraction, with every option above, of
 * the field that is NaN outside the bricks visited for it: every surface component that passes through a seed's cell is
 * complete and bit for bit that of BBFMM_FOLLOW_DENSE on the same values, a component no seed reaches is
 * absent, and no seeds give empty meshes.  A returned field is NaN where it was not evaluated.  The field array over the
 * box stays on the device (8 bytes per node, 16 with several isovalues, beside what clustering keeps); a lattice that does
 * not fit is refused before any work.  seeds: n_seeds points, coordinate a of seed s at seeds[a * seeds_ld + s]; NULL with
 * a handle's field: the handle's source points (rbf.rs:1049); a caller's values need seeds, which are then not moved. */
#define BBFMM_FOLLOW_DENSE 0
#define BBFMM_FOLLOW_SURFACE 1
/* Options of the *_opts entries.  size: sizeof(bbfmm_isosurface_options) as the caller was compiled; fields beyond it
 * take their defaults (CLUSTER_NONE, FINISH_RAW, batch_bytes 0, SELF_INTERSECTIONS_IGNORE, FOLLOW_DENSE, no seeds), as
 * does every field with options == NULL. */
struct bbfmm_interpolant_terms; /* below: "The interpolant around the tree" */
typedef struct bbfmm_isosurface_options {
    int64_t size;
    int32_t cluster_method; /* BBFMM_CLUSTER_* */
    int32_t finish;         /* BBFMM_FINISH_* */
    int64_t batch_bytes;    /* device memory for one batch of k-planes (<= 0: a default) */
    int32_t self_intersections; /* BBFMM_SELF_INTERSECTIONS_* */
    int32_t follow;         /* BBFMM_FOLLOW_*; read only where size covers seeds_ld too (it lies in the former padding) */
    const double *seeds;    /* host, n_seeds x 3 column-major with leading dimension seeds_ld, or NULL */
    int64_t n_seeds;
    int64_t seeds_ld;
    /* The field terms of an interpolant (read only where size covers the pointer; NULL: none), d = 3 and k = 1: the
     * polynomial of any degree -1 .. 2 on (x - translation) / scale, evaluated at the WORLD point of every lattice node and
     * seed, and a global trend's (B, b): the tree is asked at x B + b.  The clamp, the lattice and the whole extraction
     * stay in world coordinates; the check that every node lies in the tree's cube tests the transformed corners of the
     * lattice box (rbf.rs:599-613).  The seed projection's gradient is the tree's times B^T plus the polynomial's.  With
     * a trend the seeds must be given (the tree's own points are the transformed ones).  Giving both these terms and the
     * `drift` argument is BBFMM_BAD_ARGUMENT; the 4-value drift keeps its meaning.  On a BBFMM_FLAG_DETERMINISTIC handle
     * the field with terms is evaluated with a fixed split of every leaf's targets (64 per pass in 8 source slices instead
     * of the split sized to their number), so a node's value is the same double in the dense and the followed pass and
     * follow = surface gives the dense mesh bit for bit; what the fixed split costs on a large lattice is not measured.
     * A default handle keeps the tuned split (its f64 atomics rule the property out anyway). */
    const struct bbfmm_interpolant_terms *terms;
} bbfmm_isosurface_options;
/* The counts of BBFMM_FOLLOW_SURFACE for mesh i, stats_out[8] (all 0 with BBFMM_FOLLOW_DENSE): seeds given, distinct seed
 * cells, Newton steps run, seed bricks, rounds, bricks visited, nodes evaluated for this isovalue, nodes of E. */
int bbfmm_isosurface_follow_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out);
/* The bricks visited for mesh i: dims_out[4] = B and the number of bricks along x, y and z (all 0 with BBFMM_FOLLOW_DENSE);
 * bricks_out: NULL, or that many bytes (x fastest), 1 for a visited brick. */
int bbfmm_isosurface_follow_bricks(const bbfmm_isosurface_result *r, int32_t i, int32_t *dims_out, uint8_t *bricks_out);
/* Host wall time of its stages in milliseconds, ms_out[3]: seed stage, rounds of the wavefront, extraction. */
int bbfmm_isosurface_follow_times(const bbfmm_isosurface_result *r, int32_t i, double *ms_out);
int bbfmm_build_isosurfaces_opts(bbfmm_handle *h, const double *extents, double resolution, const double *isovalues,
                                 int32_t n_isovalues, const double *drift, double *d_field_out,
                                 const bbfmm_isosurface_options *options, bbfmm_isosurface_result **out);
int bbfmm_isosurfaces_from_values_opts(bbfmm_handle *h, const double *values, const double *extents, double resolution,
                                       const double *isovalues, int32_t n_isovalues,
                                       const bbfmm_isosurface_options *options, bbfmm_isosurface_result **out);

/* ---- Isosurfaces of any field (ferreus_rmt::build_isosurface with its surface_fn; DESIGN.md "Composite fields").
 * A composite field is evaluated on the device from up to 8 operands and one postfix program of at most 64 int32 codes
 * on a stack at most 8 deep.  An operand gives a value v and a gradient at a world point x:
 *   BBFMM_FIELD_MODEL:  the interpolant of a d = 3 handle (after bbfmm_set_local_coefficients, one column) with its
 *                       optional terms (d = 3, k = 1): exactly the field bbfmm_build_isosurfaces_opts evaluates for that
 *                       handle and those terms (trend map, leaf pass, terms kernel; the fixed split of every leaf's
 *                       targets with terms on a BBFMM_FLAG_DETERMINISTIC handle);
 *   BBFMM_FIELD_HEIGHT: x[axis] - g(u, v), (u, v) the other two coordinates in ascending axis order and g the
 *                       interpolant of a d = 2 handle with its optional terms (d = 2, k = 1); the gradient is e_axis
 *                       minus grad g on the other two axes;
 *   BBFMM_FIELD_AFFINE: affine[0] + affine[1] x0 + affine[2] x1 + affine[3] x2, summed left to right; no handle.
 * What an operand pushes is scale * v + offset (one multiply, then one add, never fused) with the gradient scale * grad v.
 * Program codes: >= 0 pushes that operand; BBFMM_FIELD_OP_MAX and _MIN pop b, then a, and push a >= b ? a : b and
 * a <= b ? a : b (not fmax / fmin: a tie keeps a with its sign of zero, a NaN gives b), the gradient travelling with
 * the value chosen; BBFMM_FIELD_OP_NEG negates both.  A valid program leaves exactly one entry.  Everything is checked
 * on the host before any device work (BBFMM_BAD_ARGUMENT, the message names the operand or the program position):
 * stack underflow or depth, unknown codes, operand ids, the entries left, non-finite scale / offset / affine, a handle
 * of the wrong dimension, without local coefficients for one column, host-only, a device group, or on another device
 * than the first, more than 8 operands or 64 codes. */
#define BBFMM_FIELD_MODEL 0
#define BBFMM_FIELD_HEIGHT 1
#define BBFMM_FIELD_AFFINE 2
#define BBFMM_FIELD_OP_MAX (-1)
#define BBFMM_FIELD_OP_MIN (-2)
#define BBFMM_FIELD_OP_NEG (-3)
typedef struct bbfmm_field_operand {
    int64_t size;          /* sizeof(bbfmm_field_operand) as the caller was compiled */
    int32_t kind;          /* BBFMM_FIELD_* */
    int32_t axis;          /* BBFMM_FIELD_HEIGHT: 0 .. 2 */
    bbfmm_handle *handle;  /* MODEL: d = 3, HEIGHT: d = 2, AFFINE: NULL */
    const struct bbfmm_interpolant_terms *terms; /* of that handle's interpolant, or NULL */
    double scale, offset;
    double affine[4];      /* BBFMM_FIELD_AFFINE */
} bbfmm_field_operand;
/* Meshes of the composite field, with every option of bbfmm_isosurface_options except terms (NULL here: terms belong to
 * operands) and the accessors above.  BBFMM_FOLLOW_SURFACE needs the seeds.  Before any evaluation the lattice box is
 * tested against every MODEL operand's cube (through its trend's transformed corners) and on its two axes against every
 * HEIGHT operand's square: BBFMM_POINT_OUTSIDE_TREE naming the operand.  The extraction runs on the stream of the first
 * operand with a handle (one of the call's own without any); every tree evaluates on its own stream and returns
 * synchronised, the affine, height and program kernels run on the extraction's stream.  The seed projection takes the
 * composite gradient when every tree operand's kernel has gradients and BBFMM_ISO_SEED_GRADIENTS is not `differences`,
 * else central differences of the composite value.  d_field_out as for bbfmm_build_isosurfaces.  *out is set whenever out
 * is not NULL and holds the message of a failure (bbfmm_isosurface_error). */
int bbfmm_isosurfaces_from_fields_opts(const bbfmm_field_operand *operands, int32_t n_operands, const int32_t *program,
                                       int32_t n_program, const double *extents, double resolution, const double *isovalues,
                                       int32_t n_isovalues, double *d_field_out, const bbfmm_isosurface_options *options,
                                       bbfmm_isosurface_result **out);
/* Meshes of a caller's function.  x: m points, coordinate a of point t at x[a * ldx + t]; values: m doubles; gradients:
 * component a of point t at gradients[a * ldg + t].  All host arrays; nonzero is failure and ends the extraction with
 * BBFMM_CALLBACK_FAILED.  Every batch of lattice nodes is downloaded, handed over and its values uploaded, on the current
 * device and a stream of the call's own.  gradient NULL: the seed projection of BBFMM_FOLLOW_SURFACE (seeds required)
 * takes central differences of `field`.  *out is set whenever out is not NULL and holds the message of a failure. */
typedef int (*bbfmm_field_fn)(const double *x, int64_t m, int64_t ldx, double *values, void *user);
typedef int (*bbfmm_gradient_fn)(const double *x, int64_t m, int64_t ldx, double *values, double *gradients, int64_t ldg, void *user);
int bbfmm_isosurfaces_from_function_opts(bbfmm_field_fn field, bbfmm_gradient_fn gradient, void *user, const double *extents,
                                         double resolution, const double *isovalues, int32_t n_isovalues,
                                         const bbfmm_isosurface_options *options, bbfmm_isosurface_result **out);
/* The composite field at m host points (coordinate a of point t at x[a * ldx + t]) through the path of the extraction's
 * FieldFn / GradFn: upload, every tree operand's check of the points (BBFMM_POINT_OUTSIDE_TREE), one column per operand,
 * the program kernel, download.  values: m doubles; gradients: NULL, or component a of point t at gradients[a * ldg + t]
 * (BBFMM_KERNEL_NO_GRADIENTS where a tree operand's kernel has none).  The message of a failure is bbfmm_last_error of
 * the first operand that has a handle. */
int bbfmm_debug_evaluate_fields(const bbfmm_field_operand *operands, int32_t n_operands, const int32_t *program, int32_t n_program,
                                const double *x, int64_t m, int64_t ldx, double *values, double *gradients, int64_t ldg);
/* The program alone on caller columns, on the host (where = 0) or the device (where = 1), one __host__ __device__
 * definition behind both (csrc/field_program.hpp).  V: m x n_operands, G: NULL or m x 3 n_operands (operand o, axis a at
 * column 3 o + a), packed column-major; out_v: m; out_g (with G): m x 3.  scale, offset: n_operands each. */
int bbfmm_debug_field_program(int32_t where, int32_t n_operands, const double *scale, const double *offset, const int32_t *program,
                              int32_t n_program, const double *V, const double *G, int64_t m, double *out_v, double *out_g);

/* BBFMM_FINISH_CLIPPED of a caller's own mesh (host arrays: n_vertices x 3 doubles, n_facets x 3 int64 ids) on the
 * current device, or the handle's when h is not NULL: *out holds one mesh.  Messages as for
 * bbfmm_isosurfaces_from_values. */
int bbfmm_isosurface_finish_mesh(bbfmm_handle *h, const double *vertices, int64_t n_vertices, const int64_t *facets,
                                 int64_t n_facets, const double *extents, bbfmm_isosurface_result **out);
/* The finishing counts of mesh i, stats_out[10] (all 0 with BBFMM_FINISH_RAW): [0] facets clipped, [1] of those kept
 * with a corner outside the extents, [2] dropped by the clip; [3] vertices the clip emitted, [4] of those welded into
 * another, [5] vertices further than eps from their representative (weld_loose; 0 where the weld is the reference's
 * greedy one); facets dropped as [6] collapsed, [7] zero-area, [8] repeated, [9] lone. */
int bbfmm_isosurface_finish_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out);
/* The boundary closure alone of a caller's own clipped and cleaned mesh (host arrays as for
 * bbfmm_isosurface_finish_mesh) on the current device, or the handle's when h is not NULL: *out holds one mesh.  mode:
 * BBFMM_FINISH_CLOSE_POSITIVE or BBFMM_FINISH_CLOSE_NEGATIVE; resolution: the spacing of the cap grid. */
int bbfmm_isosurface_close_mesh(bbfmm_handle *h, const double *vertices, int64_t n_vertices, const int64_t *facets,
                                int64_t n_facets, const double *extents, double resolution, int32_t mode,
                                bbfmm_isosurface_result **out);
/* The closure counts of mesh i, stats_out[BBFMM_CLOSURE_STATS] (all 0 where no closure ran).  Faces in the order XMin,
 * XMax, YMin, YMax, ZMin, ZMax. */
#define BBFMM_CLOSURE_OPEN_EDGES 0      /* [0, 6) open edges per face (one on a box edge counts on both faces) */
#define BBFMM_CLOSURE_OPEN_OFF_BOX 6    /* open edges with an end on no common face (the call is then refused) */
#define BBFMM_CLOSURE_CUT_CELLS 7       /* [7, 13) cut cells per face */
#define BBFMM_CLOSURE_WHOLE_KEPT 13     /* [13, 19) whole cells kept per face */
#define BBFMM_CLOSURE_REGIONS 19        /* connected components of whole cells */
#define BBFMM_CLOSURE_BAND_POINTS 20    /* points the host triangulated, summed over the faces */
#define BBFMM_CLOSURE_BAND_KEPT 21      /* band triangles in the output */
#define BBFMM_CLOSURE_BAND_DROPPED 22   /* band triangles of non-positive area (0 for a valid triangulation) */
#define BBFMM_CLOSURE_CONSTRAINT_FLIPS 23
#define BBFMM_CLOSURE_LAWSON_FLIPS 24
#define BBFMM_CLOSURE_VERTICES_ADDED 25
#define BBFMM_CLOSURE_CONFLICTS 26      /* seeded components that also border the unseeded side of an open edge */
#define BBFMM_CLOSURE_BAND_HOST_US 27   /* host time of the band triangulation and the selection, microseconds */
#define BBFMM_CLOSURE_STATS 32
int bbfmm_isosurface_closure_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out);
/* Host only: the band triangulator of the closure on one face (csrc/closure_triangulate.hpp).  gu, gv: the nu + 1 and
 * nv + 1 grid coordinates; points: n_points x 2 (the mesh vertices on the face); edges: n_edges x 2 point indices (the
 * open edges); cut: n_cut cut cells (v * nu + u, ascending); tol: 1e-9 * resolution; key_cell: max(eps, 1e-12).
 * Receives the band points (pts_out: 2 per point, ids_out: the index of a mesh point, or -1 - (gv_index * (nu + 1) +
 * gu_index) for a grid point; at most cap_points) and the triangles, counter-clockwise (tris_out: 3 band point
 * indices each; at most cap_tris).  counts_out[8]: [0] band points, [1] triangles, [2] triangles dropped as
 * non-positive, [3] constraint flips, [4] Lawson flips.  BBFMM_BAD_ARGUMENT with a message in err_out (err_cap bytes)
 * for constraints that cannot be met (two open edges that cross) or too small capacities. */
int bbfmm_debug_closure_triangulate(int32_t nu, int32_t nv, const double *gu, const double *gv, const double *points,
                                    int64_t n_points, const int64_t *edges, int64_t n_edges, const int32_t *cut,
                                    int64_t n_cut, double tol, double key_cell, int64_t cap_points, double *pts_out,
                                    int64_t *ids_out, int64_t cap_tris, int64_t *tris_out, int64_t *counts_out,
                                    char *err_out, int64_t err_cap);
/* Host only: the exact sign of the orientation determinant of n triples of points in the plane (abc: 6 doubles per
 * triple: a, b, c), the predicate of that triangulator: sign_out[i] in {-1, 0, 1}, 1 for counter-clockwise. */
int bbfmm_debug_orient2d(const double *abc, int64_t n, int32_t *sign_out);
/* The counts of the self-intersection detector for mesh i, stats_out[8] (all 0 where it did not run): [0] facets with
 * every corner inside the extents, [1] pairs of those with overlapping bounding boxes, [2] of those, pairs the Moeller
 * test accepts, [3] of those, true self-intersections, [4] triangles on a true pair, [5] their vertices that are clusters
 * of several lattice edges, [6] sample points rolled back, [7] 0 (reserved). */
int bbfmm_isosurface_intersection_stats(const bbfmm_isosurface_result *r, int32_t i, int64_t *stats_out);
/* The detector on a caller's own mesh (host arrays as for bbfmm_isosurface_finish_mesh, finite vertices) on the current
 * device, or the handle's when h is not NULL: *out holds one entry without vertices or facets, whose
 * bbfmm_isosurface_intersection_ids are the triangles on true self-intersections in ascending order (the reference's
 * get_intersecting_triangles) and whose bbfmm_isosurface_intersection_stats are [0..4] above.  extents: only facets with
 * every corner inside them (slack 1e-10 * max(|hi - lo|, 1)) take part; NULL: all facets.  The search probes a grid of
 * the largest facet's bounding box: a mesh on which that is quadratic (a huge triangle among many small ones; more than
 * max(2^26, 4096 * facets) candidates) is refused with BBFMM_BAD_ARGUMENT before any pair is tested. */
int bbfmm_isosurface_self_intersections(bbfmm_handle *h, const double *vertices, int64_t n_vertices, const int64_t *facets,
                                        int64_t n_facets, const double *extents, bbfmm_isosurface_result **out);
/* n_ids_out (may be NULL): the number of ids of entry i; ids_out (may be NULL): receives them. */
int bbfmm_isosurface_intersection_ids(const bbfmm_isosurface_result *r, int32_t i, int64_t *n_ids_out, int64_t *ids_out);
/* Host only: the pair predicate the device runs (is_true_self_intersection with the reference's constants: tolerance
 * 1e-8, Moeller epsilon 1e-6 on unnormalised normals, so it depends on the scale of the triangles).  tri_a, tri_b: 9
 * doubles each, ids_a, ids_b: their 3 vertex ids; a is the facet with the lower index (the predicate is not symmetric in
 * its last bits).  result_out: 1 for a true self-intersection.  stage_out (may be NULL), the test that decided: 0 a
 * degenerate triangle, 1 two or more shared ids, 2 the Moeller test, 3 one shared id: the crossing test, 4 coincident
 * vertices under distinct ids (two or more: no; one: the crossing test), 5 nearly coplanar, 6 a true self-intersection. */
int bbfmm_isosurface_triangle_pair(const double *tri_a, const int64_t *ids_a, const double *tri_b, const int64_t *ids_b,
                                   int32_t *result_out, int32_t *stage_out);
/* Host only: the clip of one triangle (9 doubles) by the function the device runs.  points_out: up to 12 x 3 doubles,
 * corner_out (may be NULL): per point the corner of the triangle it is a kept copy of, -1 for a point made on a plane;
 * n_points_out: 0 when the triangle is dropped. */
int bbfmm_isosurface_clip_triangle(const double *triangle, const double *extents, double *points_out,
                                   int32_t *corner_out, int32_t *n_points_out);
/* Host only: the topology test the device runs, for one 14-bit near mask.  neighbour_values: f - isovalue at the 14
 * neighbours (EDGE_DELTAS order), or NULL to leave out the flat-hole test.  case_out: 0 closed, 1 multi-hole, 2 flat-hole,
 * 3 multi-surface, 4 simple.  cluster_of_edge[14]: the lowest edge of the cluster of each edge, -1 off the mask. */
int bbfmm_isosurface_topology(uint32_t near_mask, const double *neighbour_values, int32_t *case_out,
                              int32_t *cluster_of_edge);
/* The clustering tables as the product holds them: NEIGHBOUR_MASKS (14), FLAT_HOLE_MASKS (36 x 2), ALL14_MASK. */
int bbfmm_isosurface_cluster_tables(int32_t *neighbour_masks, int32_t *flat_hole_masks, int32_t *all14_mask);
/* The curvature-weighting tables as the product holds them: rows 0..6 of NEIGHBOUR_EDGE_PLANE_PAIRS (7 x 3 x 2 edge
 * labels, an unused third plane -1) and of NEIGHBOUR_EDGE_PLANE_PHIS (7 x 3 x 2: 1 for PHI_1, 2 for PHI_2, -1 unused);
 * constants[5]: PHI_1, PHI_2, EPS, MAX_COT_THETA, MAX_CURVATURE_WEIGHT. */
int bbfmm_isosurface_curvature_tables(int32_t *plane_pairs, int32_t *plane_phis, double *constants);
/* Host only: the weight function the device runs (curvature_weight_for_edge, curvature_weighting.rs:48-234), for the
 * owned edge `label` (0..6) of the sample point owner_ijk[3] on the lattice world(ijk) = lo_world + ijk * spacing.
 * values[15]: f - isovalue at the owner, then at its 14 neighbours (EDGE_DELTAS order), NaN for a missing one.
 * weight_out: the weight, 1 where the reference gives None; fallback_out (may be NULL): 1 in that case. */
int bbfmm_isosurface_curvature_weight(const double *values, const int64_t *owner_ijk, int32_t label, const double *lo_world,
                                      const double *spacing, double *weight_out, int32_t *fallback_out);
int32_t bbfmm_isosurface_count(const bbfmm_isosurface_result *r);
int bbfmm_isosurface_size(const bbfmm_isosurface_result *r, int32_t i, int64_t *n_vertices, int64_t *n_facets);
int bbfmm_isosurface_copy(const bbfmm_isosurface_result *r, int32_t i, double *vertices, int64_t *facets);
const char *bbfmm_isosurface_error(const bbfmm_isosurface_result *r);
void bbfmm_isosurface_destroy(bbfmm_isosurface_result *r);

/* FmmTree::source_points (utils.rs:489-493): copies the N x d points to out (ld). */
int bbfmm_source_points(const bbfmm_handle *h, double *out, int64_t ld);

/*
 * The FGMRES matvec, ferreus_rbf/src/rbf.rs:1338-1379 (fast_matrix_vector_product):
 *   set_weights(w); y = evaluate(w, source_points[target_indices])
 *   result[i] = y + nugget*w[i] + P[i,:] * w[N..N+basis_size]   for i in target_indices,
 *   every other row of result (incl. the last basis_size rows) = 0.
 * w and result have N + basis_size rows, one column.  target_indices NULL -> all
 * N sources.  poly is N x basis_size column-major (ldp) or NULL.
 * Host buffers; the targets never leave the device (they are the sources).
 */
int bbfmm_fast_matrix_vector_product(bbfmm_handle *h, const double *w, int64_t rows,
                                     int64_t basis_size, const int64_t *target_indices,
                                     int64_t n_target_indices, const double *poly, int64_t ldp,
                                     double nugget, double *result);

/* Builds (and caches) what a later bbfmm_fast_matrix_vector_product with these target_indices needs -- the
 * sorted targets and the restricted downward pass -- without running a product; also allocates the
 * pinned staging buffer.  Optional: the first product with an index set does the same.  The Schwarz
 * preconditioner calls it for its levels at creation, so that setup cost does not land in the solve. */
int bbfmm_prepare_target_subset(bbfmm_handle *h, const int64_t *target_indices, int64_t n_target_indices);

/*
 * Device-resident form of the same product for the case target_indices = all,
 * basis_size = 0, nugget = 0 generalised to k right-hand sides:
 *   d_out[:, j] = K(X, X) d_w[:, j]      (set_weights + evaluate at the sources)
 * d_w / d_out are DEVICE pointers (N x k, ldw / ldo).  Asynchronous on the
 * handle's stream unless sync != 0.  This is what bench.py times.
 * Reproducibility: for ANY k (since round 4 also k > 1, and on partitioned handles) the near field runs the
 * unordered-pair kernels and M2P is fused with P2L; both accumulate with f64 atomics, so two runs agree to summation
 * order (<= 1e-12 relative), not bit for bit.  Handles created with BBFMM_FLAG_DETERMINISTIC (or a process with
 * BBFMM_P2P_SYM=0 in its environment: ordered pairs, separate P2L and M2P) keep a fixed order.  The same holds for
 * bbfmm_fast_matrix_vector_product, for bbfmm_evaluate on targets that are the sources, and for the
 * bbfmm_matvec_partition_* calls.
 */
int bbfmm_matvec_device(bbfmm_handle *h, const double *d_w, int64_t ldw, int32_t k, double *d_out,
                        int64_t ldo, int32_t sync);

/* IterativeSolver::matvec_partial (rbf.rs:119-133) on device-resident vectors, for callers that keep
 * their vectors in HBM between products (the Schwarz sweep, bbfmm_schwarz_apply).  An index set is
 * registered once -- sorted targets and restricted downward pass are built then and kept for the life
 * of the handle -- and named by the returned id afterwards (-1 is returned for "all rows in order").
 *   d_y[j] = sum_i phi(x_target_indices[j], x_i) * d_w[i],   j < n_target_indices
 * d_w: N values in the caller's point numbering, d_y: n_target_indices values (N for id -1), both DEVICE
 * pointers.  The nugget and polynomial terms of rbf.rs:1366-1376 are the caller's (they are O(n)).
 * Asynchronous on the handle's stream unless sync != 0. */
int bbfmm_target_subset_create(bbfmm_handle *h, const int64_t *target_indices, int64_t n_target_indices,
                               int32_t *subset_id);
int bbfmm_matvec_subset_device(bbfmm_handle *h, int32_t subset_id, const double *d_w, double *d_y, int32_t sync);

/* HIP stream the handle launches on (hipStream_t as void*), for event timing and for device work that has to
 * stay in order with the handle's.  A handle belongs to the HIP device that was current in bbfmm_create; every
 * entry point that takes the handle (this one included) makes that device current in the calling thread, so the
 * handle can be used from threads that never selected a device. */
void *bbfmm_stream(bbfmm_handle *h);

/* Multi-GPU target partition: restrict the downward + leaf pass of
 * bbfmm_matvec_device to the contiguous Morton range of target leaves owned by
 * `rank` of `world`; rows of d_out that this rank does not own are left
 * untouched.  The owned rows, in original point numbering, are reported by
 * bbfmm_partition_rows.  rank=0, world=1 restores the full evaluation. */
int bbfmm_set_partition(bbfmm_handle *h, int32_t rank, int32_t world);
int64_t bbfmm_partition_row_count(const bbfmm_handle *h);
int bbfmm_partition_rows(const bbfmm_handle *h, int64_t *rows_out);

/* The partitioned matvec in two calls, around the one exchange the upward pass needs (the passes
 * being split are ferreus_bbfmm/src/bbfmm.rs:666-772 and 444-507).  Every rank holds all weights but anterpolates
 * only its share: above a coarse level (4 for a uniform 10M-point tree) the cells it owns and the three-cell halo
 * its V / W lists read, complete; at and below it the partial sums over the sources it owns.  M2M is linear, so
 * one all-reduce (sum) of those partial coarse multipoles -- a contiguous prefix of M, 13 MB per right-hand side at
 * order 7 -- completes them on every rank.
 *   bbfmm_partition_coarse_count   doubles per right-hand side of that prefix (0: nothing to exchange, e.g. depth < 2)
 *   bbfmm_matvec_partition_upward  gather + this rank's P2M / M2M on the handle's stream; packs k x count partial
 *                                  multipoles rhs-major into d_coarse (device memory of the caller)
 *   -- caller: all-reduce (sum) d_coarse over the ranks, ordered after the handle's stream (RCCL on that stream, or
 *      any stream that waits for it) --
 *   bbfmm_matvec_partition_finish  takes the summed d_coarse, runs the downward and leaf passes of the owned
 *                                  targets, writes the owned rows of d_out (ld ldo) like bbfmm_matvec_device.
 * comm_stream (hipStream_t as void*, may be NULL): the stream the caller issues the all-reduce on.  _upward makes it wait
 * for the packed multipoles only and queues the near field (P2P) of the owned targets behind the pack on the handle's own
 * stream, so that the collective runs beside it; _finish makes the handle's stream wait for comm_stream before it reads
 * d_coarse.  With NULL the caller orders the collective after the handle's stream itself (everything serial).
 * bbfmm_matvec_device on a partitioned handle still works on its own (it then runs the whole upward pass).  After
 * _upward the handle's multipoles are this rank's share: bbfmm_evaluate* and bbfmm_set_local_coefficients return
 * BBFMM_BAD_ARGUMENT ("one partition's share") until bbfmm_set_weights or bbfmm_matvec_device has run a whole upward pass
 * (a device-group handle completes its first part's multipoles by itself). */
int64_t bbfmm_partition_coarse_count(const bbfmm_handle *h);
int bbfmm_matvec_partition_upward(bbfmm_handle *h, const double *d_w, int64_t ldw, int32_t k, double *d_coarse, void *comm_stream);
int bbfmm_matvec_partition_finish(bbfmm_handle *h, const double *d_coarse, double *d_out, int64_t ldo, int32_t sync, void *comm_stream);
/* The exchange of the owned potentials in the tree's sorted order (what distributed.py's PartitionedMatvec uses): a part
 * owns ONE range of the sorted points, so its potentials travel as one contiguous block and every rank writes the gathered
 * blocks to their rows in a single pass over the tree's permutation -- no index arrays on the caller's side.
 *   bbfmm_partition_world / _rank         parts of the handle's partition (1: none set) and the part it owns
 *   bbfmm_partition_bounds                world + 1 offsets: part r owns the sorted points bounds[r] .. bounds[r + 1)
 *                                         (the same on every rank; its own count is bounds[rank + 1] - bounds[rank]);
 *                                         `world` must be bbfmm_partition_world
 *   bbfmm_matvec_partition_finish_sorted  like _finish, but leaves the k x count owned potentials in d_seg (row stride
 *                                         ld >= count) instead of scattering them -- the block to all-gather
 *   bbfmm_partition_scatter               d_all[n_parts][k][m_max] = the gathered blocks of parts first_part ..
 *                                         first_part + n_parts (normally 0, world) -> their rows of d_out (k x N, row
 *                                         stride ldo); asynchronous on the handle's stream like the other calls */
int32_t bbfmm_partition_world(const bbfmm_handle *h);
int32_t bbfmm_partition_rank(const bbfmm_handle *h);
int bbfmm_partition_bounds(const bbfmm_handle *h, int32_t world, int64_t *bounds_out);
int bbfmm_matvec_partition_finish_sorted(bbfmm_handle *h, const double *d_coarse, double *d_seg, int64_t ld, void *comm_stream);
int bbfmm_partition_scatter(bbfmm_handle *h, const double *d_all, int32_t first_part, int32_t n_parts, int64_t m_max, int32_t k,
                            double *d_out, int64_t ldo);
/* Test hook (host side, also on BBFMM_FLAG_HOST_ONLY handles): walks this rank's upward plan with point COUNTS in
 * place of multipoles (P2M -> points of the leaf, M2M -> sum over the plan's children).  counts_out[c] (n_cells):
 * what the plan leaves in cell c before the exchange (-1: never written); reads_out[c] = 1 where the rank's downward
 * or leaf pass reads M_c.  info_out[0..3] = coarse level, coarse cells, leaves anterpolated, parents translated.
 * Summed over the ranks the coarse prefix must equal the true point counts, and every cell a rank reads above the
 * coarse level must hold its true count already. */
int bbfmm_debug_partition_upward_counts(const bbfmm_handle *h, int64_t *counts_out, uint8_t *reads_out, int64_t *info_out);

/* Host-side legs of the host-buffer entry points by themselves (scripts/host_buffer_legs.py; no device needed): n doubles
 * copied by the library's thread pool in 2 MB pieces, gathered through a random permutation, scattered through it.
 * out4 = {copy ms, gather ms, scatter ms, pool threads}. */
int bbfmm_debug_host_copy_rates(int64_t n, double *out4);

/* ---- introspection (tests, bench statistics; host side, no device needed) ---- */
typedef struct {
    int32_t d, order, n_nodes, depth;
    int64_t n_points, n_cells, n_leaves;
    int64_t n_u, n_v, n_w, n_x;              /* total list entries */
    int64_t p2p_pairs;                       /* sum_leaf n_t * sum_{U} n_s, targets = sources */
    int64_t p2p_tile_bytes_k1;               /* SURVEY.md 8(d) tile-traffic bytes at K=1 */
    double m2l_flops_k1;                     /* sum_pairs 4*n*r (2*n*n if uncompressed); shared basis: see m2l_basis_rank */
    double center[3];
    double radius;
    int64_t wx_pairs;                        /* sum over (leaf, W cell) of n_t * n: kernel evaluations of M2P (= of P2L) */
    int64_t wx_tile_bytes_k1;                /* tile traffic of M2P + P2L at K=1: per (leaf, W cell) n_t*(8d+8) + 2*n*8 */
    int32_t m2l_basis_rank;                  /* BBFMM_FLAG_M2L_SHARED_BASIS: largest rank of a level's basis (0: flag not set); */
    int32_t m2l_basis_len;                   /* coordinates kept per cell (rank padded to the kernel's column groups);      */
                                             /* m2l_flops_k1 then counts the stages in the basis + both changes of basis      */
    /* The intermediate of the two M2L stages (one slot of sum_t rank_t doubles per target cell; the reference holds
     * none, bbfmm.rs:864-986 multiplies pair by pair) is bounded: the levels -- or, for a level that alone exceeds the
     * budget, 2 / 4 / 8 groups of its target classes -- go through one buffer in `m2l_batches` passes, a few
     * right-hand sides at a time.  Budget: BBFMM_M2L_CBUF_MB (default: a sixteenth of the device's memory, 18 GiB on
     * MI355X, at least 4096). */
    int32_t m2l_batches;                     /* passes through the buffer per right-hand-side chunk                        */
    int32_t m2l_rhs_per_pass;                /* right-hand sides per pass (0 until weights were set)                        */
    int64_t m2l_slots_bytes_per_rhs;         /* all slots of one right-hand side (what an unbounded buffer would hold)      */
    int64_t m2l_intermediate_bytes;          /* bytes of the buffer actually allocated (0 until weights were set)           */
} bbfmm_tree_stats;

int bbfmm_get_tree_stats(const bbfmm_handle *h, bbfmm_tree_stats *out);
/* 1 when the source tree (linear_tree.rs:20-175: Morton codes, sort, subdivision, per-leaf point lists) was built
 * on the device, 0 when the host build ran (BBFMM_FLAG_HOST_ONLY, BBFMM_TREE_DEVICE=0, or a source point outside
 * the root box).  Both produce the same tree; tests compare them. */
int bbfmm_tree_built_on_device(const bbfmm_handle *h);

/* Cells in (level, key) order: Morton key (morton.rs:58-119), leaf flag. */
int bbfmm_get_cells(const bbfmm_handle *h, uint64_t *keys, uint8_t *is_leaf);
/* Source rows of every leaf: ptr has n_cells+1 entries, idx has n_points entries
 * (ascending inside a leaf, linear_tree.rs:55-66). */
int bbfmm_get_leaf_sources(const bbfmm_handle *h, int64_t *ptr, int64_t *idx);
/* which: 'U','V','W','X'.  ptr may be NULL to query the size; returns entries via *n_entries.
 * idx holds cell indices (positions in bbfmm_get_cells), sorted by key. */
int bbfmm_get_list(const bbfmm_handle *h, char which, int64_t *ptr, int32_t *idx,
                   int64_t *n_entries);
/* M2L operator ranks per (level, reference vector): ranks[level*n_ref + ref], levels
 * 0..depth (0 where no operator exists).  n_ref_out: 2/7/16 for d = 1/2/3. */
int bbfmm_get_m2l_ranks(const bbfmm_handle *h, int32_t *ranks, int32_t *n_ref_out);
/* Dense reconstruction U*Vt (n x n column-major) of one reference operator. */
int bbfmm_get_m2l_operator(const bbfmm_handle *h, int32_t level, int32_t ref, double *out);
/* The factors themselves: u is n x rank, vt is rank x n (both column-major; vt may be NULL,
 * and is not written for uncompressed operators where U is the n x n kernel block). */
int bbfmm_get_m2l_factors(const bbfmm_handle *h, int32_t level, int32_t ref, double *u, double *vt);
/* Symmetry tables (chebyshev.rs:486-585): perm / invperm are n_perm x n (row-major),
 * perm_lookup / ref_lookup have 7^d entries.  Any pointer may be NULL. */
int bbfmm_get_permutation_tables(const bbfmm_handle *h, int32_t *n_perm, int32_t *perm,
                                 int32_t *invperm, int32_t *perm_lookup, int32_t *ref_lookup);
/* Target -> leaf assignment (linear_tree.rs:487-520) for arbitrary points; cell_out
 * receives cell indices. */
int bbfmm_points_to_leaves(const bbfmm_handle *h, const double *x, int64_t m, int64_t ldx,
                           int32_t *cell_out, int64_t *bad_point_index);

/* Per-phase device time in milliseconds, accumulated since the last reset while profiling is
 * enabled.  hipEvent pairs are recorded on the handle's stream around each phase WITHOUT
 * synchronising (the timed kernels still run back to back); this call synchronises once and
 * resolves them.  count_out (optional) receives the number of recorded intervals per phase.
 * Order: gather, P2M, M2M, M2L_stage1, M2L_stage2, P2L, L2L, P2P, M2P, L2P, scatter. */
#define BBFMM_N_PHASES 11
int bbfmm_set_profiling(bbfmm_handle *h, int32_t enable);
int bbfmm_get_phase_ms(bbfmm_handle *h, double *ms_out, int64_t *count_out);
int bbfmm_reset_phase_ms(bbfmm_handle *h);

/* FP64 MFMA self-test + peak microbenchmark (device): returns measured TFLOP/s of
 * back-to-back v_mfma_f64_4x4x4 in *tflops and 0 mismatches in *layout_errors when
 * the lane layout assumed by the M2L kernels holds on this device.  info6 (optional, 6 doubles):
 * cycles/MFMA of a lone wave, its clock (MHz), cycles/MFMA/SIMD and clock with every CU busy at
 * 1 wave/SIMD, TFLOP/s at 1 and at 2 waves/SIMD. */
int bbfmm_mfma_f64_selftest(double *tflops, int32_t *layout_errors, double *info6);
/* FP64 vector-ALU microbenchmark (device): chip-wide v_fma_f64 rate in *tflops and the shader clock it ran at in
 * *clock_mhz -- the issue roofline of the pair kernels (P2P, M2P, P2L), which the FP64 load pulls under the nominal
 * 2.4 GHz. */
int bbfmm_fp64_valu_selftest(double *tflops, double *clock_mhz);

/* ---- test hooks (never reached from a compute entry point) ----
 * The kernel functions of csrc/kernels.hpp, element by element: for each r2[i] (a squared distance) value_out[i] is the
 * kernel value as the value passes compute it, value_g_out[i] / factor_out[i] the value and the scalar `factor`
 * (gradient = factor * (target - source)) as the gradient passes compute them.  where = 0: the host branch (libm and
 * IEEE division: what assembles the M2L operators) in a plain loop, no device needed; where = 1: the device branch (what
 * every P2P / M2P / P2L pair is evaluated with), one thread per element.  Arrays are host memory, n doubles each. */
int bbfmm_debug_kernel_values(int32_t where, int32_t kernel_id, double base_range, double total_sill, const double *r2,
                              int64_t n, double *value_out, double *value_g_out, double *factor_out);
/* The arithmetic primitives under them: which = 0 bb_sqrt, 1 bb_sqrt_rsqrt (sqrt in out, 1/sqrt in out2), 2 bb_rcp
 * (x > 0, finite), 3 bb_log (x > 0, normal).  out2 may be NULL.  where as above. */
int bbfmm_debug_math(int32_t where, int32_t which, const double *x, int64_t n, double *out, double *out2);

/* ---- test hooks (host loops, no device) ----
 * Dense n x n (column-major) M2M matrix of child `child_index` exactly as the reference
 * stores it (chebyshev.rs:216-240); the device applies the same operator sum-factorised. */
int bbfmm_debug_dense_m2m(const bbfmm_handle *h, int32_t child_index, double *out);
/* Applies the stacked per-class M2L tables (what the MFMA kernels consume) with plain host
 * loops: L[c][:] += M2L(M) for one rhs, M and L being n_cells x n cell-major.  Only valid on
 * BBFMM_FLAG_HOST_ONLY handles (the tables are released after upload otherwise). */
int bbfmm_debug_apply_m2l_tables_host(const bbfmm_handle *h, const double *M, double *L);
/* Number of stage-1 boundary variants (stacked operators with the transfer vectors towards missing targets left
 * out, fmm_m2l_tables.cpp build_m2l_tables) and of source cells that use one. */
int bbfmm_debug_m2l_variants(const bbfmm_handle *h, int64_t *n_variants, int64_t *n_cells);
int bbfmm_debug_m2l_pairs(const bbfmm_handle *h, int32_t *out, int64_t cap, int64_t *n_out, int32_t *pairs_on);
int bbfmm_debug_m2l_pairs_axes(const bbfmm_handle *h, int32_t *out, int64_t cap, int64_t *n_out);
int bbfmm_debug_m2l_pairs_stage2(const bbfmm_handle *h, int32_t *out, int64_t cap, int64_t *n_out, int32_t *pairs_on);
int bbfmm_debug_m2l_pairs_axes_stage2(const bbfmm_handle *h, int32_t *out, int64_t cap, int64_t *n_out);
/* The kernel instance stage 2 runs in the parity basis: out[6] = column groups per chunk of the x-even and of the x-odd half
 * (ga, gb), chunks per half (ce, co), and with two axes the groups of a chunk that belong to its y-even part (ya, yb; 0, 0
 * with one axis).  All zeros when the handle has no stage-2 pairs.  Made on the host: BBFMM_FLAG_HOST_ONLY handles answer. */
int bbfmm_debug_m2l_s2_plan(const bbfmm_handle *h, int32_t *out);
/* The W / X jobs of the resident target set (targets = sources): out[8] = the number of M2P jobs, of chunk jobs and of
 * whole-leaf jobs of the fused M2P + P2L pass; the largest row count of a chunk job and of a whole-leaf job; the largest
 * W-cell count of a chunk job, of a whole-leaf job and of an M2P job.  Planned on the host: BBFMM_FLAG_HOST_ONLY handles
 * answer (with the default count of compute units).  BBFMM_UNSUPPORTED if a handle with a device uploaded other counts. */
int bbfmm_debug_wx_jobs(const bbfmm_handle *h, int32_t *out);
/* One 64-bit FNV-1a digest per family of the integer M2L tables (FmmTree::debug_m2l_table_digests lists the families and
 * their order), for BBFMM_FLAG_HOST_ONLY handles: *n_out = number of families, digests (capacity cap, may be NULL)
 * receives the first min(cap, *n_out).  flops_level (capacity flops_cap, may be NULL) receives the M2L flop count of
 * every level, *n_levels_out (may be NULL) their number: sums in a fixed order, compared as values, not hashed. */
int bbfmm_debug_m2l_table_digests(const bbfmm_handle *h, uint64_t *digests, int32_t cap, int32_t *n_out, double *flops_level,
                                  int32_t flops_cap, int32_t *n_levels_out);
int bbfmm_debug_m2l_s2_last_ksplit(const bbfmm_handle *h, int32_t *ksplit); /* debug only */
/* The leaf passes over runs of leaves (BBFMM_LEAF_PASSES): counts[0] the handle's mask, counts[1] the runs of the resident
 * target set's job list, counts[2] its jobs outside every run, counts[3] all its jobs (0 runs: one leaf per wave). */
int bbfmm_debug_leaf_runs(const bbfmm_handle *h, int32_t *counts); /* debug only */
/* What a device group holds and has queued, for the tests that run its several-device paths on one device
 * (BBFMM_GROUP_OWN_COPIES=1 when the handle is created: every part keeps its own copy of the weights and data moves between
 * parts as between devices).  out (capacity cap >= 9 + parts): out[0] parts, out[1] the switch, out[2] the weight mirrors
 * the primary holds now (0 outside a staging), then counted since creation where the calls are queued: out[3] pieces of
 * staged weights sent to mirrors, out[4] peer copies, out[5] plain device copies between two parts, out[6] waits of a part
 * for the arrival of another part's copy of the weights, out[7] columns of device-resident weights copied to other parts
 * (each one also in out[4] or out[5]), out[8] 1 when the runtime refused a peer copy within one device and the plain copy
 * serves instead; out[9 + g] the part whose copy of the weights part g reads.  A plain handle: one part, zeros. */
int bbfmm_debug_group_state(const bbfmm_handle *h, int64_t *out, int64_t cap); /* debug only */

/* The Morton primitives of csrc/morton.hpp as the host tree build uses them (morton.rs:58-263; the
 * reference's byte lookup tables, morton_constants.rs:77-346, are replaced by bit arithmetic): checked
 * bit-exactly against the reference's own tables in tests/test_reference_tables.py.
 *   encode: anchor[d] (16 bits per axis are read) + level -> key;   decode: key -> anchor[d], level
 *   neighbours: same-level neighbour keys inside the root box, in the reference's direction order
 *               (morton_constants.rs:32-74); keys_out holds up to 26, the count is returned
 *   direction_vectors: out is n x d (row-major), n = 2 / 8 / 26 returned
 *   reference_vectors: the handle's M2L reference vectors (chebyshev.rs:272-294), n_ref x d row-major */
uint64_t bbfmm_debug_morton_encode(int32_t d, const uint64_t *anchor, uint64_t level);
void bbfmm_debug_morton_decode(int32_t d, uint64_t key, uint64_t *anchor_out, uint64_t *level_out);
int32_t bbfmm_debug_morton_neighbours(int32_t d, uint64_t key, uint64_t *keys_out);
int32_t bbfmm_debug_direction_vectors(int32_t d, int32_t *out);
int bbfmm_debug_reference_vectors(const bbfmm_handle *h, int32_t *out, int32_t *n_ref_out);

/* Copies the device-resident multipole ('M') or local ('L') coefficients of the last pass to
 * the host as k x n_cells x n (rhs-major, cell-major), i.e. column c + j*n_cells of the
 * reference's n x (C*K) matrices (bbfmm.rs:234-242).  Per-phase parity checks. */
int bbfmm_debug_get_coefficients(bbfmm_handle *h, char which, int32_t k, double *out);
/* 'P': the multipoles in stage 1's parity basis as the stage reads them, k x n_cells x len with the pads of every row;
 * len from bbfmm_debug_m2l_parity_len (0: the handle keeps none).  Debug only. */
int bbfmm_debug_m2l_parity_len(const bbfmm_handle *h, int32_t *len);

/* ------------------------------------------------------------------ iterative solvers
 * ferreus_rbf/src/iterative_solvers.rs: host FGMRES / stationary Schwarz
 * drivers around operator callbacks, so the reference's closures (`matvec`, `precon`,
 * rbf.rs:523-524) plug in unchanged.  Vectors are host arrays of n doubles. */

/* y = Op(x); return BBFMM_OK or an error code (which the solver returns as is). */
typedef int (*bbfmm_apply_fn)(void *user, const double *x, double *y, int64_t n);
/* ProgressMsg::SolverIteration {iter, residual, progress} (iterative_solvers.rs:142-148) */
typedef void (*bbfmm_iteration_fn)(void *user, int64_t iter, double residual, double progress);

/* FittingAccuracyType (interpolant_config.rs:54-63) */
enum { BBFMM_ACCURACY_ABSOLUTE = 0, BBFMM_ACCURACY_RELATIVE = 1 };

/* givens_rotation (iterative_solvers.rs:185-227), a port of LAPACK dlartg:
 * [c s; -s c] [f; g] = [r; 0]. */
void bbfmm_givens_rotation(double f, double g, double *c, double *s, double *r);

/*
 * fgmres (iterative_solvers.rs:38-172): restarted flexible GMRES, right preconditioner m
 * (NULL: none), initial guess x0 (NULL: zero), max_outer_iterations restarts of
 * max_inner_iterations Krylov vectors (the solver uses 20 x 5, rbf.rs:545-554), modified
 * Gram-Schmidt, Givens rotations.  Stopping: Absolute -> |g[j+1]| (max-norm of the true residual
 * at restarts) < tolerance; Relative -> the same over the initial 2-norm.  callback (may be NULL)
 * receives every inner iteration.  Outputs: x (n), the number of inner iterations done and the
 * last residual measure (both optional).
 * Deviation: an exactly zero residual returns x instead of dividing by zero.
 */
int bbfmm_fgmres(int64_t n, bbfmm_apply_fn a, void *a_user, const double *b, bbfmm_apply_fn m, void *m_user,
                 const double *x0, int32_t max_outer_iterations, int32_t max_inner_iterations,
                 int32_t tolerance_type, double tolerance, bbfmm_iteration_fn callback, void *cb_user,
                 double *x, int64_t *iterations, double *final_residual);

/* schwarz_ddm_solver (iterative_solvers.rs:229-281): s += M(r); r = rhs - A s, at most
 * max_iterations times (the solver uses 100, rbf.rs:555-562).  m NULL -> zero vector, as the
 * reference. */
int bbfmm_schwarz_ddm_solver(int64_t n, bbfmm_apply_fn matvec, void *a_user, const double *rhs,
                             bbfmm_apply_fn m, void *m_user, int32_t max_iterations, int32_t tolerance_type,
                             double tolerance, bbfmm_iteration_fn callback, void *cb_user, double *x,
                             int64_t *iterations, double *final_residual);

/* IterativeSolver::matvec (rbf.rs:105-117) as an operator callback: pass a bbfmm_rbf_system as
 * `user`; n must be N + basis_size.  Runs bbfmm_fast_matrix_vector_product on all sources. */
typedef struct bbfmm_rbf_system {
    bbfmm_handle *tree;
    int64_t basis_size;            /* InterpolantSettings::basis_size */
    const double *monomial_matrix; /* N x basis_size column-major, or NULL */
    int64_t ld_monomial;
    double nugget;
} bbfmm_rbf_system;
int bbfmm_rbf_system_apply(void *user, const double *x, double *y, int64_t n);

/* ------------------------------------------------------------------ iterative solvers, vectors on the device
 * The same two drivers with every vector in HBM ("Device-resident solvers"): x, r, the Krylov basis V and
 * the preconditioned basis Z never leave the device, the dot products, norms and updates are kernels on one stream,
 * and the host keeps only H, g and the Givens rotations.  Opt-in: the host entries above are unchanged. */

/* d_y = Op(d_x) on DEVICE vectors of n doubles: enqueue the work on `stream` (a hipStream_t) and return BBFMM_OK or
 * an error code (which the solver returns as is).  d_x and d_y never alias. */
typedef int (*bbfmm_apply_device_fn)(void *user, const double *d_x, double *d_y, int64_t n, void *stream);

/* IterativeSolver::matvec (rbf.rs:105-117) on device vectors: the device twin of bbfmm_rbf_system_apply.  Created once
 * from the tree, basis_size, the N x basis_size column-major monomial matrix (host pointer, ld >= N; NULL with
 * basis_size 0) and the nugget; the matrix is uploaded once.  An apply is bbfmm_matvec_device followed by one kernel:
 * y[i] += nugget x[i] + sum_q P[i,q] x[N+q] (the polynomial sum first, then added, as the host entry does), and
 * y[N .. N+basis_size) = 0 (rbf.rs:1346).  BBFMM_DEVICE_ERROR with a message in bbfmm_last_error(tree) on a
 * BBFMM_FLAG_HOST_ONLY handle, BBFMM_UNSUPPORTED with a message on a device group (bbfmm_create_on_devices). */
typedef struct bbfmm_rbf_system_device bbfmm_rbf_system_device;
int bbfmm_rbf_system_device_create(bbfmm_handle *tree, int64_t basis_size, const double *monomial_matrix, int64_t ld,
                                   double nugget, bbfmm_rbf_system_device **out);
void bbfmm_rbf_system_device_destroy(bbfmm_rbf_system_device *s);
/* a bbfmm_apply_device_fn: user = bbfmm_rbf_system_device*, n = N + basis_size, stream = bbfmm_stream(tree)
 * (any other stream: BBFMM_BAD_ARGUMENT) */
int bbfmm_rbf_system_apply_device(void *user, const double *d_x, double *d_y, int64_t n, void *stream);

/*
 * fgmres (iterative_solvers.rs:38-281) with b, x0 (NULL: zero) and x as DEVICE pointers and everything enqueued on
 * `stream`: the algorithm of bbfmm_fgmres statement for statement (restarts, Givens rotations on the host, the
 * residual measure from |g[j+1]| and from the true residual at a restart, the zero-residual return, the iteration
 * count, the callback).  Reductions run in two stages without atomics -- one partial per 65,536 elements, the
 * partials added in index order -- so a solve is bitwise reproducible and differs from bbfmm_fgmres only by the order
 * of summation inside a chunk.  The host waits for the stream once per inner iteration (the new Hessenberg column and
 * the norm, max_inner_iterations + 2 doubles at most) and once more per restart or return.  Work memory:
 * 2 max_inner_iterations + 3 vectors of n doubles, allocated per call and freed on every return path.
 * Native operators (bbfmm_rbf_system_apply_device, bbfmm_schwarz_apply_device) must belong to one tree whose stream is
 * `stream`: BBFMM_BAD_ARGUMENT otherwise.  `stream` is a created stream: the null stream is refused (BBFMM_BAD_ARGUMENT) --
 * work that the solver and a caller's operator (torch) enqueue on it was measured not to stay in order.
 */
int bbfmm_fgmres_device(int64_t n, bbfmm_apply_device_fn a, void *a_user, const double *d_b, bbfmm_apply_device_fn m,
                        void *m_user, const double *d_x0, int32_t max_outer_iterations, int32_t max_inner_iterations,
                        int32_t tolerance_type, double tolerance, bbfmm_iteration_fn callback, void *cb_user,
                        double *d_x, int64_t *iterations, double *final_residual, void *stream);

/* schwarz_ddm_solver (iterative_solvers.rs:229-281) in the same way: one wait per iteration (the residual norm). */
int bbfmm_schwarz_ddm_solver_device(int64_t n, bbfmm_apply_device_fn matvec, void *a_user, const double *d_rhs,
                                    bbfmm_apply_device_fn m, void *m_user, int32_t max_iterations,
                                    int32_t tolerance_type, double tolerance, bbfmm_iteration_fn callback,
                                    void *cb_user, double *d_x, int64_t *iterations, double *final_residual,
                                    void *stream);

/* Test hook: one vector kernel of the device solvers on the caller's HOST vectors (uploaded, run, downloaded).
 *   op 0: out = a - b                         scalars_out[0] = sum out^2, [1] = max |out|   (the fused residual pass)
 *   op 1: out = alpha' a
 *   op 2: out = b + alpha' a                  scalars_out[0] = <c, out> (c NULL: <out, out>)
 *   op 3: scalars_out[0] = <a, b>             op 4: ||a||_2         op 5: max |a|
 *   op 6: out = b + sum_c coeffs[c] a[:, c]   (a: n x count column-major, the solution update)
 * alpha' is read from a device scalar holding alpha: alpha_mode 0 alpha, 1 -alpha, 2 1/alpha (0 when alpha == 0);
 * alpha_mode 3 passes alpha as a kernel argument.  offset (0 or 1): the device vectors start that many doubles past a
 * 16-byte boundary (1: the kernels take their 8-byte path).  Reductions need n >= 1. */
int bbfmm_debug_solver_vector_op(int32_t op, int32_t alpha_mode, int64_t n, const double *a, const double *b,
                                 const double *c, double alpha, int32_t count, const double *coeffs, int32_t offset,
                                 double *out, double *scalars_out);

/* ------------------------------------------------------------------ domain decomposition (host part)
 * DDMTree::new (ferreus_rbf/src/preconditioning/domain_decomposition.rs:67-347), SURVEY.md 8(f)-1:
 * the multi-level overlapping decomposition of the Schwarz preconditioner -- which points form which
 * leaf domain on which level.  The local factorisations (domain.rs) and the apply (schwarz.rs) on these
 * index sets are the bbfmm_schwarz_* entry points further down. */
typedef struct bbfmm_ddm bbfmm_ddm;
typedef struct bbfmm_ddm_params { /* DDMParams, config.rs:42-69 */
    int64_t leaf_threshold;   /* 1024 */
    double overlap_quota;     /* 0.5 */
    double coarse_ratio;      /* 0.125 */
    int64_t coarse_threshold; /* 4096 */
} bbfmm_ddm_params;
void bbfmm_ddm_params_defaults(bbfmm_ddm_params *out);
/* Extension (not in the reference): the defaults with coarse_threshold raised so that the hierarchy over
 * n points keeps at most three fine levels, coarse_threshold = max(4096, n/470 + 1): a level keeps
 * ceil(ceil(N/8)/leaves) points per leaf, at most N (1/8 + 1/341), so three levels leave at most n/478.  With the plain
 * defaults a fourth fine level appears above about 2.1M points and leaves one coarse point per ~7 level-0
 * domains, where the sweep of schwarz.rs stalls for the thin-plate spline. */
void bbfmm_ddm_params_for_points(int64_t n, bbfmm_ddm_params *out);
/* points: n x d column-major (ld); params NULL -> defaults */
int bbfmm_ddm_build(const double *points, int64_t n, int32_t d, int64_t ld, const bbfmm_ddm_params *params,
                    bbfmm_ddm **out);
void bbfmm_ddm_destroy(bbfmm_ddm *t);
int32_t bbfmm_ddm_num_levels(const bbfmm_ddm *t);                 /* finest first, coarse domain last */
int64_t bbfmm_ddm_level_size(const bbfmm_ddm *t, int32_t level);  /* Level::point_indices.len() */
int bbfmm_ddm_level_points(const bbfmm_ddm *t, int32_t level, int64_t *out);
int64_t bbfmm_ddm_num_domains(const bbfmm_ddm *t, int32_t level); /* Level::leaf_domains.len() */
int64_t bbfmm_ddm_domain_size(const bbfmm_ddm *t, int32_t level, int64_t domain);
/* Domain::{overlapping_point_indices, internal_points_mask, extents [mins..., maxs...]} */
int bbfmm_ddm_domain(const bbfmm_ddm *t, int32_t level, int64_t domain, int64_t *indices, uint8_t *internal,
                     double *extents);

/* ------------------------------------------------------------------ Schwarz preconditioner
 * schwarz_preconditioner (ferreus_rbf/src/preconditioning/schwarz.rs:32-155) with Domain::factorise /
 * Domain::solve (domain.rs:153-475) for all leaf domains of a level batched on the device: Beatson's Q
 * formulation, Q^T A Q assembled from the points, blocked Cholesky and substitutions one workgroup
 * per domain.  The two partial matvecs per fine level go through `tree`
 * (IterativeSolver::precon, rbf.rs:140-155).  With a global trend the
 * monomials are evaluated at the world points: bbfmm_schwarz_create_ex below.
 * A domain whose Cholesky factorisation fails is solved through a host-computed inverse instead (the
 * role of the reference's LBL^T fallback, domain.rs:60-68); the one large coarse domain (more than 2048
 * points) is then factorised by pivoted LU on the device (rocSOLVER, loaded on demand).  BBFMM_UNSUPPORTED
 * is returned only when a local system is singular or that library is missing. */
typedef struct bbfmm_schwarz bbfmm_schwarz;
typedef struct bbfmm_interpolant { /* InterpolantSettings, interpolant_config.rs:118-147, as the solver reads it */
    int32_t kernel_type;       /* bbfmm_kernel_type 0..6 (Linear, ThinPlateSpline, Cubic, Spheroidal3/5/7/9) */
    int32_t polynomial_degree; /* -1 none, 0 constant, 1 linear, 2 quadratic (Drift) */
    double nugget, base_range, total_sill;
    uint32_t flags;            /* 0, or BBFMM_FLAG_GLOBAL_SCALING */
} bbfmm_interpolant;
/* Default (0): the coarse domain scales its monomials by the extents of its own points, as the
 * reference does (domain.rs:171-172).  With this flag it uses the extents of all points, the basis
 * of the system's monomial matrix, which makes its polynomial tail exact (see csrc/schwarz.cpp). */
#define BBFMM_FLAG_GLOBAL_SCALING 1u
/* tree: a handle over the same points, kernel and ranges (it serves matvec_partial); it must outlive
 * the preconditioner.  params NULL -> DDMParams defaults. */
int bbfmm_schwarz_create(bbfmm_handle *tree, const double *points, int64_t n, int32_t d, int64_t ld,
                         const bbfmm_interpolant *settings, const bbfmm_ddm_params *params, bbfmm_schwarz **out);
/* The same preconditioner with its FACTORS SHARDED over the ranks of a job (level 0 of 10M points holds
 * 95 GB of Cholesky factors, one GPU's 288 GB end near 28M points).  No counterpart in the reference (one address space).
 * Every rank decomposes the same points the same way, keeps the contiguous share [nd * rank / world, nd * (rank + 1) /
 * world) of every fine level's domains -- factorises and solves only those -- and after a level's local solves the
 * corrections of all ranks are summed: the internal points of the domains partition the level's rows (restricted
 * additive Schwarz, schwarz.rs:96-113), so each row is written by exactly one rank and the sum adds zeros (the result
 * equals the unsharded preconditioner's bit for bit).  The coarse domain (one domain) and the partial products through
 * `tree` are replicated.
 *   d_exchange: DEVICE buffer of the caller, exchange_capacity >= the largest fine level (N) doubles;
 *   allreduce(user, count): sum d_exchange[0 .. count) over the ranks in place (ncclAllReduce / torch.distributed);
 *     called from bbfmm_schwarz_apply with the library's stream idle, must return with the result visible to the device.
 * The ranks run the replicated parts (the partial products through `tree`, the coarse solve, the solver around the sweep)
 * in LOCK STEP: `tree` must be a BBFMM_FLAG_DETERMINISTIC handle on every rank (the default path's f64 atomics leave the
 * ranks' replicated results different in their last bits, and a solver near its tolerance could stop on one rank while
 * the others wait in the next all-reduce), or the caller broadcasts the solver's decisions.  A rank that fails inside a
 * sharded level still takes part in the level's all-reduce with a poisoned (NaN) contribution, so every rank returns an
 * error from that bbfmm_schwarz_apply instead of one returning and the others waiting; after a failed CREATE the caller
 * must agree on the status itself before the first apply (ddm.py does: MIN over the group).
 * rank 0 / world 1 (no exchange) is bbfmm_schwarz_create. */
typedef int (*bbfmm_allreduce_fn)(void *user, int64_t count);
int bbfmm_schwarz_create_sharded(bbfmm_handle *tree, const double *points, int64_t n, int32_t d, int64_t ld,
                                 const bbfmm_interpolant *settings, const bbfmm_ddm_params *params, int32_t rank,
                                 int32_t world, double *d_exchange, int64_t exchange_capacity,
                                 bbfmm_allreduce_fn allreduce, void *allreduce_user, bbfmm_schwarz **out);
/* The same two with a global trend (GlobalTrend, global_trend.rs): `points` are the TRANSFORMED points -- the geometry of
 * the decomposition, the kernel blocks and the cube scaling factors of every monomial basis come from them -- and the
 * monomials are evaluated at monomial_points (n x d, ld_monomial), the WORLD points, as the reference does
 * (domain.rs:161-175; rbf.rs:418-421, 476-491; domain_decomposition.rs:315, 338).  monomial_points NULL is the entry
 * above, bit for bit (bbfmm_schwarz_create forwards with NULL). */
int bbfmm_schwarz_create_ex(bbfmm_handle *tree, const double *points, int64_t n, int32_t d, int64_t ld,
                            const double *monomial_points, int64_t ld_monomial, const bbfmm_interpolant *settings,
                            const bbfmm_ddm_params *params, bbfmm_schwarz **out);
int bbfmm_schwarz_create_sharded_ex(bbfmm_handle *tree, const double *points, int64_t n, int32_t d, int64_t ld,
                                    const double *monomial_points, int64_t ld_monomial, const bbfmm_interpolant *settings,
                                    const bbfmm_ddm_params *params, int32_t rank, int32_t world, double *d_exchange,
                                    int64_t exchange_capacity, bbfmm_allreduce_fn allreduce, void *allreduce_user,
                                    bbfmm_schwarz **out);
int64_t bbfmm_schwarz_factor_bytes(const bbfmm_schwarz *h); /* device bytes of the packed factors this handle holds */
/* domains of `level` this handle factorised (returned), the first of them and the level's total in the decomposition */
int64_t bbfmm_schwarz_domains_owned(const bbfmm_schwarz *h, int32_t level, int64_t *first, int64_t *total);
void bbfmm_schwarz_destroy(bbfmm_schwarz *h);
int64_t bbfmm_schwarz_basis_size(const bbfmm_schwarz *h);           /* InterpolantSettings::basis_size */
int32_t bbfmm_schwarz_num_levels(const bbfmm_schwarz *h);
const double *bbfmm_schwarz_monomial_matrix(const bbfmm_schwarz *h); /* N x basis column-major (rbf.rs:485-491) or NULL */
/* evaluate_monomials (ferreus_rbf/src/polynomials.rs:30-74) as the solver's matrix and the domains' matrices compute it:
 * out (n x basis column-major, basis = 1 / d + 1 / (d + 1)(d + 2) / 2 for degree 0 / 1 / 2) on (x - translation) / scale
 * (NULL: 0 and 1).  Host only; the reference's own known answers (polynomials.rs:163-242) are checked through it. */
int bbfmm_debug_evaluate_monomials(const double *points, int64_t n, int32_t d, int64_t ld, int32_t degree,
                                   const double *translation, const double *scale, double *out);
int64_t bbfmm_schwarz_level_size(const bbfmm_schwarz *h, int32_t level);      /* Level::point_indices */
int bbfmm_schwarz_level_points(const bbfmm_schwarz *h, int32_t level, int64_t *out);
/* solve_fine_level / solve_coarse_level (schwarz.rs:84-155) of one level for a given residual
 * (n = N + basis_size values in, n out); parity checks. */
int bbfmm_schwarz_debug_level_solve(bbfmm_schwarz *h, int32_t level, const double *residual, double *out,
                                    int64_t n, int32_t add_poly);
/* Test hook: the local solvers of ONE level (Domain::factorise / Domain::solve, domain.rs:153-475, batched on the device)
 * on domains the caller prescribes instead of those of the decomposition.  Domain i holds the points
 * dom_idx[dom_ptr[i] .. dom_ptr[i + 1]) of `points` (n x d column-major, ld) with their internal flags; settings as for
 * bbfmm_schwarz_create, basis_size = the monomial basis of (d, polynomial_degree).  The level is built and solved by the
 * functions the preconditioner itself calls; the getters only copy its buffers out.
 *   _info: info[8] = {domains, entries (points of all domains), doubles of Q, doubles of the packed matrices, 1 when the
 *          level is one large domain (more than 2048 rows: the multi-launch path), 1 when that domain went to the pivoted
 *          LU, domains on the host fallback, largest m}
 *   _layout: per domain k (special points); per entry, in the domains' reordered point order (special points first), the
 *          global index and the internal flag; Q (per domain k x m row-major, m = points - k); per domain mode (1: the
 *          Cholesky factorisation failed, the packed matrix holds the symmetric inverse)
 *   _assembled: Q^T A Q of every domain as the assembly kernels write it, packed lower triangles column by column (m (m +
 *          1) / 2 doubles each), assembled again into a scratch buffer by the same launches
 *   _factor: the packed matrices as the solves read them (the Cholesky factors, or the inverses of mode 1)
 *   _solve: ddm_level_solve: values n doubles in; out n doubles in and out -- rows of internal points (all points when
 *          all_points) receive the domain coefficients, the other rows are left alone. */
typedef struct bbfmm_ddm_debug_level bbfmm_ddm_debug_level;
int bbfmm_ddm_debug_level_create(const double *points, int64_t n, int32_t d, int64_t ld, int64_t n_dom,
                                 const int64_t *dom_ptr, const int64_t *dom_idx, const uint8_t *dom_internal,
                                 const bbfmm_interpolant *settings, int32_t basis_size, int32_t solve_for_poly,
                                 bbfmm_ddm_debug_level **out);
/* ... with the monomials evaluated at monomial_points (NULL: at points), as bbfmm_schwarz_create_ex */
int bbfmm_ddm_debug_level_create_ex(const double *points, int64_t n, int32_t d, int64_t ld, const double *monomial_points,
                                    int64_t ld_monomial, int64_t n_dom, const int64_t *dom_ptr, const int64_t *dom_idx,
                                    const uint8_t *dom_internal, const bbfmm_interpolant *settings, int32_t basis_size,
                                    int32_t solve_for_poly, bbfmm_ddm_debug_level **out);
void bbfmm_ddm_debug_level_destroy(bbfmm_ddm_debug_level *h);
int bbfmm_ddm_debug_level_info(const bbfmm_ddm_debug_level *h, int64_t *info);
int bbfmm_ddm_debug_level_layout(const bbfmm_ddm_debug_level *h, int32_t *k, int64_t *indices, uint8_t *internal, double *q,
                                 uint8_t *mode);
int bbfmm_ddm_debug_level_assembled(const bbfmm_ddm_debug_level *h, double *out);
int bbfmm_ddm_debug_level_factor(const bbfmm_ddm_debug_level *h, double *out);
int bbfmm_ddm_debug_level_solve(bbfmm_ddm_debug_level *h, const double *values, double *out, int64_t n, int32_t all_points);
/* a bbfmm_apply_fn: user = bbfmm_schwarz*, vectors of N + basis_size doubles */
int bbfmm_schwarz_apply(void *user, const double *residual, double *correction, int64_t n);
/* schwarz_preconditioner (schwarz.rs:32-82) as a bbfmm_apply_device_fn: the same sweep with the residual taken from and
 * the correction left in DEVICE memory (device-to-device copies in place of the two bus legs; the polynomial tail is
 * written by a kernel).  user = bbfmm_schwarz*, n = N + basis_size, stream = the tree's stream (any other:
 * BBFMM_BAD_ARGUMENT).  The coarse domain's polynomial tail is solved on the host as in bbfmm_schwarz_apply, so an apply
 * with a drift waits for the stream once; a sharded preconditioner is refused (BBFMM_UNSUPPORTED). */
int bbfmm_schwarz_apply_device(void *user, const double *d_residual, double *d_correction, int64_t n, void *stream);
/* Test hook: bbfmm_schwarz_apply with the device vectors of the sweep copied out after every level step.  The apply and the
 * hook run the same loop; the hook alone waits for the stream and copies (unsharded handles only).
 *   _trace_steps: the level steps of one apply (2 (levels - 1), or 1 for a single level)
 *   step_info:  5 per step: level, coarse, have_sl, add_poly, values of the polynomial tail the step produced (0: none)
 *   initial:    2 N: the level residual and the local-solve output as the sweep finds them (they persist between applies)
 *   vectors:    4 N per step: the partial product (the level's size; zeros when have_sl is 0), the level residual, the
 *               local-solve output, the running correction
 *   small:      32 per step: the projection on the polynomial basis (fine levels with a basis) at 0, the tail at 16
 * _debug_ortho_matrix: the orthonormal polynomial basis the sweep projects on (rbf.rs:493-495), N x basis column-major, or NULL. */
int32_t bbfmm_schwarz_debug_trace_steps(const bbfmm_schwarz *h);
int bbfmm_schwarz_debug_apply_trace(bbfmm_schwarz *h, const double *residual, double *correction, int64_t n, int32_t max_steps,
                                    int32_t *step_info, double *initial, double *vectors, double *small, int32_t *n_steps);
const double *bbfmm_schwarz_debug_ortho_matrix(const bbfmm_schwarz *h);

/* ---- The interpolant around the tree: what ferreus_rbf::RBFInterpolator (ferreus_rbf/src/rbf.rs:304-1298) adds to the
 * kernel sum.  Arrays of points, values and gradients are column-major like every other entry's (column a at + a * ld);
 * gradients are m x (k * d), columns [rhs0_dx, rhs0_dy, rhs0_dz, rhs1_dx, ...].  Nothing throws across the ABI. */

/* GlobalTrendTransform::new (global_trend.rs:135-264) for GlobalTrend::One / Two / Three (d = 1, 2, 3).
 * params: d = 1 {major_ratio}; d = 2 {rotation_angle, major_ratio, minor_ratio}; d = 3 {dip, dip_direction, pitch,
 * major_ratio, semi_major_ratio, minor_ratio}; angles in degrees.  affine_out and inverse_out are (d + 1) x (d + 1)
 * row-major for row-vector points, [x 1] * affine: its leading d x d block is B, the first d entries of its last row b
 * (transform_points, global_trend.rs:266-272).  The matrices are multiplied in the reference's order (transform_back *
 * scale * rotation * transform, then transposed); the inverse is taken by LU with partial pivoting on the host. */
int bbfmm_global_trend_transform(int32_t d, const double *params, const double *center, double *affine_out, double *inverse_out);

/* duplicate_cutoff_distance (rbf.rs:1391-1415): h_ref when |phi(h_ref) - phi(0)| is already within the target eps *
 * |phi(h_ref) - phi(0)| (only when that rise is 0), else a root r in (0, h_ref) of |phi(r) - phi(0)| = target by
 * bisection to 1e-13 relative, towards the smallest crossing.  The rise is evaluated without the subtraction's
 * cancellation (r, |r^2 ln r|, r^3, slope * r), so the root is that of the kernel's formula where the reference's
 * own residual is a step function of one ulp of phi(0) (the spheroidal family). */
int bbfmm_duplicate_cutoff_distance(const bbfmm_interpolant *interpolant, double h_ref, double *out);

/* remove_duplicates (rbf.rs:1430-1467) with tol given: point i is kept iff no KEPT j < i has |x_i - x_j|_inf <= tol
 * (inclusive, kdtree.rs:187); keep_out (n entries allocated) receives the n_keep_out kept indices, ascending.
 * where = 0: the host (a hash of a uniform grid; the checker and the path without a device).  where = 1: the device --
 * points sorted by grid cell key (rocPRIM), each point probing the 3^d cells around it for earlier neighbours, resolved
 * in rounds to the fixed point (no earlier neighbour, or all of them dropped: kept; an earlier kept neighbour: dropped;
 * one status word read back per round, *rounds_out of them), which is the sequential set exactly.  The cell side is
 * max(tol (1 + 2^-10), largest extent / 2^20 (2^30 below 3-D)), so the key always fits 64 bits: a tolerance far below
 * the extent costs larger cells, never another path.  2^31 points or more, or a machine with no device at all, take
 * the host path from where = 1 as well (the same set).  Cost, neither case measured: a point scans its 3^d cells linearly,
 * so a cloud that a few far outliers squeeze into a handful of cells costs O(n^2) pair tests per round, and a chain of
 * n points each within tol of the next costs n / 2 rounds of one launch and one read each.
 * Non-finite coordinates or tol are BBFMM_BAD_ARGUMENT. */
int bbfmm_remove_duplicates(const double *points, int64_t n, int32_t d, int64_t ld, double tol, int32_t where, int64_t *keep_out,
                            int64_t *n_keep_out, int64_t *rounds_out);

/* The terms of one interpolant besides its kernel sum.  size = sizeof(bbfmm_interpolant_terms). */
typedef struct bbfmm_interpolant_terms {
    int64_t size;
    int32_t d;                  /* 1..3 */
    int32_t polynomial_degree;  /* -1 none .. 2 quadratic */
    int32_t k;                  /* value columns */
    int32_t has_affine;         /* 0: no global trend (B, b ignored) */
    const double *coefficients; /* basis_size x k polynomial coefficients, column c at + c * ld_coefficients, monomials in
                                 * the order of polynomials.rs:30-74 (1 | s_a | s_a s_b, a <= b) */
    int64_t ld_coefficients;
    double translation[3], scale[3]; /* s = (x - translation) / scale, common.rs:330-336 */
    double B[9], b[3];               /* x' = x B + b, B row-major d x d */
} bbfmm_interpolant_terms;

/* The three per-target operations on caller arrays, on the host (where = 0) or the device (where = 1, one kernel
 * between an upload and a download), one __host__ __device__ definition of the arithmetic behind both
 * (csrc/interpolant_terms.hpp; sums in a fixed order, never contracted to fused multiply-adds):
 *   which = 0, affine_points: points_out = x B + b, summed a = 0 .. d-1 then + b (global_trend.rs:266-272);
 *   which = 1, polynomial_terms: values[:, c] += sum_j m_j(s) coefficients[j, c], j ascending, and with grad
 *              grad[:, c d + a] += d/dx_a of that sum (polynomials.rs:64-116); x are WORLD points;
 *   which = 2, trend_gradients: grad <- grad B^T per target and column, in place (rbf.rs:1272-1298). */
int bbfmm_debug_interpolant_terms(int32_t where, int32_t which, const bbfmm_interpolant_terms *terms, const double *x, int64_t m,
                                  int64_t ldx, double *points_out, int64_t ldp, double *values, int64_t ldv, double *grad,
                                  int64_t ldg);

/* _evaluate (rbf.rs:1180-1270) in one call: the targets x (WORLD points) are mapped by the trend on the device, the
 * existing Full (mode 0: bbfmm_evaluate[_with_gradients]) or Leaves (mode 1: bbfmm_evaluate_leaves[...]) pass runs at
 * the mapped targets with the same w / rows / k / ldw, then one kernel applies trend_gradients, nugget * w (nugget != 0
 * asks for it: the at-source case, m = N and w given) and polynomial_terms, in the reference's order.  terms NULL, or
 * no trend with degree -1 and nugget 0, is the plain entry point bit for bit.  The mapped targets and the results
 * make one extra trip through the host between the trend kernel, the tree's pass and the terms kernel (the tree's
 * passes take host targets; each kernel sits between its own upload and download on the null stream).  A failure here
 * sets the handle's bbfmm_last_error like the entries it forwards to.  On a device group (FERREUS_BBFMM_DEVICES) the terms run on the primary part's device. */
#define BBFMM_EVALUATE_FULL 0
#define BBFMM_EVALUATE_LEAVES 1
int bbfmm_evaluate_interpolant(bbfmm_handle *h, int32_t mode, int32_t with_gradients, const double *w, int64_t rows, int32_t k,
                               int64_t ldw, const double *x, int64_t m, int64_t ldx, const bbfmm_interpolant_terms *terms,
                               double nugget, double *values_out, int64_t ldo, double *grad_out, int64_t ldg,
                               int64_t *bad_point_index);

/* ---- Evaluation at device-resident targets and on regular grids (Leaves mode: bbfmm_set_local_coefficients first,
 * BBFMM_BAD_ARGUMENT otherwise; all k columns of the weights).
 *
 * A regular grid.  size = sizeof(bbfmm_grid).  steps is 3 x 3 row-major whatever d is: row j (steps[3 j + a]) is the
 * world step of index j, so a rotated block model is a non-diagonal steps.  Rows are in C order,
 * r = (i0 n1 + i1) n2 + i2.  Axes at or beyond d are absent: their shape counts as 1 and they add no term.  The node is
 *   x_a = ((origin_a + (double)i0 S[0][a]) + (double)i1 S[1][a]) + (double)i2 S[2][a],
 * every product and sum rounded, in this order, never fused, on the host and on the device alike. */
typedef struct bbfmm_grid {
    int64_t size;
    int32_t d; /* 1..3, the tree's */
    int32_t reserved;
    int64_t shape[3];
    double origin[3];
    double steps[9];
} bbfmm_grid;

/* Options of the two entries below.  size: sizeof(bbfmm_evaluate_options) as the caller was compiled; fields beyond it,
 * and a NULL struct, take the defaults.
 *   batch_independent: -1 (the default) the handle's BBFMM_FLAG_DETERMINISTIC flag, 0 / 1: the near field and M2P split a
 *     job's targets the same way whatever their number, so that on a deterministic handle a target's value is the same
 *     double whichever other targets, slab or job cut share the call;
 *   max_job_targets: the jobs of the leaf pass (P2P, M2P, L2P) hold at most this many targets: a leaf with n targets is
 *     cut into q = ceil(n / cap) jobs, job j taking [floor(j n / q), floor((j + 1) n / q)) of them.  0: one job per leaf,
 *     the target set of every other entry point.  -1 (the default): the library's choice;
 *   batch_bytes (grid): device memory of one slab (<= 0: 2 GiB, the isosurfacer's default);
 *   outputs_on_device (grid): values_out / grad_out are device pointers on the handle's device. */
typedef struct bbfmm_evaluate_options {
    int64_t size;
    int32_t batch_independent;
    int32_t max_job_targets;
    int64_t batch_bytes;
    int32_t outputs_on_device;
} bbfmm_evaluate_options;

/* m targets on the handle's device as SoA, column a at d_x + a * ldx.  Values m x k column-major to d_values (device,
 * leading dimension ldo); with_gradients: component a of column c to column c * d + a of d_grad (leading dimension ldg),
 * as in the host entries; both in the caller's row order.  terms (NULL: none; k = the weights' columns, host
 * coefficients): the trend's map of the targets runs before the pass, trend_gradients and polynomial_terms behind it, on
 * the handle's stream, which is idle on return.  A row outside the tree: BBFMM_POINT_OUTSIDE_TREE with the smallest such
 * row in *bad_point_index.  On a device group the call runs on the primary part. */
int bbfmm_evaluate_device(bbfmm_handle *h, int32_t with_gradients, const double *d_x, int64_t m, int64_t ldx,
                          const bbfmm_interpolant_terms *terms, double *d_values, int64_t ldo, double *d_grad, int64_t ldg,
                          const bbfmm_evaluate_options *options, int64_t *bad_point_index);

/* The same at the nodes of a grid, rows in C order: slabs of whole leading-index planes sized to batch_bytes (a plane
 * that does not fit is cut by rows; a slab holds fewer than 2^31 rows), each slab coordinates -> the pass above -> its
 * rows of values_out / grad_out (host arrays, or device arrays with outputs_on_device).  ldo, ldg >= the grid's rows.
 * A zero in shape is an empty grid and BBFMM_OK. */
int bbfmm_evaluate_grid(bbfmm_handle *h, int32_t with_gradients, const bbfmm_grid *grid, const bbfmm_interpolant_terms *terms,
                        double *values_out, int64_t ldo, double *grad_out, int64_t ldg, const bbfmm_evaluate_options *options,
                        int64_t *bad_point_index);

/* Of the handle's last grid call: nodes, slabs, leaf runs (leaves with targets, summed over the slabs), jobs after the
 * cut, targets of the largest job, M2P (W) jobs, 0, 0: eight values. */
int bbfmm_evaluate_grid_stats(bbfmm_handle *h, int64_t *stats_out);

/* Test hooks, where = 0 on the host and 1 on the device (one kernel between an upload and a download), one definition
 * of the arithmetic behind both: rows [r0, r0 + n) of the grid as SoA columns, column a at out + a * ld; */
int bbfmm_debug_grid_coords(int32_t where, const bbfmm_grid *grid, int64_t r0, int64_t n, double *out, int64_t ld);
/* and the cut of n_runs runs (job_cell / tgt_begin / tgt_end, lengths >= 0) into jobs of at most cap >= 1 targets.
 * out_*: capacity values each (NULL: the count alone); *n_jobs_out the number of jobs, BBFMM_BAD_ARGUMENT when it
 * exceeds the capacity. */
int bbfmm_debug_split_runs(int32_t where, const int32_t *tgt_begin, const int32_t *tgt_end, const int32_t *job_cell, int64_t n_runs,
                           int32_t cap, int32_t *out_begin, int32_t *out_end, int32_t *out_cell, int64_t capacity,
                           int64_t *n_jobs_out);

#ifdef __cplusplus
}
#endif
#endif /* FERREUS_BBFMM_HIP_H */
