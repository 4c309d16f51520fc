// Dense marching tetrahedra on the regularised-marching-tetrahedra (RMT) sampling lattice: the triangles of
// ferreus_rmt's build_isosurface with ClusterMethod::None (raw, one vertex per crossed lattice edge) or
// ClusterMethod::Average or ClusterMethod::CurvatureWeighted (the intersections near a sample point merged where the topology tests allow it, with the
// predicted-edge and non-manifold rollbacks and, where asked for, the self-intersection rollback), taken from every sample
// point of the extraction domain in device passes instead of a CPU wavefront; with kFinishClipped followed by its clip_mesh_to_aabb and clean_mesh on the device (the
// finished mesh of BoundaryClosure::None) and with kFinishClosePositive / kFinishCloseNegative then closed on the six faces
// of the extents (isosurface_closure.hpp).  With kFollowSurface the field is evaluated only in the
// bricks of lattice nodes that a wavefront reaches from projected seed points (isosurface_follow.hip), as the reference
// follows the surface, and the same passes run on that field.  Contract: DESIGN.md "Isosurfaces on the RMT
// lattice"; numpy restatements: tests/isosurface_restatement.py, tests/isosurface_cluster_restatement.py,
// tests/isosurface_finish_restatement.py, tests/isosurface_intersect_restatement.py and
// tests/isosurface_follow_restatement.py.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace bbfmm {
namespace iso {

// ---- the reference's tables (ferreus_rmt/src/constants.rs; values checked against tests/golden/rmt_tables.json)
// IJK offsets of the 14 edges of a sample point; 0..6 are the edges it owns.
constexpr int kEdgeDeltas[14][3] = {{-1, 1, 0}, {-2, 0, 0}, {-1, -1, 0}, {0, 1, -1}, {-1, 0, -1}, {0, -1, -1}, {1, 0, -1},
                                    {1, -1, 0}, {2, 0, 0},  {1, 1, 0},   {0, -1, 1}, {1, 0, 1},   {0, 1, 1},   {-1, 0, 1}};
constexpr int kReverseEdge[14] = {7, 8, 9, 10, 11, 12, 13, 0, 1, 2, 3, 4, 5, 6};
// the 6 tetrahedra a sample point owns (edge labels of its 3 other corners)
constexpr int kOwnedTetEdges[6][3] = {{0, 4, 1}, {0, 3, 4}, {3, 6, 4}, {1, 4, 2}, {2, 4, 5}, {4, 6, 5}};
// tetrahedron edges as corner pairs
constexpr int kTetEdgePairs[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// marching-tetrahedra table: per case (bit i = corner i inside) its triangle count and up to 2 triangles of tet edges
constexpr int kMtCount[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
constexpr int kMtTable[16][2][3] = {
    {{0, 0, 0}, {0, 0, 0}}, {{0, 1, 2}, {0, 0, 0}}, {{0, 4, 3}, {0, 0, 0}}, {{3, 1, 2}, {3, 2, 4}},
    {{1, 3, 5}, {0, 0, 0}}, {{5, 2, 0}, {5, 0, 3}}, {{5, 1, 0}, {5, 0, 4}}, {{2, 4, 5}, {0, 0, 0}},
    {{2, 5, 4}, {0, 0, 0}}, {{4, 0, 1}, {4, 1, 5}}, {{3, 0, 2}, {3, 2, 5}}, {{1, 5, 3}, {0, 0, 0}},
    {{4, 2, 1}, {4, 1, 3}}, {{0, 3, 4}, {0, 0, 0}}, {{0, 2, 1}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}};
constexpr int kPad = 2;             // OPEN_CLIP_IJK_PADDING (lattice.rs:119)
constexpr double kInsideEps = 1e-9; // is_inside (isosurface.rs:286-289)

// ---- vertex clustering (ferreus_rmt/src/topology.rs; values checked against tests/golden/rmt_cluster_tables.json)
constexpr uint16_t kAll14 = (1u << 14) - 1; // ALL14_MASK
// Table 3: the edges of a sample point that neighbour each edge (NEIGHBOUR_MASKS)
constexpr uint16_t kNeighbourMasks[14] = {0x321A, 0x2015, 0x24B2, 0x0251, 0x006F, 0x00D4, 0x03B8,
                                          0x0D64, 0x0AC0, 0x1949, 0x2884, 0x3780, 0x2A01, 0x1C07};
// Table 4: flat-hole rows, edges OA/OB without and OC/OD with a near intersection (FLAT_HOLE_MASKS)
constexpr uint16_t kFlatHoleMasks[36][2] = {
    {0x0003, 0x2010}, {0x0009, 0x0210}, {0x0011, 0x000A}, {0x0201, 0x1008}, {0x1001, 0x2200}, {0x2001, 0x1002},
    {0x0006, 0x2010}, {0x0012, 0x0005}, {0x2002, 0x0005}, {0x0014, 0x0022}, {0x0024, 0x0090}, {0x0084, 0x0420},
    {0x0404, 0x2080}, {0x2004, 0x0402}, {0x0018, 0x0041}, {0x0048, 0x0210}, {0x0208, 0x0041}, {0x0030, 0x0044},
    {0x0050, 0x0028}, {0x0060, 0x0090}, {0x00A0, 0x0044}, {0x00C0, 0x0120}, {0x0140, 0x0280}, {0x0240, 0x0108},
    {0x0180, 0x0840}, {0x0480, 0x0804}, {0x0880, 0x0500}, {0x0300, 0x0840}, {0x0900, 0x0280}, {0x0A00, 0x1100},
    {0x1200, 0x0801}, {0x0C00, 0x2080}, {0x2400, 0x0804}, {0x1800, 0x2200}, {0x2800, 0x1400}, {0x3000, 0x0801}};

// The cases of test_topology (topology.rs:232-314) in the order of the stats, and the case of a sample point whose 14
// neighbours are not all in E (singletons; the reference evaluates the missing ones instead, isosurface.rs:668-697).
enum TopologyCase : int { kClosed = 0, kMultiHole = 1, kFlatHole = 2, kMultiSurface = 3, kSimple = 4, kIncomplete = 5 };

// A partition of a near mask into clusters: 4 bits per edge, the lowest edge of its cluster, 15 for an edge not in the
// mask.
constexpr uint64_t kNoClusters = ~uint64_t(0);
__host__ __device__ inline int part_label(uint64_t part, int e) { return static_cast<int>((part >> (4 * e)) & 15u); }
__host__ __device__ inline uint64_t part_set(uint64_t part, int e, int label) {
    return (part & ~(uint64_t(15) << (4 * e))) | (uint64_t(label) << (4 * e));
}
__host__ __device__ inline uint16_t part_mask(uint64_t part) { // the edges it holds
    uint16_t m = 0;
    for (int e = 0; e < 14; ++e)
        if (part_label(part, e) != 15) m |= uint16_t(1u << e);
    return m;
}
__host__ __device__ inline uint16_t part_leaders(uint64_t part) { // the lowest edge of every cluster
    uint16_t m = 0;
    for (int e = 0; e < 14; ++e)
        if (part_label(part, e) == e) m |= uint16_t(1u << e);
    return m;
}
__host__ __device__ inline uint64_t part_singletons(uint16_t mask) { // do_not_cluster (topology.rs:224-228)
    uint64_t p = kNoClusters;
    for (int e = 0; e < 14; ++e)
        if (mask & (1u << e)) p = part_set(p, e, e);
    return p;
}
__host__ __device__ inline uint64_t part_one(uint64_t part, uint16_t comp) { // one cluster of the edges of comp
    int lead = 0;
    while (!(comp & (1u << lead))) ++lead;
    for (int e = lead; e < 14; ++e)
        if (comp & (1u << e)) part = part_set(part, e, lead);
    return part;
}

// The component of `seed` (one bit) among the edges of `within` under kNeighbourMasks: a bit-parallel flood of at most
// 14 steps (connected_components_masks, topology.rs:106-133; the components are the same sets whatever the order).
__host__ __device__ inline uint16_t topology_component(uint16_t seed, uint16_t within) {
    uint16_t comp = seed;
    for (int step = 0; step < 14; ++step) {
        uint16_t grow = comp;
        for (int e = 0; e < 14; ++e)
            if (comp & (1u << e)) grow |= kNeighbourMasks[e];
        grow &= within;
        if (grow == comp) break;
        comp = grow;
    }
    return comp;
}

__host__ __device__ inline bool topology_inside(double g) { return g < -1e-9; } // is_inside (topology.rs:156-160)

// crossing_alpha(a, b).is_some_and(|t| t < 0.5) (topology.rs:162-169 with lerp_alpha, isosurface.rs:173-181)
__host__ __device__ inline bool topology_near(double a, double b) {
    if (topology_inside(a) == topology_inside(b)) return false;
    const double den = a - b;
    double t = 0.5;
    if (!((den < 0 ? -den : den) < 1e-30)) {
        t = a / den;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
    return t < 0.5;
}

// is_flat_hole (topology.rs:180-221); v: g at the 14 neighbours, a row that reads a non-finite one is skipped
__host__ __device__ inline bool topology_flat_hole(uint16_t m, const double *v) {
    for (int r = 0; r < 36; ++r) {
        const uint16_t em = kFlatHoleMasks[r][0], om = kFlatHoleMasks[r][1];
        if ((m & em) != 0 || (m & om) != om) continue;
        int ab[2] = {0, 0}, cd[2] = {0, 0}, na = 0, nc = 0;
        for (int e = 0; e < 14; ++e) {
            if ((em >> e) & 1) ab[na++ & 1] = e;
            if ((om >> e) & 1) cd[nc++ & 1] = e;
        }
        if (na != 2 || nc != 2) continue;
        const double a = v[ab[0]], b = v[ab[1]], c = v[cd[0]], d = v[cd[1]];
        // finite: x - x == 0 fails for NaN and the infinities
        if (!(a - a == 0.0) || !(b - b == 0.0) || !(c - c == 0.0) || !(d - d == 0.0)) continue;
        if ((topology_near(a, d) && topology_near(a, c)) || (topology_near(b, d) && topology_near(b, c))) return true;
    }
    return false;
}

// test_topology (topology.rs:232-314) of a near mask with clustering on.  values: g at the 14 neighbours, or null to
// leave out the flat-hole test.  An empty mask is a simple surface without clusters.
__host__ __device__ inline uint64_t topology_partition(uint16_t mask, const double *values, int *case_out) {
    const uint16_t m = mask & kAll14;
    *case_out = kSimple;
    if (m == 0) return kNoClusters;
    if (m == kAll14) {
        *case_out = kClosed;
        return part_singletons(m);
    }
    const uint16_t first = topology_component(uint16_t(m & (~m + 1)), m);
    if (first != m) {
        *case_out = kMultiSurface;
        uint64_t p = kNoClusters;
        uint16_t rest = m;
        while (rest) {
            const uint16_t comp = topology_component(uint16_t(rest & (~rest + 1)), rest);
            p = part_one(p, comp);
            rest = uint16_t(rest & ~comp);
        }
        return p;
    }
    const uint16_t holes = uint16_t(kAll14 & ~m);
    if (topology_component(uint16_t(holes & (~holes + 1)), holes) != holes) {
        *case_out = kMultiHole;
        return part_singletons(m);
    }
    if (values && topology_flat_hole(m, values)) {
        *case_out = kFlatHole;
        return part_singletons(m);
    }
    return part_one(kNoClusters, m);
}

// The extraction domain of (extents, resolution), host-side (SampleLattice::new, lattice.rs:55-96).
struct Lattice {
    double lo_world[3] = {0, 0, 0}, spacing[3] = {0, 0, 0};
    int64_t max_ijk[3] = {0, 0, 0};
    int64_t lo[3] = {0, 0, 0};   // ijk of entry (0, 0, 0) of a field array: the bounding box of E
    int64_t dims[3] = {0, 0, 0}; // ni, nj, nk of that box (arrays are (nk, nj, ni), i fastest)
    int64_t n_keys = 0, n_nodes = 0; // |K| and |E|
    // per row (j, k) of the box (index k * nj + j): the i ranges [begin, end] of E and of the keys (begin > end: none)
    std::vector<int32_t> e_rows, key_rows; // 2 ints per row
    // the world coordinates of the first and the last node of the box on every axis
    void node_box(double *box_lo, double *box_hi) const {
        for (int a = 0; a < 3; ++a) {
            box_lo[a] = lo_world[a] + static_cast<double>(lo[a]) * spacing[a];
            box_hi[a] = lo_world[a] + static_cast<double>(lo[a] + dims[a] - 1) * spacing[a];
        }
    }
};

// Validates (finite extents with lo <= hi, finite resolution > 0, a lattice of at most 2^36 box nodes) and fills *out.
bool make_lattice(const double *extents, double resolution, Lattice *out, std::string *err);

// ---- clip and clean (ferreus_rmt/src/aabb_clipping.rs, mesh_cleanup.rs; DESIGN.md "Clip and clean")
struct ClipBox {
    double lo[3], hi[3];
    double eps; // bbox_eps (aabb_clipping.rs:40-48)
};
// Points a clipped triangle can hold: a convex polygon gains at most one point per plane (9); the slack covers polygons
// that the snapping leaves non-convex by eps.  Points beyond it are not stored.
constexpr int kClipMaxPoints = 12;

__host__ __device__ inline double clip_abs(double x) { return x < 0 ? -x : x; }

// snap_near_bbox (aabb_clipping.rs:148-168)
__host__ __device__ inline void clip_snap_near(double *p, const ClipBox &b) {
    for (int a = 0; a < 3; ++a) {
        if (clip_abs(p[a] - b.lo[a]) <= b.eps) p[a] = b.lo[a];
        if (clip_abs(p[a] - b.hi[a]) <= b.eps) p[a] = b.hi[a];
    }
}

// point_inside_plane (aabb_clipping.rs:216-225); planes XMin, XMax, YMin, YMax, ZMin, ZMax
__host__ __device__ inline bool clip_inside_plane(const double *p, int plane, const ClipBox &b) {
    const int a = plane >> 1;
    return (plane & 1) ? p[a] <= b.hi[a] + b.eps : p[a] >= b.lo[a] - b.eps;
}

// One triangle through clip_polygon_to_plane (aabb_clipping.rs:238-274) for the six planes in order.  Returns the
// number of points of the polygon (0: dropped, fewer than 3 were left); corner[k]: the corner of the triangle that
// point k is a kept copy of, -1 for a point made on a plane.
__host__ __device__ inline int clip_triangle(const double tri[3][3], const ClipBox &b, double out[kClipMaxPoints][3],
                                             int corner[kClipMaxPoints]) {
#pragma clang fp contract(off)
    double buf[2][kClipMaxPoints][3];
    int src[2][kClipMaxPoints];
    int n = 3, cur = 0;
    for (int k = 0; k < 3; ++k) {
        for (int a = 0; a < 3; ++a) buf[0][k][a] = tri[k][a];
        src[0][k] = k;
    }
    for (int plane = 0; plane < 6 && n >= 3; ++plane) {
        const int ax = plane >> 1;
        const double c = (plane & 1) ? b.hi[ax] : b.lo[ax];
        int m = 0;
        const double *prev = buf[cur][n - 1];
        bool prev_in = clip_inside_plane(prev, plane, b);
        for (int i = 0; i < n; ++i) {
            const double *curr = buf[cur][i];
            const bool curr_in = clip_inside_plane(curr, plane, b);
            if (curr_in != prev_in) {
                // segment_plane_t (aabb_clipping.rs:186-213)
                const double da = prev[ax] - c, db = curr[ax] - c;
                bool has = true;
                double t = 0.0;
                if (clip_abs(da) <= b.eps) t = 0.0;
                else if (clip_abs(db) <= b.eps) t = 1.0;
                else if ((da < 0.0) == (db < 0.0)) has = false;
                else t = (c - prev[ax]) / (curr[ax] - prev[ax]);
                if (has && m < kClipMaxPoints) {
                    double *q = buf[cur ^ 1][m];
                    for (int a = 0; a < 3; ++a) q[a] = prev[a] + t * (curr[a] - prev[a]);
                    q[ax] = c; // snap_to_plane
                    clip_snap_near(q, b);
                    src[cur ^ 1][m] = -1;
                    ++m;
                }
            }
            if (curr_in && m < kClipMaxPoints) {
                double *q = buf[cur ^ 1][m];
                for (int a = 0; a < 3; ++a) q[a] = curr[a];
                clip_snap_near(q, b);
                src[cur ^ 1][m] = src[cur][i];
                ++m;
            }
            prev = curr;
            prev_in = curr_in;
        }
        cur ^= 1;
        n = m;
    }
    if (n < 3) return 0;
    for (int k = 0; k < n; ++k) {
        for (int a = 0; a < 3; ++a) out[k][a] = buf[cur][k][a];
        corner[k] = src[cur][k];
    }
    return n;
}

// Mesh::finish_stats
enum FinishStat : int {
    kFinFacetsIn = 0,   // facets of the mesh that was clipped
    kFinStraddling = 1, // kept by the clip with a corner outside the extents
    kFinOutside = 2,    // dropped by the clip
    kFinEmitted = 3,    // vertices the clip emitted (unwelded)
    kFinWelded = 4,     // of those, welded into another
    kFinLoose = 5,      // vertices further than eps from their representative (weld_loose)
    kFinCollapsed = 6,
    kFinTiny = 7,
    kFinDuplicate = 8,
    kFinLone = 9,
    kFinStats = 10
};

// One mesh: row-major vertices (n x 3) and facets (m x 3).
struct Mesh {
    std::vector<double> vertices;
    std::vector<int64_t> facets;
    int64_t stats[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // kStat*, all 0 without clustering
    int64_t finish_stats[kFinStats] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};    // FinishStat, all 0 with kFinishRaw
    int64_t isect_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};                   // IntersectStat, all 0 without the detector
    int64_t curv_stats[4] = {0, 0, 0, 0};                                // CurvStat (isosurface_curvature.hpp), all 0 without kClusterCurvature
    int64_t follow_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};                  // FollowStat, all 0 with kFollowDense
    double follow_ms[3] = {0, 0, 0};                                     // host time of the seed stage, the rounds, the extraction
    int32_t follow_dims[4] = {0, 0, 0, 0};                               // B and the bricks per axis (x, y, z)
    std::vector<uint8_t> follow_bricks;                                  // 1 per brick visited for this isovalue, x fastest
    std::vector<int64_t> isect_ids;                                      // the detector on a caller's mesh: the triangles found
    int64_t closure_stats[32] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // ClosureStat (isosurface_closure.hpp), all 0 without a closure
};

// Mesh::stats: [0, 6) sample points per TopologyCase; mesh edges with more than 2 faces before pass A and the clusters
// pass A split (isosurface.rs:798-878); per round of pass B (isosurface.rs:888-930) the sample points rolled back and
// the mesh edges with more than 2 faces it found.
constexpr int kStatOverA = 6, kStatSplitA = 7, kStatRolledB = 8, kStatOverB = 12, kRoundsB = 4;

enum ClusterMethod : int { kClusterNone = 0, kClusterAverage = 1, kClusterCurvature = 2 };
enum Finish : int { kFinishRaw = 0, kFinishClipped = 1, kFinishClosePositive = 2, kFinishCloseNegative = 3 };
enum SelfIntersections : int { kSelfIntersectionsIgnore = 0, kSelfIntersectionsRollback = 1 };

// ---- self-intersections (ferreus_rmt/src/mesh_intersections.rs; DESIGN.md "Self-intersection rollback")
// Mesh::isect_stats
enum IntersectStat : int {
    kIsectKept = 0,      // facets with all corners inside the extents (all facets without extents)
    kIsectBoxPairs = 1,  // pairs a < b of those with overlapping bounding boxes
    kIsectMoller = 2,    // of those, pairs that tri_tri_intersect accepts
    kIsectTrue = 3,      // of those, true self-intersections
    kIsectTriangles = 4, // triangles on a true pair
    kIsectVertices = 5,  // their vertices that are clusters of several lattice edges
    kIsectRolled = 6,    // sample points rolled back
    kIsectStats = 8      // [7] reserved
};
// The broad phase puts every facet into the cell of its box's lowest corner on a grid of the largest box side and
// probes the 27 cells around it.  A mesh where that is quadratic (one huge triangle among many small ones puts them all
// into a few cells) is refused before any pair is tested: the estimate is the sum over the kept facets of the facets in
// the 27 cells around them, the bound max(kIsectPairFloor, kIsectPairsPerFacet * kept facets).  A mesh of near-uniform
// triangles has some hundreds per facet.
constexpr int64_t kIsectPairFloor = int64_t(1) << 26, kIsectPairsPerFacet = 4096;

// ---- following the surface (ferreus_rmt/src/seed_projection.rs, isosurface.rs:551-697; DESIGN.md "Following the surface")
enum Follow : int { kFollowDense = 0, kFollowSurface = 1 };
// Mesh::follow_stats
enum FollowStat : int {
    kFolSeeds = 0,      // seeds given
    kFolCells = 1,      // distinct seed cells (after the clamp to the extents)
    kFolNewton = 2,     // Newton steps run (evaluations of values and gradients)
    kFolSeedBricks = 3, // bricks of the first frontier
    kFolRounds = 4,     // rounds of the wavefront
    kFolBricks = 5,     // bricks visited for this isovalue
    kFolNodes = 6,      // nodes of E in them
    kFolNodesE = 7,     // nodes of E
    kFolStats = 8
};
// The halo of a crossed edge's ends, in (i, j, k): two edge steps (the topology test at an edge's near end reads that
// sample point's 14 neighbours, and marching resolves every edge of a tetrahedron at its near end).
constexpr int kFollowHalo[3] = {4, 2, 2};
// seed_projection.rs:35-37
constexpr int kSeedNewtonSteps = 30;
constexpr double kSeedTol = 0.01, kSeedG2Min = 1.0e-20;

// world_to_ijk (lattice.rs:98-121) of a point given in fine-grid coordinates p = (world - lo) / spacing: the origin of
// its cell in the basis U, V, W = EDGE_DELTAS[0], [2], [6], whose inverse is written out here (the reference solves by LU).
__host__ __device__ inline void seed_cell(const double p[3], int64_t ijk[3]) {
#pragma clang fp contract(off)
    const double eps = 1e-9;
    const double qa = (p[1] - p[2] - p[0]) * 0.5, qb = (-p[2] - p[0] - p[1]) * 0.5, qc = -p[2];
    const int64_t a = static_cast<int64_t>(floor(qa + eps)), b = static_cast<int64_t>(floor(qb + eps)),
                  c = static_cast<int64_t>(floor(qc + eps));
    ijk[0] = -a - b + c;
    ijk[1] = a - b;
    ijk[2] = -c;
}

// Finite extents with lo <= hi as a ClipBox with its eps; false with *err set otherwise.
bool make_clip_box(const double *extents, ClipBox *out, std::string *err);

// The largest mesh finish_device takes: its vertex and corner ids are packed in 32 bits.
constexpr int64_t kFinishMaxFacets = int64_t(1) << 26, kFinishMaxVertices = (int64_t(1) << 31) - 1;
// false with *err set for a mesh over those limits (checked before any work).
bool finish_fits(int64_t n_vertices, int64_t n_facets, std::string *err);

// clean_mesh(clip_mesh_to_aabb(mesh)) of a mesh on the device (facet ids in [0, n_vertices)), on `stream`; the finished
// mesh and its finish_stats go to *mesh on the host.  close_mode kFinishClosePositive / kFinishCloseNegative: the finished
// mesh stays on the device and goes through closure_device (isosurface_closure.hpp) with close_resolution before that one
// download.  Returns a bbfmm_status.
int finish_device(const double *d_vertices, int64_t n_vertices, const int64_t *d_facets, int64_t n_facets, const ClipBox &box,
                  hipStream_t stream, Mesh *mesh, std::string *err, int close_mode = kFinishClipped, double close_resolution = 0.0);

// The true self-intersections of a mesh on the device (get_intersecting_triangles, mesh_intersections.rs:163-208, with a
// uniform grid in place of the R-tree): d_tri_flag[t] (n_facets bytes, zeroed here) becomes 1 for every facet on a true
// pair, stats[kIsectKept .. kIsectTriangles] are filled.  box: only facets with every corner inside it (slack box->eps,
// facet_fully_inside_aabb) take part; nullptr: all.  At most kFinishMaxFacets facets.  Returns a bbfmm_status.
int self_intersections_device(const double *d_vertices, int64_t n_vertices, const int64_t *d_facets, int64_t n_facets,
                              const ClipBox *box, hipStream_t stream, uint8_t *d_tri_flag, int64_t *stats, std::string *err);

// Field values at m lattice nodes (SoA world coordinates on the device), written to d_vals[0..m) on the stream.
// d_vals == nullptr: only check that every node can be evaluated (BBFMM_POINT_OUTSIDE_TREE otherwise).
using FieldFn = std::function<int(const double *d_x0, const double *d_x1, const double *d_x2, int64_t m, double *d_vals)>;
// The same with gradients: d_grad[a * m + t] = d f / d x_a at point t (seed projection).
using GradFn = std::function<int(const double *d_x0, const double *d_x1, const double *d_x2, int64_t m, double *d_vals, double *d_grad)>;

struct Request {
    const double *isovalues = nullptr;
    int n_iso = 0;
    const double *drift = nullptr;     // 4 values a, b0, b1, b2: a + b . x added to the field (null: none)
    const double *host_field = nullptr; // caller's field over the box of E (then no FieldFn is used)
    double *d_field_out = nullptr;     // device array over the box of E receiving the field (NaN off E), or null
    int64_t budget_bytes = 0;          // device memory for one batch of k-planes (<= 0: the default)
    int cluster = kClusterNone;        // kClusterAverage, kClusterCurvature: the whole lattice field stays on the device (see extract)
    int finish = kFinishRaw;           // kFinishClipped: every mesh goes through finish_device before its download
    const double *extents = nullptr;   // the 6 extents of the lattice, needed with kFinishClipped and the rollback
    int self_intersections = kSelfIntersectionsIgnore; // kSelfIntersectionsRollback: with clustering, one round
    const double *d_field_in = nullptr; // as host_field, already on the device (the field extract_follow filled)
    int follow = kFollowDense;         // kFollowSurface: extract_follow evaluates the bricks a wavefront reaches from the seeds
    const double *seeds = nullptr;     // host, coordinate a of seed s at seeds[a * seeds_ld + s]
    int64_t n_seeds = 0, seeds_ld = 0;
    GradFn grad;                       // values and gradients for the seed projection (empty: central differences of the FieldFn)
};

// Runs the extraction on `stream`.  Returns a bbfmm_status; *err holds the message of a failure.  With kClusterAverage
// the field is evaluated in the same batches but kept over the whole box (40 bytes of state per box node, refused before
// any work where that does not fit), and each isovalue is then clustered and marched over the whole lattice.
// kClusterCurvature is the same with the cluster points weighted by the curvature estimate of every crossed edge
// (isosurface_curvature.hpp; 48 bytes per box node and 8 per crossed edge).
int extract(const Lattice &lat, const FieldFn &field, const Request &req, hipStream_t stream, std::vector<Mesh> *out,
            std::string *err);

// extract() with kFollowSurface (isosurface_follow.hip): the field is evaluated brick by brick along a wavefront from
// the seeds into an array over the box of E that is NaN everywhere else, and every isovalue then goes through the dense
// extraction above on the bricks visited for it.  The brick side comes from BBFMM_ISO_BRICK (4, 8 or 16; default 8).
int extract_follow(const Lattice &lat, const FieldFn &field, const Request &req, hipStream_t stream, std::vector<Mesh> *out,
                   std::string *err);

} // namespace iso
} // namespace bbfmm
