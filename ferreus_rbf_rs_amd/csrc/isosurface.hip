// See isosurface.hpp.  Memory-bound integer and f64 streaming over k-plane slabs of the lattice: one thread per node,
// grid-stride, i fastest so that neighbouring lanes read neighbouring doubles; placement by rocPRIM exclusive scans,
// no atomics.
#include "isosurface.hpp"
#include "isosurface_curvature.hpp"

#include <algorithm>
#include <limits>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "ferreus_bbfmm_hip.h"

// Coordinates are world(ijk) = lo + ijk * spacing and vertices u + alpha * (v - u), each a multiply and then an add as
// the reference computes them: no fused multiply-add, so that the host restatement reproduces them bit for bit.
#pragma clang fp contract(off)

namespace bbfmm {
namespace iso {

namespace {

constexpr int kThreads = 256;
constexpr int64_t kEvalPlanes = 16; // k-planes per field evaluation (see extract)

// Owner offset (from the key) and label of every edge of every owned tetrahedron (get_edge_owner), and the corner
// offsets of the tetrahedra.
struct TetTables {
    int corner[6][4][3];
    int own[6][6][4]; // dx, dy, dz, label
};

int delta_to_edge(const int d[3]) {
    for (int e = 0; e < 14; ++e)
        if (kEdgeDeltas[e][0] == d[0] && kEdgeDeltas[e][1] == d[1] && kEdgeDeltas[e][2] == d[2]) return e;
    return -1;
}

bool make_tet_tables(TetTables *t) {
    for (int tt = 0; tt < 6; ++tt) {
        for (int a = 0; a < 3; ++a) t->corner[tt][0][a] = 0;
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 3; ++a) t->corner[tt][c + 1][a] = kEdgeDeltas[kOwnedTetEdges[tt][c]][a];
        for (int e = 0; e < 6; ++e) {
            const int *ca = t->corner[tt][kTetEdgePairs[e][0]], *cb = t->corner[tt][kTetEdgePairs[e][1]];
            const int d[3] = {cb[0] - ca[0], cb[1] - ca[1], cb[2] - ca[2]};
            const int eid = delta_to_edge(d);
            if (eid < 0) return false;
            const int *o = eid < 7 ? ca : cb;
            for (int a = 0; a < 3; ++a) t->own[tt][e][a] = o[a];
            t->own[tt][e][3] = eid < 7 ? eid : kReverseEdge[eid];
        }
    }
    return true;
}

// The slab of one batch: planes [k0 - 1, k1) of the box, plane s = 0 the halo carried from the previous batch.
struct Slab {
    int32_t ni, nj;
    int64_t P;       // ni * nj
    int64_t k0;      // box plane of slab plane 1
    int64_t nodes;   // nb * P: the nodes of planes [k0, k1), n = (s - 1) * P + j * ni + i
    int64_t lo[3];   // ijk of box entry (0, 0, 0)
    double lo_world[3], spacing[3];
    const int32_t *e_rows, *key_rows; // per row of the box: i range [begin, end]
};

__device__ __forceinline__ bool in_range(const int32_t *rows, int64_t row, int32_t i) {
    return i >= rows[2 * row] && i <= rows[2 * row + 1];
}

__device__ __forceinline__ double world(const Slab &s, int a, int64_t ijk) { return s.lo_world[a] + static_cast<double>(ijk) * s.spacing[a]; }

// flag[n] = node n is in E (sample points only)
__global__ __launch_bounds__(kThreads) void node_flags_kernel(Slab s, int32_t *__restrict__ flag) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        const int64_t kb = s.k0 + n / s.P, r = n % s.P;
        const int32_t j = static_cast<int32_t>(r / s.ni), i = static_cast<int32_t>(r % s.ni);
        const bool even = ((i + j + kb + s.lo[0] + s.lo[1] + s.lo[2]) & 1) == 0;
        flag[n] = even && in_range(s.e_rows, kb * s.nj + j, i) ? 1 : 0;
    }
}

// the compacted world coordinates of the nodes of E (SoA)
__global__ __launch_bounds__(kThreads) void node_coords_kernel(Slab s, const int32_t *__restrict__ flag, const int32_t *__restrict__ idx,
                                                                double *__restrict__ x0, double *__restrict__ x1, double *__restrict__ x2) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        if (!flag[n]) continue;
        const int64_t kb = s.k0 + n / s.P, r = n % s.P;
        const int64_t j = r / s.ni, i = r % s.ni;
        const int32_t t = idx[n];
        x0[t] = world(s, 0, s.lo[0] + i);
        x1[t] = world(s, 1, s.lo[1] + j);
        x2[t] = world(s, 2, s.lo[2] + kb);
    }
}

// field of slab planes 1..nb: the evaluated value plus the drift at the nodes of E, the caller's value there (vals ==
// nullptr: already in place), NaN everywhere else
__global__ __launch_bounds__(kThreads) void field_kernel(Slab s, const int32_t *__restrict__ flag, const int32_t *__restrict__ idx,
                                                         const double *__restrict__ vals, bool drift, double a, double b0, double b1,
                                                         double b2, double *__restrict__ f) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        double v = __builtin_nan("");
        if (flag[n]) {
            if (vals) {
                v = vals[idx[n]];
                if (drift) {
                    const int64_t kb = s.k0 + n / s.P, r = n % s.P;
                    const int64_t j = r / s.ni, i = r % s.ni;
                    const double d = a + b0 * world(s, 0, s.lo[0] + i) + b1 * world(s, 1, s.lo[1] + j) + b2 * world(s, 2, s.lo[2] + kb);
                    v = v + d;
                }
            } else {
                v = f[s.P + n];
            }
        }
        f[s.P + n] = v;
    }
}

__device__ __forceinline__ bool inside(double g) { return g < -kInsideEps; }

// Per node of planes [k0, k1): crossing mask of its 7 owned edges and their count; per key: triangles of its 6 tetrahedra.
__global__ __launch_bounds__(kThreads) void classify_kernel(Slab s, TetTables tt, const double *__restrict__ f, double iso,
                                                            uint8_t *__restrict__ mask, int32_t *__restrict__ vcnt,
                                                            int32_t *__restrict__ fcnt) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        const int64_t sp = n / s.P + 1, r = n % s.P; // slab plane
        const int32_t j = static_cast<int32_t>(r / s.ni), i = static_cast<int32_t>(r % s.ni);
        const int64_t kb = s.k0 + sp - 1;
        const double g0 = f[sp * s.P + r] - iso;
        uint32_t m = 0;
        int32_t nt = 0;
        if (isfinite(g0)) { // in E (NaN elsewhere), hence a sample point
            const bool in0 = inside(g0);
            for (int l = 0; l < 7; ++l) {
                const int32_t qi = i + kEdgeDeltas[l][0], qj = j + kEdgeDeltas[l][1];
                if (qi < 0 || qi >= s.ni || qj < 0 || qj >= s.nj) continue;
                const double g1 = f[(sp + kEdgeDeltas[l][2]) * s.P + int64_t(qj) * s.ni + qi] - iso;
                if (isfinite(g1) && inside(g1) != in0) m |= 1u << l;
            }
            if (in_range(s.key_rows, kb * s.nj + j, i)) {
                for (int t = 0; t < 6; ++t) {
                    int c = 0;
                    bool ok = true;
                    for (int q = 0; q < 4; ++q) {
                        const int32_t qi = i + tt.corner[t][q][0], qj = j + tt.corner[t][q][1];
                        if (qi < 0 || qi >= s.ni || qj < 0 || qj >= s.nj) { ok = false; break; }
                        const double g = f[(sp + tt.corner[t][q][2]) * s.P + int64_t(qj) * s.ni + qi] - iso;
                        if (!isfinite(g)) { ok = false; break; }
                        if (inside(g)) c |= 1 << q;
                    }
                    if (ok) nt += kMtCount[c];
                }
            }
        }
        mask[sp * s.P + r] = static_cast<uint8_t>(m);
        vcnt[n] = __popc(m);
        fcnt[n] = nt;
    }
}

// Vertex ids of the slab's nodes (vbase: global id of a node's first vertex) and the vertices they own.
__global__ __launch_bounds__(kThreads) void vertices_kernel(Slab s, const double *__restrict__ f, double iso, const uint8_t *__restrict__ mask,
                                                            const int64_t *__restrict__ voff, int64_t vtotal, int64_t *__restrict__ vbase,
                                                            double *__restrict__ out) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        const int64_t sp = n / s.P + 1, r = n % s.P;
        const int64_t vb = vtotal + voff[n];
        vbase[sp * s.P + r] = vb;
        uint32_t m = mask[sp * s.P + r];
        if (!m) continue;
        const int64_t j = r / s.ni, i = r % s.ni, kb = s.k0 + sp - 1;
        const int64_t p[3] = {s.lo[0] + i, s.lo[1] + j, s.lo[2] + kb};
        const double gp = f[sp * s.P + r] - iso;
        int64_t v = vb;
        for (int l = 0; l < 7; ++l) {
            if (!(m & (1u << l))) continue;
            const int64_t qi = i + kEdgeDeltas[l][0], qj = j + kEdgeDeltas[l][1];
            const double gq = f[(sp + kEdgeDeltas[l][2]) * s.P + qj * s.ni + qi] - iso;
            const int64_t q[3] = {p[0] + kEdgeDeltas[l][0], p[1] + kEdgeDeltas[l][1], p[2] + kEdgeDeltas[l][2]};
            // the end that holds the intersection (isosurface.rs:599-610), then edge_intersection_point from it
            const double t = gp / (gp - gq);
            const bool own = t < 0.5;
            const int64_t *u = own ? p : q, *w = own ? q : p;
            const double gu = own ? gp : gq, gw = own ? gq : gp;
            const double den = gu - gw;
            double alpha = 0.5;
            if (!(fabs(den) < 1e-30)) { // lerp_alpha (isosurface.rs:173-181): f64::clamp(0, 1)
                alpha = gu / den;
                alpha = alpha < 0.0 ? 0.0 : (alpha > 1.0 ? 1.0 : alpha);
            }
            for (int a = 0; a < 3; ++a) {
                const double wu = world(s, a, u[a]), ww = world(s, a, w[a]);
                out[3 * v + a] = wu + alpha * (ww - wu);
            }
            ++v;
        }
    }
}

// The triangles of each key: tetrahedra 0..5, table rows in order (march_tets, isosurface.rs:224-283).
__global__ __launch_bounds__(kThreads) void facets_kernel(Slab s, TetTables tt, const double *__restrict__ f, double iso,
                                                          const uint8_t *__restrict__ mask, const int64_t *__restrict__ vbase,
                                                          const int32_t *__restrict__ fcnt, const int64_t *__restrict__ foff,
                                                          int64_t ftotal, int64_t *__restrict__ out) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        if (!fcnt[n]) continue;
        const int64_t sp = n / s.P + 1, r = n % s.P;
        const int32_t j = static_cast<int32_t>(r / s.ni), i = static_cast<int32_t>(r % s.ni);
        int64_t o = ftotal + foff[n];
        for (int t = 0; t < 6; ++t) {
            int c = 0;
            bool ok = true;
            for (int q = 0; q < 4; ++q) {
                const int32_t qi = i + tt.corner[t][q][0], qj = j + tt.corner[t][q][1];
                if (qi < 0 || qi >= s.ni || qj < 0 || qj >= s.nj) { ok = false; break; }
                const double g = f[(sp + tt.corner[t][q][2]) * s.P + int64_t(qj) * s.ni + qi] - iso;
                if (!isfinite(g)) { ok = false; break; }
                if (inside(g)) c |= 1 << q;
            }
            if (!ok) continue;
            for (int row = 0; row < kMtCount[c]; ++row) {
                for (int e3 = 0; e3 < 3; ++e3) {
                    const int *ow = tt.own[t][kMtTable[c][row][e3]];
                    const int64_t on = (sp + ow[2]) * s.P + int64_t(j + ow[1]) * s.ni + (i + ow[0]);
                    const uint32_t m = mask[on];
                    out[3 * o + e3] = vbase[on] + __popc(m & ((1u << ow[3]) - 1u));
                }
                ++o;
            }
        }
    }
}

// ---- vertex clustering (Request::cluster == kClusterAverage).  The slab is the whole box: field plane s = k + 1 with a
// NaN plane below and above, the per-node arrays (part, ccnt, vbase, fcnt) indexed by n = k * P + j * ni + i.

__device__ __forceinline__ int64_t edge_step(const Slab &s, int e) {
    return kEdgeDeltas[e][2] * s.P + int64_t(kEdgeDeltas[e][1]) * s.ni + kEdgeDeltas[e][0];
}

// lerp_alpha (isosurface.rs:173-181)
__device__ __forceinline__ double lerp_alpha(double gu, double gw) {
    const double den = gu - gw;
    if (fabs(den) < 1e-30) return 0.5;
    const double a = gu / den;
    return a < 0.0 ? 0.0 : (a > 1.0 ? 1.0 : a);
}

// Per node: the near mask N(p) of its 14 edges (isosurface.rs:588-610) and its partition by test_topology.
__global__ __launch_bounds__(kThreads) void near_topology_kernel(Slab s, int64_t nk, const double *__restrict__ f, double iso,
                                                                  uint64_t *__restrict__ part, int32_t *__restrict__ ccnt,
                                                                  unsigned long long *__restrict__ stats) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        const int64_t k = n / s.P, r = n % s.P;
        const int32_t j = static_cast<int32_t>(r / s.ni), i = static_cast<int32_t>(r % s.ni);
        const double gp = f[s.P + n] - iso;
        uint64_t p = kNoClusters;
        if (isfinite(gp)) { // in E (NaN elsewhere), hence a sample point
            const bool inp = inside(gp);
            double v[14];
            uint32_t m = 0;
            bool complete = true;
            for (int e = 0; e < 14; ++e) {
                const int32_t qi = i + kEdgeDeltas[e][0], qj = j + kEdgeDeltas[e][1];
                const int64_t qk = k + kEdgeDeltas[e][2];
                v[e] = __builtin_nan("");
                if (qi < 0 || qi >= s.ni || qj < 0 || qj >= s.nj || qk < 0 || qk >= nk || !in_range(s.e_rows, qk * s.nj + qj, qi)) {
                    complete = false;
                    continue;
                }
                const double gq = f[s.P + n + edge_step(s, e)] - iso;
                v[e] = gq;
                if (!isfinite(gq) || inside(gq) == inp) continue;
                // t from the owner of the edge: p for e < 7, the neighbour otherwise
                const bool near_p = e < 7 ? gp / (gp - gq) < 0.5 : !(gq / (gq - gp) < 0.5);
                if (near_p) m |= 1u << e;
            }
            if (m) {
                int c = kIncomplete;
                p = complete ? topology_partition(static_cast<uint16_t>(m), v, &c) : part_singletons(static_cast<uint16_t>(m));
                atomicAdd(&stats[c], 1ull); // a count only: nothing is placed by it
            }
        }
        part[n] = p;
        ccnt[n] = __popc(part_leaders(p));
    }
}

// The candidate point of every cluster, at the vertex ids the scan gave (vbase) (isosurface.rs:738-796): the intersection of a single
// edge, the mean of several (average_point, isosurface.rs:183-192).  vinfo: node << 5 | lowest edge << 1 | several edges.
__global__ __launch_bounds__(kThreads) void candidates_kernel(Slab s, const double *__restrict__ f, double iso, const uint64_t *__restrict__ part,
                                                               const int64_t *__restrict__ vbase, double *__restrict__ out,
                                                               int64_t *__restrict__ vinfo) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        int64_t v = vbase[n];
        const uint64_t p = part[n];
        if (p == kNoClusters) continue;
        const int64_t k = n / s.P, r = n % s.P;
        const int64_t ijk[3] = {s.lo[0] + r % s.ni, s.lo[1] + r / s.ni, s.lo[2] + k};
        const double gp = f[s.P + n] - iso;
        for (int lead = 0; lead < 14; ++lead) {
            if (part_label(p, lead) != lead) continue;
            double sum[3] = {0.0, 0.0, 0.0}, one[3] = {0.0, 0.0, 0.0};
            int cnt = 0;
            for (int e = lead; e < 14; ++e) {
                if (part_label(p, e) != lead) continue;
                const double gq = f[s.P + n + edge_step(s, e)] - iso;
                const double alpha = lerp_alpha(gp, gq);
                for (int a = 0; a < 3; ++a) {
                    const double wu = world(s, a, ijk[a]), ww = world(s, a, ijk[a] + kEdgeDeltas[e][a]);
                    one[a] = wu + alpha * (ww - wu);
                    sum[a] = sum[a] + one[a];
                }
                ++cnt;
            }
            const double inv = 1.0 / static_cast<double>(cnt);
            for (int a = 0; a < 3; ++a) out[3 * v + a] = cnt == 1 ? one[a] : sum[a] * inv;
            vinfo[v] = (n << 5) | (int64_t(lead) << 1) | (cnt > 1 ? 1 : 0);
            ++v;
        }
    }
}

// ---- curvature-weighted clusters (Request::cluster == kClusterCurvature; DESIGN.md "Curvature-weighted clusters").
// A crossed edge is in exactly one near mask, at its near end, so the edges of all masks in node order are every crossed
// edge once: ebase (the scan of the masks' sizes) numbers them, and their weights are computed once per isovalue, one
// thread per edge, whatever the partition becomes afterwards.

__global__ __launch_bounds__(kThreads) void edge_count_kernel(Slab s, const uint64_t *__restrict__ part, int32_t *__restrict__ ecnt) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads)
        ecnt[n] = __popc(part_mask(part[n]));
}

// The list of crossed edges, node << 4 | edge, written where the edge's weight will be.
__global__ __launch_bounds__(kThreads) void edge_list_kernel(Slab s, const uint64_t *__restrict__ part, const int64_t *__restrict__ ebase,
                                                              int64_t *__restrict__ list) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        const uint64_t p = part[n];
        if (p == kNoClusters) continue;
        int64_t o = ebase[n];
        for (int e = 0; e < 14; ++e)
            if (part_label(p, e) != 15) list[o++] = (n << 4) | e;
    }
}

// f - isovalue around one sample point of the resident field: NaN for a neighbour outside the box of E or off E (a node
// of E that was not evaluated, or a non-finite value, is refused by the weight function itself).
struct OwnerField {
    const Slab &s;
    const double *__restrict__ f;
    double iso;
    int64_t nk, n; // the owner's box index
    int32_t i, j;
    int64_t k;
    __device__ double operator()(int e) const {
        if (e < 0) return f[s.P + n] - iso;
        const int32_t qi = i + kEdgeDeltas[e][0], qj = j + kEdgeDeltas[e][1];
        const int64_t qk = k + kEdgeDeltas[e][2];
        if (qi < 0 || qi >= s.ni || qj < 0 || qj >= s.nj || qk < 0 || qk >= nk || !in_range(s.e_rows, qk * s.nj + qj, qi))
            return __builtin_nan("");
        return f[s.P + n + edge_step(s, e)] - iso;
    }
};

// One thread per crossed edge: its list entry becomes its weight (curvature_weight_for_edge(..).unwrap_or(1.0),
// curvature_weighting.rs:259).  The owner of edge e of node n is n for e < 7 and the other end otherwise, which lies in
// the box because the edge was crossed.
__global__ __launch_bounds__(kThreads) void curvature_weights_kernel(Slab s, int64_t nk, const double *__restrict__ f, double iso, CurvTrig trig,
                                                                      int64_t n_edges, double *__restrict__ weights,
                                                                      unsigned long long *__restrict__ n_fallback) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < n_edges; t += int64_t(gridDim.x) * kThreads) {
        const int64_t entry = reinterpret_cast<const int64_t *>(weights)[t];
        int e = static_cast<int>(entry & 15);
        int64_t n = entry >> 4;
        if (e >= 7) {
            n += edge_step(s, e);
            e = kReverseEdge[e];
        }
        const int64_t k = n / s.P, r = n % s.P;
        const OwnerField get{s, f, iso, nk, n, static_cast<int32_t>(r % s.ni), static_cast<int32_t>(r / s.ni), k};
        const int64_t ijk[3] = {s.lo[0] + r % s.ni, s.lo[1] + r / s.ni, s.lo[2] + k};
        double w = 1.0;
        if (!curvature_weight(get, ijk, e, s.lo_world, s.spacing, trig, &w)) {
            w = 1.0;
            atomicAdd(n_fallback, 1ull); // a count only
        }
        weights[t] = w;
    }
}

// candidates_kernel with curvature_weighted_cluster_point (curvature_weighting.rs:242-276) for every cluster, those of
// one edge too: the sum of w * p and of w in ascending edge order, then the sum times 1 / sum of w; a sum of w of EPS or
// less falls back to the candidate of candidates_kernel.
__global__ __launch_bounds__(kThreads) void candidates_curvature_kernel(Slab s, const double *__restrict__ f, double iso,
                                                                         const uint64_t *__restrict__ part, const int64_t *__restrict__ vbase,
                                                                         const int64_t *__restrict__ ebase, const double *__restrict__ weights,
                                                                         double *__restrict__ out, int64_t *__restrict__ vinfo,
                                                                         unsigned long long *__restrict__ n_fallback) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        int64_t v = vbase[n];
        const uint64_t p = part[n];
        if (p == kNoClusters) continue;
        const int64_t k = n / s.P, r = n % s.P;
        const int64_t ijk[3] = {s.lo[0] + r % s.ni, s.lo[1] + r / s.ni, s.lo[2] + k};
        const double gp = f[s.P + n] - iso;
        const uint32_t mask = part_mask(p);
        const int64_t eb = ebase[n];
        for (int lead = 0; lead < 14; ++lead) {
            if (part_label(p, lead) != lead) continue;
            double sum[3] = {0.0, 0.0, 0.0}, one[3] = {0.0, 0.0, 0.0}, wsum[3] = {0.0, 0.0, 0.0}, total = 0.0;
            int cnt = 0;
            for (int e = lead; e < 14; ++e) {
                if (part_label(p, e) != lead) continue;
                const double gq = f[s.P + n + edge_step(s, e)] - iso;
                const double alpha = lerp_alpha(gp, gq);
                const double w = weights[eb + __popc(mask & ((1u << e) - 1u))];
                for (int a = 0; a < 3; ++a) {
                    const double wu = world(s, a, ijk[a]), ww = world(s, a, ijk[a] + kEdgeDeltas[e][a]);
                    one[a] = wu + alpha * (ww - wu);
                    sum[a] = sum[a] + one[a];
                    wsum[a] = wsum[a] + one[a] * w;
                }
                total = total + w;
                ++cnt;
            }
            if (total <= kCurvEps) {
                const double inv = 1.0 / static_cast<double>(cnt);
                for (int a = 0; a < 3; ++a) out[3 * v + a] = cnt == 1 ? one[a] : sum[a] * inv;
                atomicAdd(n_fallback, 1ull); // a count only
            } else {
                const double inv = 1.0 / total;
                for (int a = 0; a < 3; ++a) out[3 * v + a] = wsum[a] * inv;
            }
            vinfo[v] = (n << 5) | (int64_t(lead) << 1) | (cnt > 1 ? 1 : 0);
            ++v;
        }
    }
}

// The vertex of the cluster that holds the owned edge `lab` of node `on` at its near end; -1: none.
__device__ __forceinline__ int64_t resolve_cluster(const Slab &s, const uint64_t *__restrict__ part, const int64_t *__restrict__ vbase,
                                                   int64_t on, int lab) {
    uint64_t p = part[on];
    int l = part_label(p, lab);
    if (l == 15) {
        on += edge_step(s, lab);
        p = part[on];
        l = part_label(p, kReverseEdge[lab]);
        if (l == 15) return -1;
    }
    return vbase[on] + __popc(part_leaders(p) & ((1u << l) - 1u));
}

// march_tets (isosurface.rs:224-283) of the key at node n with clustered vertices; degenerate triangles are dropped.
template <class Emit>
__device__ __forceinline__ void march_key(const Slab &s, const TetTables &tt, const double *__restrict__ f, double iso,
                                          const uint64_t *__restrict__ part, const int64_t *__restrict__ vbase, int64_t n, Emit emit) {
    const int64_t r = n % s.P;
    const int32_t j = static_cast<int32_t>(r / s.ni), i = static_cast<int32_t>(r % s.ni);
    for (int t = 0; t < 6; ++t) {
        int c = 0;
        bool ok = true;
        for (int q = 0; q < 4; ++q) {
            const int32_t qi = i + tt.corner[t][q][0], qj = j + tt.corner[t][q][1];
            if (qi < 0 || qi >= s.ni || qj < 0 || qj >= s.nj) { ok = false; break; }
            const double g = f[s.P + n + tt.corner[t][q][2] * s.P + int64_t(tt.corner[t][q][1]) * s.ni + tt.corner[t][q][0]] - iso;
            if (!isfinite(g)) { ok = false; break; }
            if (inside(g)) c |= 1 << q;
        }
        if (!ok) continue;
        for (int row = 0; row < kMtCount[c]; ++row) {
            int64_t id[3];
            for (int e3 = 0; e3 < 3; ++e3) {
                const int *ow = tt.own[t][kMtTable[c][row][e3]];
                id[e3] = resolve_cluster(s, part, vbase, n + ow[2] * s.P + int64_t(ow[1]) * s.ni + ow[0], ow[3]);
            }
            if (id[0] < 0 || id[1] < 0 || id[2] < 0 || id[0] == id[1] || id[1] == id[2] || id[0] == id[2]) continue;
            emit(id);
        }
    }
}

__device__ __forceinline__ bool is_key(const Slab &s, const double *__restrict__ f, int64_t n) {
    if (!isfinite(f[s.P + n])) return false;
    const int64_t r = n % s.P;
    return in_range(s.key_rows, (n / s.P) * s.nj + r / s.ni, static_cast<int32_t>(r % s.ni));
}

__global__ __launch_bounds__(kThreads) void cluster_count_kernel(Slab s, TetTables tt, const double *__restrict__ f, double iso,
                                                                  const uint64_t *__restrict__ part, const int64_t *__restrict__ vbase,
                                                                  int32_t *__restrict__ fcnt) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        int32_t c = 0;
        if (is_key(s, f, n)) march_key(s, tt, f, iso, part, vbase, n, [&](const int64_t *) { ++c; });
        fcnt[n] = c;
    }
}

__global__ __launch_bounds__(kThreads) void cluster_facets_kernel(Slab s, TetTables tt, const double *__restrict__ f, double iso,
                                                                   const uint64_t *__restrict__ part, const int64_t *__restrict__ vbase,
                                                                   const int32_t *__restrict__ fcnt, const int64_t *__restrict__ foff,
                                                                   int64_t *__restrict__ out) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        if (!fcnt[n]) continue;
        int64_t o = foff[n];
        march_key(s, tt, f, iso, part, vbase, n, [&](const int64_t *id) {
            for (int a = 0; a < 3; ++a) out[3 * o + a] = id[a];
            ++o;
        });
    }
}

// The 3 undirected edges of every facet as keys min << 32 | max, the facet as their value.
__global__ __launch_bounds__(kThreads) void facet_edges_kernel(int64_t nf, const int64_t *__restrict__ facets, uint64_t *__restrict__ keys,
                                                                int64_t *__restrict__ vals) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nf; t += int64_t(gridDim.x) * kThreads) {
        for (int a = 0; a < 3; ++a) {
            const uint64_t u = static_cast<uint64_t>(facets[3 * t + a]), w = static_cast<uint64_t>(facets[3 * t + (a + 1) % 3]);
            keys[3 * t + a] = u < w ? (u << 32 | w) : (w << 32 | u);
            vals[3 * t + a] = t;
        }
    }
}

// Over the sorted edges: an entry of a run of more than 2 equal keys is a face on an over-used mesh edge.  Pass A
// (isosurface.rs:840-851) flags the edge's two vertices, pass B (collect_invalid_topology_cluster_owners,
// isosurface.rs:326-356) the three of the face; only clusters of several edges count.  Plain stores of one value.
__global__ __launch_bounds__(kThreads) void flag_over_used_kernel(int64_t m, const uint64_t *__restrict__ keys, const int64_t *__restrict__ vals,
                                                                   const int64_t *__restrict__ facets, const int64_t *__restrict__ vinfo,
                                                                   bool pass_b, uint8_t *__restrict__ vflag, int32_t *__restrict__ found,
                                                                   unsigned long long *__restrict__ n_over) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < m; i += int64_t(gridDim.x) * kThreads) {
        const uint64_t k = keys[i];
        const bool lo1 = i >= 1 && keys[i - 1] == k, lo2 = i >= 2 && keys[i - 2] == k;
        const bool hi1 = i + 1 < m && keys[i + 1] == k, hi2 = i + 2 < m && keys[i + 2] == k;
        if (!(hi2 || (lo1 && hi1) || lo2)) continue;
        if (!lo1) atomicAdd(n_over, 1ull); // a count only
        int64_t v[3];
        int nv = 2;
        if (pass_b) {
            nv = 3;
            for (int a = 0; a < 3; ++a) v[a] = facets[3 * vals[i] + a];
        } else {
            v[0] = static_cast<int64_t>(k >> 32);
            v[1] = static_cast<int64_t>(k & 0xffffffffull);
        }
        for (int a = 0; a < nv; ++a)
            if (vinfo[v[a]] & 1) {
                vflag[v[a]] = pass_b ? 2 : 1;
                *found = 1;
            }
    }
}

// Pass A: a flagged cluster becomes singletons.  Pass B (rollback_cluster_owners, isosurface.rs:359-395): every cluster
// of a sample point that owns a flagged one does.
__global__ __launch_bounds__(kThreads) void split_clusters_kernel(Slab s, const int64_t *__restrict__ vbase, const uint8_t *__restrict__ vflag,
                                                                   uint64_t *__restrict__ part, int32_t *__restrict__ ccnt,
                                                                   unsigned long long *__restrict__ n_split, unsigned long long *__restrict__ n_rolled) {
    for (int64_t n = blockIdx.x * int64_t(kThreads) + threadIdx.x; n < s.nodes; n += int64_t(gridDim.x) * kThreads) {
        if (!ccnt[n]) continue;
        uint64_t p = part[n];
        const uint64_t before = p;
        int64_t v = vbase[n];
        bool roll = false;
        int split = 0;
        for (int lead = 0; lead < 14; ++lead) {
            if (part_label(before, lead) != lead) continue;
            const uint8_t fl = vflag[v++];
            if (fl == 2) roll = true;
            if (fl != 1) continue;
            ++split;
            for (int e = lead + 1; e < 14; ++e)
                if (part_label(before, e) == lead) p = part_set(p, e, e);
        }
        if (roll) {
            p = part_singletons(part_mask(before));
            atomicAdd(n_rolled, 1ull);
        } else if (split) {
            atomicAdd(n_split, static_cast<unsigned long long>(split));
        }
        if (p != before) {
            part[n] = p;
            ccnt[n] = __popc(part_leaders(p));
        }
    }
}

// The self-intersection rollback (isosurface.rs:959-974): the vertices of the triangles on a true self-intersection
// that are clusters of several edges are flagged as pass B flags them, so that split_clusters_kernel rolls the sample
// points that own them back.  Plain stores of one value.
__global__ __launch_bounds__(kThreads) void flag_intersecting_kernel(int64_t nf, const uint8_t *__restrict__ tri_flag,
                                                                      const int64_t *__restrict__ facets, const int64_t *__restrict__ vinfo,
                                                                      uint8_t *__restrict__ vflag, int32_t *__restrict__ found) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nf; t += int64_t(gridDim.x) * kThreads) {
        if (!tri_flag[t]) continue;
        for (int a = 0; a < 3; ++a) {
            const int64_t v = facets[3 * t + a];
            if (vinfo[v] & 1) {
                vflag[v] = 2;
                *found = 1;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void count_flagged_kernel(int64_t nv, const uint8_t *__restrict__ vflag, unsigned long long *__restrict__ n) {
    for (int64_t v = blockIdx.x * int64_t(kThreads) + threadIdx.x; v < nv; v += int64_t(gridDim.x) * kThreads)
        if (vflag[v]) atomicAdd(n, 1ull); // a count only
}

int grid_for(int64_t n) {
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 4096)));
}

// Device allocations of one extract() call, freed on every exit.
struct Pool {
    std::vector<void *> ptrs;
    ~Pool() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <class T> hipError_t get(T **p, size_t n) {
        *p = nullptr;
        if (n == 0) n = 1;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(p), n * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
    template <class T> void put(T *p) {
        auto it = std::find(ptrs.begin(), ptrs.end(), static_cast<void *>(p));
        if (it != ptrs.end()) {
            (void)hipFree(p);
            ptrs.erase(it);
        }
    }
};

// A device array that grows by doubling, the ids it holds kept (vertices and facets of one isovalue).
template <class T> struct Growing {
    T *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(Pool &pool, size_t n, size_t used, hipStream_t st) {
        if (n <= cap) return hipSuccess;
        size_t c = std::max<size_t>(n, cap * 2);
        T *q = nullptr;
        hipError_t e = pool.get(&q, c);
        if (e != hipSuccess) return e;
        if (used) e = hipMemcpyAsync(q, p, used * sizeof(T), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return e;
        e = hipStreamSynchronize(st);
        if (e != hipSuccess) return e;
        pool.put(p);
        p = q;
        cap = c;
        return hipSuccess;
    }
};

struct IsoState {
    double iso = 0;
    uint8_t *mask = nullptr; // slab planes 0..nb
    int64_t *vbase = nullptr;
    int64_t vtotal = 0, ftotal = 0;
    Growing<double> v;
    Growing<int64_t> fc;
};

#define ISO_HIP(x)                                                                        \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            *err = std::string("isosurface: ") + #x + ": " + hipGetErrorString(e_);      \
            return BBFMM_DEVICE_ERROR;                                                    \
        }                                                                                 \
    } while (0)

// Bytes per box node of the clustered extraction: the field (8), the partition (8), cluster and facet counts (4 + 4),
// their scans (8 + 8); with kClusterCurvature also the scan that numbers the crossed edges (8).
constexpr int64_t kClusterNodeBytes = 40, kCurvatureNodeBytes = 48;

// The per-node state of the clustered extraction, shared by the isovalues of a call.
struct ClusterState {
    double *f = nullptr; // (nk + 2) planes: NaN below and above
    uint64_t *part = nullptr;
    int32_t *ccnt = nullptr, *fcnt = nullptr;
    int64_t *vbase = nullptr, *foff = nullptr;
    void *scan_tmp = nullptr;
    size_t scan_bytes = 0;
    unsigned long long *d_stats = nullptr; // 16 counters, then kIsectVertices and kIsectRolled of the rollback, then CurvStat
    int32_t *d_found = nullptr;
    int64_t *ebase = nullptr; // kClusterCurvature: the first crossed edge of every node
};
constexpr int kStatCurv = 18, kStatCount = kStatCurv + kCurvStats;

// The clustered mesh of one isovalue of the resident field (DESIGN.md "Isosurfaces on the RMT lattice", clustering).
// inside: the extents of the self-intersection rollback, nullptr without it.
int cluster_extract(const Slab &s, int64_t nk, const TetTables &tt, const ClusterState &c, double iso, const ClipBox *clip,
                    const ClipBox *inside, Pool &pool, hipStream_t st, Mesh *mesh, std::string *err, int finish = kFinishClipped,
                    double resolution = 0.0) {
    const int g = grid_for(s.nodes);
    const size_t nodes = static_cast<size_t>(s.nodes);
    ISO_HIP(hipMemsetAsync(c.d_stats, 0, kStatCount * sizeof(unsigned long long), st));
    near_topology_kernel<<<g, kThreads, 0, st>>>(s, nk, c.f, iso, c.part, c.ccnt, c.d_stats);
    ISO_HIP(hipGetLastError());
    // the weights of the crossed edges: once, the near masks do not change below
    double *weights = nullptr;
    int64_t n_edges = 0;
    if (c.ebase) {
        edge_count_kernel<<<g, kThreads, 0, st>>>(s, c.part, c.fcnt);
        ISO_HIP(hipGetLastError());
        size_t bytes = c.scan_bytes;
        ISO_HIP(rocprim::exclusive_scan(c.scan_tmp, bytes, c.fcnt, c.ebase, int64_t(0), nodes, rocprim::plus<int64_t>(), st));
        int64_t last = 0;
        int32_t lastc = 0;
        ISO_HIP(hipMemcpyAsync(&last, c.ebase + s.nodes - 1, 8, hipMemcpyDeviceToHost, st));
        ISO_HIP(hipMemcpyAsync(&lastc, c.fcnt + s.nodes - 1, 4, hipMemcpyDeviceToHost, st));
        ISO_HIP(hipStreamSynchronize(st));
        n_edges = last + lastc;
        ISO_HIP(pool.get(&weights, static_cast<size_t>(n_edges)));
        if (n_edges > 0) {
            edge_list_kernel<<<g, kThreads, 0, st>>>(s, c.part, c.ebase, reinterpret_cast<int64_t *>(weights));
            ISO_HIP(hipGetLastError());
            curvature_weights_kernel<<<grid_for(n_edges), kThreads, 0, st>>>(s, nk, c.f, iso, curvature_trig(), n_edges, weights,
                                                                             c.d_stats + kStatCurv + kCurvEdgeFallback);
            ISO_HIP(hipGetLastError());
        }
    }
    double *verts = nullptr;
    int64_t *vinfo = nullptr, *facets = nullptr;
    uint8_t *vflag = nullptr;
    int64_t nv = 0, nf = 0;
    // candidates and facets of the current partition
    auto march = [&]() -> int {
        pool.put(verts);
        pool.put(vinfo);
        pool.put(facets);
        pool.put(vflag);
        size_t bytes = c.scan_bytes;
        ISO_HIP(rocprim::exclusive_scan(c.scan_tmp, bytes, c.ccnt, c.vbase, int64_t(0), nodes, rocprim::plus<int64_t>(), st));
        int64_t last = 0;
        int32_t lastc = 0;
        ISO_HIP(hipMemcpyAsync(&last, c.vbase + s.nodes - 1, 8, hipMemcpyDeviceToHost, st));
        ISO_HIP(hipMemcpyAsync(&lastc, c.ccnt + s.nodes - 1, 4, hipMemcpyDeviceToHost, st));
        ISO_HIP(hipStreamSynchronize(st));
        nv = last + lastc;
        if (nv >= (int64_t(1) << 32)) {
            *err = "isosurface: " + std::to_string(nv) + " clusters, mesh edges are keyed by two 32-bit vertex ids (use a coarser resolution)";
            return BBFMM_BAD_ARGUMENT;
        }
        ISO_HIP(pool.get(&verts, 3 * static_cast<size_t>(nv)));
        ISO_HIP(pool.get(&vinfo, static_cast<size_t>(nv)));
        ISO_HIP(pool.get(&vflag, static_cast<size_t>(nv)));
        if (c.ebase) {
            ISO_HIP(hipMemsetAsync(c.d_stats + kStatCurv + kCurvClusterFallback, 0, sizeof(unsigned long long), st));
            candidates_curvature_kernel<<<g, kThreads, 0, st>>>(s, c.f, iso, c.part, c.vbase, c.ebase, weights, verts, vinfo,
                                                                c.d_stats + kStatCurv + kCurvClusterFallback);
        } else {
            candidates_kernel<<<g, kThreads, 0, st>>>(s, c.f, iso, c.part, c.vbase, verts, vinfo);
        }
        ISO_HIP(hipGetLastError());
        cluster_count_kernel<<<g, kThreads, 0, st>>>(s, tt, c.f, iso, c.part, c.vbase, c.fcnt);
        ISO_HIP(hipGetLastError());
        bytes = c.scan_bytes;
        ISO_HIP(rocprim::exclusive_scan(c.scan_tmp, bytes, c.fcnt, c.foff, int64_t(0), nodes, rocprim::plus<int64_t>(), st));
        ISO_HIP(hipMemcpyAsync(&last, c.foff + s.nodes - 1, 8, hipMemcpyDeviceToHost, st));
        ISO_HIP(hipMemcpyAsync(&lastc, c.fcnt + s.nodes - 1, 4, hipMemcpyDeviceToHost, st));
        ISO_HIP(hipStreamSynchronize(st));
        nf = last + lastc;
        ISO_HIP(pool.get(&facets, 3 * static_cast<size_t>(nf)));
        cluster_facets_kernel<<<g, kThreads, 0, st>>>(s, tt, c.f, iso, c.part, c.vbase, c.fcnt, c.foff, facets);
        ISO_HIP(hipGetLastError());
        return BBFMM_OK;
    };
    int rc = march();
    if (rc != BBFMM_OK) return rc;
    // round 0: pass A (predicted edges); rounds 1..4: pass B (non-manifold rollback).  Both split clusters of the
    // partition and march again; the host only learns whether a round flagged anything.
    for (int round = 0; round <= kRoundsB && nf > 0; ++round) {
        const size_t m = 3 * static_cast<size_t>(nf);
        uint64_t *k_in = nullptr, *k_out = nullptr;
        int64_t *v_in = nullptr, *v_out = nullptr;
        uint8_t *tmp = nullptr;
        ISO_HIP(pool.get(&k_in, m));
        ISO_HIP(pool.get(&k_out, m));
        ISO_HIP(pool.get(&v_in, m));
        ISO_HIP(pool.get(&v_out, m));
        size_t tmp_bytes = 0;
        ISO_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, k_in, k_out, v_in, v_out, m, 0, 64, st));
        ISO_HIP(pool.get(&tmp, tmp_bytes));
        facet_edges_kernel<<<grid_for(nf), kThreads, 0, st>>>(nf, facets, k_in, v_in);
        ISO_HIP(hipGetLastError());
        ISO_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, k_in, k_out, v_in, v_out, m, 0, 64, st));
        ISO_HIP(hipMemsetAsync(vflag, 0, static_cast<size_t>(std::max<int64_t>(nv, 1)), st));
        ISO_HIP(hipMemsetAsync(c.d_found, 0, sizeof(int32_t), st));
        const bool pass_b = round > 0;
        flag_over_used_kernel<<<grid_for(static_cast<int64_t>(m)), kThreads, 0, st>>>(
            static_cast<int64_t>(m), k_out, v_out, facets, vinfo, pass_b, vflag, c.d_found,
            c.d_stats + (pass_b ? kStatOverB + round - 1 : kStatOverA));
        ISO_HIP(hipGetLastError());
        int32_t found = 0;
        ISO_HIP(hipMemcpyAsync(&found, c.d_found, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        ISO_HIP(hipStreamSynchronize(st));
        pool.put(k_in);
        pool.put(k_out);
        pool.put(v_in);
        pool.put(v_out);
        pool.put(tmp);
        if (!found) {
            if (pass_b) break;
            continue;
        }
        split_clusters_kernel<<<g, kThreads, 0, st>>>(s, c.vbase, vflag, c.part, c.ccnt, c.d_stats + kStatSplitA,
                                                      c.d_stats + kStatRolledB + (pass_b ? round - 1 : 0));
        ISO_HIP(hipGetLastError());
        if ((rc = march()) != BBFMM_OK) return rc;
    }
    // The self-intersection rollback (isosurface.rs:932-1007), one round: the triangles on true self-intersections among
    // the facets inside the extents, their vertices that are clusters of several edges, the sample points that own those:
    // pass B's update, and one more march.  Nothing flagged: the mesh stays as it is.
    if (inside && nf > 0) {
        uint8_t *tri_flag = nullptr;
        ISO_HIP(pool.get(&tri_flag, static_cast<size_t>(nf)));
        if ((rc = self_intersections_device(verts, nv, facets, nf, inside, st, tri_flag, mesh->isect_stats, err)) != BBFMM_OK) return rc;
        if (mesh->isect_stats[kIsectTriangles] > 0) {
            ISO_HIP(hipMemsetAsync(vflag, 0, static_cast<size_t>(std::max<int64_t>(nv, 1)), st));
            ISO_HIP(hipMemsetAsync(c.d_found, 0, sizeof(int32_t), st));
            flag_intersecting_kernel<<<grid_for(nf), kThreads, 0, st>>>(nf, tri_flag, facets, vinfo, vflag, c.d_found);
            ISO_HIP(hipGetLastError());
            count_flagged_kernel<<<grid_for(nv), kThreads, 0, st>>>(nv, vflag, c.d_stats + 16);
            ISO_HIP(hipGetLastError());
            int32_t found = 0;
            ISO_HIP(hipMemcpyAsync(&found, c.d_found, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            ISO_HIP(hipStreamSynchronize(st));
            pool.put(tri_flag);
            if (found) {
                split_clusters_kernel<<<g, kThreads, 0, st>>>(s, c.vbase, vflag, c.part, c.ccnt, c.d_stats + kStatSplitA, c.d_stats + 17);
                ISO_HIP(hipGetLastError());
                if ((rc = march()) != BBFMM_OK) return rc;
            }
        } else {
            pool.put(tri_flag);
        }
    }
    unsigned long long h_stats[kStatCount];
    ISO_HIP(hipMemcpyAsync(h_stats, c.d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, st));
    const auto curvature_stats = [&]() { // after the stream is synchronised
        if (!c.ebase) return;
        mesh->curv_stats[kCurvEdges] = n_edges;
        mesh->curv_stats[kCurvEdgeFallback] = static_cast<int64_t>(h_stats[kStatCurv + kCurvEdgeFallback]);
        mesh->curv_stats[kCurvClusters] = nv;
        mesh->curv_stats[kCurvClusterFallback] = static_cast<int64_t>(h_stats[kStatCurv + kCurvClusterFallback]);
    };
    if (clip) { // clipped and cleaned while still on the device
        ISO_HIP(hipStreamSynchronize(st));
        for (int q = 0; q < 16; ++q) mesh->stats[q] = static_cast<int64_t>(h_stats[q]);
        mesh->isect_stats[kIsectVertices] = static_cast<int64_t>(h_stats[16]);
        mesh->isect_stats[kIsectRolled] = static_cast<int64_t>(h_stats[17]);
        curvature_stats();
        pool.put(weights);
        pool.put(vinfo);
        pool.put(vflag);
        rc = finish_device(verts, nv, facets, nf, *clip, st, mesh, err, finish, resolution);
        pool.put(verts);
        pool.put(facets);
        return rc;
    }
    mesh->vertices.resize(3 * static_cast<size_t>(nv));
    mesh->facets.resize(3 * static_cast<size_t>(nf));
    if (nv) ISO_HIP(hipMemcpyAsync(mesh->vertices.data(), verts, mesh->vertices.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (nf) ISO_HIP(hipMemcpyAsync(mesh->facets.data(), facets, mesh->facets.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ISO_HIP(hipStreamSynchronize(st));
    for (int q = 0; q < 16; ++q) mesh->stats[q] = static_cast<int64_t>(h_stats[q]);
    mesh->isect_stats[kIsectVertices] = static_cast<int64_t>(h_stats[16]);
    mesh->isect_stats[kIsectRolled] = static_cast<int64_t>(h_stats[17]);
    curvature_stats();
    pool.put(weights);
    pool.put(verts);
    pool.put(vinfo);
    pool.put(facets);
    pool.put(vflag);
    return BBFMM_OK;
}

} // namespace

bool make_lattice(const double *extents, double resolution, Lattice *out, std::string *err) {
    if (!extents) {
        *err = "isosurface: extents must not be null";
        return false;
    }
    for (int a = 0; a < 6; ++a)
        if (!std::isfinite(extents[a])) {
            *err = "isosurface: extents must be finite";
            return false;
        }
    for (int a = 0; a < 3; ++a)
        if (extents[a + 3] < extents[a]) {
            *err = "isosurface: inverted extents (max < min on axis " + std::to_string(a) + ")";
            return false;
        }
    if (!std::isfinite(resolution) || !(resolution > 0.0)) {
        *err = "isosurface: resolution must be finite and > 0";
        return false;
    }
    Lattice L;
    const double s2 = std::sqrt(2.0); // std::f64::consts::SQRT_2, correctly rounded
    L.spacing[0] = resolution / 2.0;
    L.spacing[1] = (resolution * s2) / 2.0;
    L.spacing[2] = resolution / s2;
    for (int a = 0; a < 3; ++a) {
        const double c = std::ceil((extents[a + 3] - extents[a]) / L.spacing[a]);
        if (!(c < 1e9)) {
            *err = "isosurface: lattice too large for these extents and resolution";
            return false;
        }
        L.max_ijk[a] = static_cast<int64_t>(c);
        L.lo_world[a] = extents[a];
    }
    L.max_ijk[0] += 1;
    // corner offsets of a key: 0 and EDGE_DELTAS[0..7)
    int dmin[3] = {0, 0, 0}, dmax[3] = {0, 0, 0};
    for (int e = 0; e < 7; ++e)
        for (int a = 0; a < 3; ++a) {
            dmin[a] = std::min(dmin[a], kEdgeDeltas[e][a]);
            dmax[a] = std::max(dmax[a], kEdgeDeltas[e][a]);
        }
    int64_t blo[3], bhi[3], klo[3], khi[3];
    for (int a = 0; a < 3; ++a) {
        blo[a] = -kPad;
        bhi[a] = L.max_ijk[a] + kPad;
        klo[a] = blo[a] - dmax[a];
        khi[a] = bhi[a] - dmin[a];
        L.lo[a] = klo[a] + dmin[a];
        L.dims[a] = khi[a] + dmax[a] - L.lo[a] + 1;
    }
    const int64_t ni = L.dims[0], nj = L.dims[1], nk = L.dims[2];
    if (static_cast<double>(ni) * nj * nk > static_cast<double>(int64_t(1) << 36) || ni * nj >= (int64_t(1) << 30)) {
        *err = "isosurface: lattice too large for these extents and resolution";
        return false;
    }
    const int64_t rows = nj * nk;
    L.key_rows.assign(2 * rows, 0);
    L.e_rows.assign(2 * rows, 0);
    auto count_parity = [](int64_t a, int64_t b, int64_t par) -> int64_t { // i in [a, b] with (i + par) even
        if (b < a) return 0;
        const int64_t first = ((a + par) & 1) ? a + 1 : a;
        return first > b ? 0 : (b - first) / 2 + 1;
    };
    // keys: c with c + d in [blo, bhi] for a corner d; per row the union of the i ranges [blo - di, bhi - di] of the
    // corners whose (j, k) fit -- one interval, as those ranges are longer than their spread
    std::vector<int64_t> kb(rows), ke(rows);
    for (int64_t k = 0; k < nk; ++k)
        for (int64_t j = 0; j < nj; ++j) {
            const int64_t aj = L.lo[1] + j, ak = L.lo[2] + k, row = k * nj + j;
            int64_t b = std::numeric_limits<int64_t>::max(), e = std::numeric_limits<int64_t>::min();
            for (int c = 0; c < 8; ++c) {
                const int *d = c == 0 ? nullptr : kEdgeDeltas[c - 1];
                const int dx = d ? d[0] : 0, dy = d ? d[1] : 0, dz = d ? d[2] : 0;
                if (aj + dy < blo[1] || aj + dy > bhi[1] || ak + dz < blo[2] || ak + dz > bhi[2]) continue;
                b = std::min<int64_t>(b, blo[0] - dx);
                e = std::max<int64_t>(e, bhi[0] - dx);
            }
            kb[row] = b;
            ke[row] = e;
            if (b <= e) L.n_keys += count_parity(b, e, aj + ak);
            L.key_rows[2 * row] = static_cast<int32_t>(b <= e ? b - L.lo[0] : 1);
            L.key_rows[2 * row + 1] = static_cast<int32_t>(b <= e ? e - L.lo[0] : 0);
        }
    // E: p = c + d for a key c; per row the union of the key ranges of rows (j - dy, k - dz) shifted by dx
    for (int64_t k = 0; k < nk; ++k)
        for (int64_t j = 0; j < nj; ++j) {
            const int64_t row = k * nj + j;
            std::vector<std::pair<int64_t, int64_t>> iv;
            for (int c = 0; c < 8; ++c) {
                const int *d = c == 0 ? nullptr : kEdgeDeltas[c - 1];
                const int dx = d ? d[0] : 0, dy = d ? d[1] : 0, dz = d ? d[2] : 0;
                const int64_t sj = j - dy, sk = k - dz;
                if (sj < 0 || sj >= nj || sk < 0 || sk >= nk) continue;
                const int64_t r2 = sk * nj + sj;
                if (kb[r2] <= ke[r2]) iv.push_back({kb[r2] + dx, ke[r2] + dx});
            }
            std::sort(iv.begin(), iv.end());
            int64_t b = 1, e = 0;
            if (!iv.empty()) {
                b = iv[0].first;
                e = iv[0].second;
                for (size_t q = 1; q < iv.size(); ++q) {
                    if (iv[q].first > e + 1) {
                        *err = "isosurface: internal error (E is not one i range per row)";
                        return false;
                    }
                    e = std::max(e, iv[q].second);
                }
                L.n_nodes += count_parity(b, e, L.lo[1] + j + L.lo[2] + k);
                b -= L.lo[0];
                e -= L.lo[0];
            }
            L.e_rows[2 * row] = static_cast<int32_t>(b);
            L.e_rows[2 * row + 1] = static_cast<int32_t>(e);
        }
    *out = std::move(L);
    return true;
}

int extract(const Lattice &lat, const FieldFn &field, const Request &req, hipStream_t st, std::vector<Mesh> *meshes,
            std::string *err) {
    if (req.follow == kFollowSurface) return extract_follow(lat, field, req, st, meshes, err);
    if (req.follow != kFollowDense) {
        *err = "isosurface: unknown follow mode " + std::to_string(req.follow);
        return BBFMM_BAD_ARGUMENT;
    }
    TetTables tt;
    if (!make_tet_tables(&tt)) {
        *err = "isosurface: internal error (a tetrahedron edge is not a lattice edge)";
        return BBFMM_BAD_ARGUMENT;
    }
    const bool given = req.host_field || req.d_field_in; // the field is the caller's
    const int64_t ni = lat.dims[0], nj = lat.dims[1], nk = lat.dims[2], P = ni * nj;
    const int n_iso = req.n_iso;
    const bool cluster = req.cluster != kClusterNone, curvature = req.cluster == kClusterCurvature;
    if (cluster && req.cluster != kClusterAverage && !curvature) {
        *err = "isosurface: unknown cluster method " + std::to_string(req.cluster);
        return BBFMM_BAD_ARGUMENT;
    }
    const bool clipped = req.finish == kFinishClipped || req.finish == kFinishClosePositive || req.finish == kFinishCloseNegative;
    const double resolution = lat.spacing[0] * 2.0; // (make_lattice halves it: exact both ways)
    if (req.finish != kFinishRaw && !clipped) {
        *err = "isosurface: unknown finish " + std::to_string(req.finish);
        return BBFMM_BAD_ARGUMENT;
    }
    if (req.self_intersections != kSelfIntersectionsIgnore && req.self_intersections != kSelfIntersectionsRollback) {
        *err = "isosurface: unknown self-intersection handling " + std::to_string(req.self_intersections);
        return BBFMM_BAD_ARGUMENT;
    }
    const bool rollback = cluster && req.self_intersections == kSelfIntersectionsRollback; // nothing to roll back without clusters
    ClipBox clip_box;
    if ((clipped || rollback) && !make_clip_box(req.extents, &clip_box, err)) return BBFMM_BAD_ARGUMENT;
    // bytes per k-plane: field, flags, indices, targets and the evaluator's per-target buffers; per isovalue masks,
    // vertex ids, counts and offsets
    const int64_t per_plane = P * (8 + 4 + 4 + 128 + 40 * static_cast<int64_t>(n_iso));
    const int64_t budget = req.budget_bytes > 0 ? req.budget_bytes : (int64_t(1) << 31);
    // The leaf pass's value at a node depends, in its last bits, on which other targets share its call (the layout of
    // the near-field jobs), so the field is evaluated in groups of G k-planes fixed by the lattice alone and a batch
    // holds whole groups: the meshes do not depend on the budget.
    const int64_t plane_cap = std::max<int64_t>(1, ((int64_t(1) << 31) - 1) / P - 1);
    const int64_t G = std::min<int64_t>({kEvalPlanes, plane_cap, nk});
    int64_t nb = budget / std::max<int64_t>(per_plane, 1);
    nb = std::max<int64_t>(G, std::min<int64_t>(nb, std::min(nk, plane_cap)) / G * G);

    // Clustering looks at the whole mesh, so the field of every batch is kept and the extraction runs once over the whole
    // lattice: refused before any work where that state does not fit.
    if (cluster) {
        size_t free_b = 0, total_b = 0;
        ISO_HIP(hipMemGetInfo(&free_b, &total_b));
        const int64_t node_bytes = curvature ? kCurvatureNodeBytes : kClusterNodeBytes;
        const double need = static_cast<double>(node_bytes) * static_cast<double>(nk + 2) * static_cast<double>(P) +
                            static_cast<double>(per_plane) * static_cast<double>(nb);
        if (need > static_cast<double>(free_b)) {
            *err = std::string("isosurface: cluster=") + (curvature ? "curvature" : "average") + " keeps " + std::to_string(node_bytes) + " bytes per node of the " +
                   std::to_string(ni) + " x " + std::to_string(nj) + " x " + std::to_string(nk) + " lattice box on the device, about " +
                   std::to_string(static_cast<int64_t>(need / 1048576.0)) + " MiB with one batch; " +
                   std::to_string(free_b / 1048576) + " MiB are free (use a coarser resolution or smaller extents)";
            return BBFMM_BAD_ARGUMENT;
        }
    }
    Pool pool;
    int32_t *d_erows = nullptr, *d_krows = nullptr, *flag = nullptr, *idx = nullptr, *vcnt = nullptr, *fcnt = nullptr;
    double *f = nullptr, *xs[3] = {nullptr, nullptr, nullptr}, *vals = nullptr;
    int64_t *voff = nullptr, *foff = nullptr;
    ISO_HIP(pool.get(&d_erows, lat.e_rows.size()));
    ISO_HIP(pool.get(&d_krows, lat.key_rows.size()));
    ISO_HIP(hipMemcpyAsync(d_erows, lat.e_rows.data(), lat.e_rows.size() * 4, hipMemcpyHostToDevice, st));
    ISO_HIP(hipMemcpyAsync(d_krows, lat.key_rows.data(), lat.key_rows.size() * 4, hipMemcpyHostToDevice, st));
    const size_t slab_nodes = static_cast<size_t>(nb * P);
    ISO_HIP(pool.get(&f, slab_nodes + P));
    ISO_HIP(pool.get(&flag, slab_nodes));
    ISO_HIP(pool.get(&idx, slab_nodes));
    ISO_HIP(pool.get(&vcnt, slab_nodes));
    ISO_HIP(pool.get(&fcnt, slab_nodes));
    ISO_HIP(pool.get(&voff, slab_nodes));
    ISO_HIP(pool.get(&foff, slab_nodes));
    if (!given) {
        for (auto &x : xs) ISO_HIP(pool.get(&x, slab_nodes / 2 + P));
        ISO_HIP(pool.get(&vals, slab_nodes / 2 + P));
    }
    size_t scan_bytes = 0, b2 = 0;
    ISO_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, flag, idx, int32_t(0), slab_nodes, rocprim::plus<int32_t>(), st));
    ISO_HIP(rocprim::exclusive_scan(nullptr, b2, vcnt, voff, int64_t(0), slab_nodes, rocprim::plus<int64_t>(), st));
    scan_bytes = std::max(scan_bytes, b2);
    void *scan_tmp = nullptr;
    ISO_HIP(pool.get(reinterpret_cast<uint8_t **>(&scan_tmp), scan_bytes));
    ClusterState cs;
    if (cluster) {
        const size_t box = static_cast<size_t>(nk * P);
        ISO_HIP(pool.get(&cs.f, box + 2 * P));
        ISO_HIP(pool.get(&cs.part, box));
        ISO_HIP(pool.get(&cs.ccnt, box));
        ISO_HIP(pool.get(&cs.fcnt, box));
        ISO_HIP(pool.get(&cs.vbase, box));
        ISO_HIP(pool.get(&cs.foff, box));
        ISO_HIP(pool.get(&cs.d_stats, kStatCount));
        if (curvature) ISO_HIP(pool.get(&cs.ebase, box));
        ISO_HIP(pool.get(&cs.d_found, 1));
        ISO_HIP(rocprim::exclusive_scan(nullptr, cs.scan_bytes, cs.ccnt, cs.vbase, int64_t(0), box, rocprim::plus<int64_t>(), st));
        ISO_HIP(pool.get(reinterpret_cast<uint8_t **>(&cs.scan_tmp), cs.scan_bytes));
    }
    std::vector<IsoState> states(cluster ? 0 : n_iso);
    for (int q = 0; q < static_cast<int>(states.size()); ++q) {
        states[q].iso = req.isovalues[q];
        ISO_HIP(pool.get(&states[q].mask, slab_nodes + P));
        ISO_HIP(pool.get(&states[q].vbase, slab_nodes + P));
        ISO_HIP(hipMemsetAsync(states[q].mask, 0, P, st)); // plane k = -1: nothing
        ISO_HIP(hipMemsetAsync(states[q].vbase, 0, P * sizeof(int64_t), st));
    }
    // plane k = -1: no nodes (NaN)
    {
        std::vector<double> nan_plane(static_cast<size_t>(P), std::numeric_limits<double>::quiet_NaN());
        ISO_HIP(hipMemcpyAsync(f, nan_plane.data(), P * sizeof(double), hipMemcpyHostToDevice, st));
        if (cluster) { // planes k = -1 and k = nk of the resident field
            ISO_HIP(hipMemcpyAsync(cs.f, nan_plane.data(), P * sizeof(double), hipMemcpyHostToDevice, st));
            ISO_HIP(hipMemcpyAsync(cs.f + (nk + 1) * P, nan_plane.data(), P * sizeof(double), hipMemcpyHostToDevice, st));
        }
        ISO_HIP(hipStreamSynchronize(st)); // (pageable source)
    }
    int64_t *h_tot = nullptr;
    ISO_HIP(hipHostMalloc(reinterpret_cast<void **>(&h_tot), 4 * sizeof(int64_t)));
    struct PinnedFree {
        int64_t *p;
        ~PinnedFree() { (void)hipHostFree(p); }
    } pin_guard{h_tot};

    auto slab_for = [&](int64_t k0, int64_t k1) {
        Slab s;
        s.ni = static_cast<int32_t>(ni);
        s.nj = static_cast<int32_t>(nj);
        s.P = P;
        s.k0 = k0;
        s.nodes = (k1 - k0) * P;
        for (int a = 0; a < 3; ++a) {
            s.lo[a] = lat.lo[a];
            s.lo_world[a] = lat.lo_world[a];
            s.spacing[a] = lat.spacing[a];
        }
        s.e_rows = d_erows;
        s.key_rows = d_krows;
        return s;
    };
    // E nodes of planes [k0, k1) compacted into xs; returns their count
    auto gather_nodes = [&](const Slab &s, int64_t *m_out) -> int {
        const int g = grid_for(s.nodes);
        node_flags_kernel<<<g, kThreads, 0, st>>>(s, flag);
        ISO_HIP(hipGetLastError());
        size_t bytes = scan_bytes;
        ISO_HIP(rocprim::exclusive_scan(scan_tmp, bytes, flag, idx, int32_t(0), static_cast<size_t>(s.nodes), rocprim::plus<int32_t>(), st));
        int32_t last[2];
        ISO_HIP(hipMemcpyAsync(&last[0], idx + s.nodes - 1, 4, hipMemcpyDeviceToHost, st));
        ISO_HIP(hipMemcpyAsync(&last[1], flag + s.nodes - 1, 4, hipMemcpyDeviceToHost, st));
        ISO_HIP(hipStreamSynchronize(st));
        *m_out = static_cast<int64_t>(last[0]) + last[1];
        if (!given) {
            node_coords_kernel<<<g, kThreads, 0, st>>>(s, flag, idx, xs[0], xs[1], xs[2]);
            ISO_HIP(hipGetLastError());
        }
        return BBFMM_OK;
    };

    // every node must lie in the tree before any work is done (the reference pads its evaluator by 10 r, rbf.rs:992-998)
    if (!given) {
        for (int64_t k0 = 0; k0 < nk; k0 += nb) {
            const Slab s = slab_for(k0, std::min(nk, k0 + nb));
            int64_t m = 0;
            int rc = gather_nodes(s, &m);
            if (rc != BBFMM_OK) return rc;
            if (m > 0 && (rc = field(xs[0], xs[1], xs[2], m, nullptr)) != BBFMM_OK) return rc;
        }
    }

    const bool drift = req.drift != nullptr;
    const double da = drift ? req.drift[0] : 0, db0 = drift ? req.drift[1] : 0, db1 = drift ? req.drift[2] : 0,
                 db2 = drift ? req.drift[3] : 0;
    for (int64_t k0 = 0; k0 < nk; k0 += nb) {
        const int64_t k1 = std::min(nk, k0 + nb), nbc = k1 - k0;
        const Slab s = slab_for(k0, k1);
        const int g = grid_for(s.nodes);
        int64_t m = 0;
        int rc = gather_nodes(s, &m);
        if (rc != BBFMM_OK) return rc;
        if (req.d_field_in) {
            ISO_HIP(hipMemcpyAsync(f + P, req.d_field_in + k0 * P, s.nodes * sizeof(double), hipMemcpyDeviceToDevice, st));
        } else if (req.host_field) {
            ISO_HIP(hipMemcpyAsync(f + P, req.host_field + k0 * P, s.nodes * sizeof(double), hipMemcpyHostToDevice, st));
        } else if (m > 0) {
            // one call per group of G planes: the group's nodes are a contiguous range of the compacted arrays
            std::vector<int32_t> start((nbc + G - 1) / G + 1, 0);
            for (size_t q = 1; q + 1 < start.size(); ++q)
                ISO_HIP(hipMemcpyAsync(&start[q], idx + static_cast<int64_t>(q) * G * P, 4, hipMemcpyDeviceToHost, st));
            ISO_HIP(hipStreamSynchronize(st));
            start.back() = static_cast<int32_t>(m);
            for (size_t q = 0; q + 1 < start.size(); ++q) {
                const int64_t b = start[q], c = start[q + 1] - start[q];
                if (c > 0 && (rc = field(xs[0] + b, xs[1] + b, xs[2] + b, c, vals + b)) != BBFMM_OK) return rc;
            }
        }
        field_kernel<<<g, kThreads, 0, st>>>(s, flag, idx, given ? nullptr : vals, drift, da, db0, db1, db2, f);
        ISO_HIP(hipGetLastError());
        if (req.d_field_out)
            ISO_HIP(hipMemcpyAsync(req.d_field_out + k0 * P, f + P, s.nodes * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (cluster) ISO_HIP(hipMemcpyAsync(cs.f + (k0 + 1) * P, f + P, s.nodes * sizeof(double), hipMemcpyDeviceToDevice, st));
        for (IsoState &is : states) {
            classify_kernel<<<g, kThreads, 0, st>>>(s, tt, f, is.iso, is.mask, vcnt, fcnt);
            ISO_HIP(hipGetLastError());
            size_t bytes = scan_bytes;
            ISO_HIP(rocprim::exclusive_scan(scan_tmp, bytes, vcnt, voff, int64_t(0), static_cast<size_t>(s.nodes), rocprim::plus<int64_t>(), st));
            bytes = scan_bytes;
            ISO_HIP(rocprim::exclusive_scan(scan_tmp, bytes, fcnt, foff, int64_t(0), static_cast<size_t>(s.nodes), rocprim::plus<int64_t>(), st));
            int32_t lastc[2];
            ISO_HIP(hipMemcpyAsync(&h_tot[0], voff + s.nodes - 1, 8, hipMemcpyDeviceToHost, st));
            ISO_HIP(hipMemcpyAsync(&h_tot[1], foff + s.nodes - 1, 8, hipMemcpyDeviceToHost, st));
            ISO_HIP(hipMemcpyAsync(&lastc[0], vcnt + s.nodes - 1, 4, hipMemcpyDeviceToHost, st));
            ISO_HIP(hipMemcpyAsync(&lastc[1], fcnt + s.nodes - 1, 4, hipMemcpyDeviceToHost, st));
            ISO_HIP(hipStreamSynchronize(st));
            const int64_t nv = h_tot[0] + lastc[0], nf = h_tot[1] + lastc[1];
            ISO_HIP(is.v.reserve(pool, 3 * static_cast<size_t>(is.vtotal + nv), 3 * static_cast<size_t>(is.vtotal), st));
            ISO_HIP(is.fc.reserve(pool, 3 * static_cast<size_t>(is.ftotal + nf), 3 * static_cast<size_t>(is.ftotal), st));
            vertices_kernel<<<g, kThreads, 0, st>>>(s, f, is.iso, is.mask, voff, is.vtotal, is.vbase, is.v.p);
            ISO_HIP(hipGetLastError());
            facets_kernel<<<g, kThreads, 0, st>>>(s, tt, f, is.iso, is.mask, is.vbase, fcnt, foff, is.ftotal, is.fc.p);
            ISO_HIP(hipGetLastError());
            is.vtotal += nv;
            is.ftotal += nf;
            // the last plane becomes the next batch's halo
            ISO_HIP(hipMemcpyAsync(is.mask, is.mask + nbc * P, P, hipMemcpyDeviceToDevice, st));
            ISO_HIP(hipMemcpyAsync(is.vbase, is.vbase + nbc * P, P * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        }
        ISO_HIP(hipMemcpyAsync(f, f + nbc * P, P * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    meshes->assign(n_iso, Mesh());
    if (cluster) {
        const Slab box = slab_for(0, nk);
        for (int q = 0; q < n_iso; ++q) {
            const int rc = cluster_extract(box, nk, tt, cs, req.isovalues[q], clipped ? &clip_box : nullptr, rollback ? &clip_box : nullptr,
                                           pool, st, &(*meshes)[q], err, req.finish, resolution);
            if (rc != BBFMM_OK) return rc;
        }
        return BBFMM_OK;
    }
    if (clipped) { // clipped and cleaned while still on the device
        for (int q = 0; q < n_iso; ++q) {
            const int rc = finish_device(states[q].v.p, states[q].vtotal, states[q].fc.p, states[q].ftotal, clip_box, st, &(*meshes)[q], err, req.finish,
                                          resolution);
            if (rc != BBFMM_OK) return rc;
        }
        return BBFMM_OK;
    }
    for (int q = 0; q < n_iso; ++q) {
        Mesh &mh = (*meshes)[q];
        mh.vertices.resize(3 * static_cast<size_t>(states[q].vtotal));
        mh.facets.resize(3 * static_cast<size_t>(states[q].ftotal));
        if (!mh.vertices.empty())
            ISO_HIP(hipMemcpyAsync(mh.vertices.data(), states[q].v.p, mh.vertices.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        if (!mh.facets.empty())
            ISO_HIP(hipMemcpyAsync(mh.facets.data(), states[q].fc.p, mh.facets.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    ISO_HIP(hipStreamSynchronize(st));
    return BBFMM_OK;
#undef ISO_HIP
}

} // namespace iso
} // namespace bbfmm
