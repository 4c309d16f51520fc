// See isosurface.hpp.  Memory-bound integer and f64 streaming over k-plane slabs of the lattice: one thread per node,
// grid-stride, i fastest so that neighbouring lanes read neighbouring doubles; placement by rocPRIM exclusive scans,
// no atomics.
#include "isosurface.hpp"

#include <algorithm>
#include <limits>

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
#define ISO_HIP(x)                                                                        \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            *err = std::string("isosurface: ") + #x + ": " + hipGetErrorString(e_);      \
            return BBFMM_DEVICE_ERROR;                                                    \
        }                                                                                 \
    } while (0)
    TetTables tt;
    if (!make_tet_tables(&tt)) {
        *err = "isosurface: internal error (a tetrahedron edge is not a lattice edge)";
        return BBFMM_BAD_ARGUMENT;
    }
    const int64_t ni = lat.dims[0], nj = lat.dims[1], nk = lat.dims[2], P = ni * nj;
    const int n_iso = req.n_iso;
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
    if (!req.host_field) {
        for (auto &x : xs) ISO_HIP(pool.get(&x, slab_nodes / 2 + P));
        ISO_HIP(pool.get(&vals, slab_nodes / 2 + P));
    }
    size_t scan_bytes = 0, b2 = 0;
    ISO_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, flag, idx, int32_t(0), slab_nodes, rocprim::plus<int32_t>(), st));
    ISO_HIP(rocprim::exclusive_scan(nullptr, b2, vcnt, voff, int64_t(0), slab_nodes, rocprim::plus<int64_t>(), st));
    scan_bytes = std::max(scan_bytes, b2);
    void *scan_tmp = nullptr;
    ISO_HIP(pool.get(reinterpret_cast<uint8_t **>(&scan_tmp), scan_bytes));
    std::vector<IsoState> states(n_iso);
    for (int q = 0; q < n_iso; ++q) {
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
        if (!req.host_field) {
            node_coords_kernel<<<g, kThreads, 0, st>>>(s, flag, idx, xs[0], xs[1], xs[2]);
            ISO_HIP(hipGetLastError());
        }
        return BBFMM_OK;
    };

    // every node must lie in the tree before any work is done (the reference pads its evaluator by 10 r, rbf.rs:992-998)
    if (!req.host_field) {
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
        if (req.host_field) {
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
        field_kernel<<<g, kThreads, 0, st>>>(s, flag, idx, req.host_field ? nullptr : vals, drift, da, db0, db1, db2, f);
        ISO_HIP(hipGetLastError());
        if (req.d_field_out)
            ISO_HIP(hipMemcpyAsync(req.d_field_out + k0 * P, f + P, s.nodes * sizeof(double), hipMemcpyDeviceToDevice, st));
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
