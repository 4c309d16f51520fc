// Clip and clean of an extracted mesh on the device (isosurface.hpp, finish_device): clip_mesh_to_aabb
// (ferreus_rmt/src/aabb_clipping.rs:55-105) and clean_mesh (mesh_cleanup.rs:32-96).  One thread per facet or vertex,
// grid-stride; placement by rocPRIM exclusive scans and stable radix sorts.  The integer atomics (minimum over indices,
// use counts, stats) are order-independent, so the mesh does not depend on thread order.
#include "isosurface.hpp"
#include "isosurface_closure.hpp"

#include <algorithm>
#include <cmath>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "ferreus_bbfmm_hip.h"

// The crossing point is prev + t * (curr - prev), a multiply and then an add as the reference computes it.
#pragma clang fp contract(off)

namespace bbfmm {
namespace iso {

namespace {

constexpr int kThreads = 256;
constexpr int32_t kNone = 0x7f7f7f7f; // hipMemset(0x7f): no copy / no use yet; above every id (see finish_fits)

int grid_for(int64_t n) {
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 4096)));
}

// Device allocations of one finish_device() call, freed on every exit.
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

// ---- clip

// The polygon of facet t.  All corners inside every plane: the three corners, snapped (what the six planes leave of
// them).  All corners further than 2 eps outside one plane: nothing (every point an earlier plane makes lies between
// them on that axis).  Only the facets in between run the general clip with its indexed private arrays.
__device__ __forceinline__ int clip_facet(const double *__restrict__ verts, const int64_t *__restrict__ facets, int64_t t,
                                          const ClipBox &b, double out[kClipMaxPoints][3], int corner[kClipMaxPoints],
                                          bool *all_in) {
    double tri[3][3];
    for (int k = 0; k < 3; ++k) {
        const int64_t v = facets[3 * t + k];
        for (int a = 0; a < 3; ++a) tri[k][a] = verts[3 * v + a];
    }
    bool in = true;
    for (int k = 0; k < 3; ++k)
        for (int plane = 0; plane < 6; ++plane) in = in && clip_inside_plane(tri[k], plane, b);
    *all_in = in;
    if (in) {
        for (int k = 0; k < 3; ++k) {
            for (int a = 0; a < 3; ++a) out[k][a] = tri[k][a];
            clip_snap_near(out[k], b);
            corner[k] = k;
        }
        return 3;
    }
    const double far = 2.0 * b.eps;
    for (int a = 0; a < 3; ++a) {
        if (tri[0][a] < b.lo[a] - far && tri[1][a] < b.lo[a] - far && tri[2][a] < b.lo[a] - far) return 0;
        if (tri[0][a] > b.hi[a] + far && tri[1][a] > b.hi[a] + far && tri[2][a] > b.hi[a] + far) return 0;
    }
    return clip_triangle(tri, b, out, corner);
}

__global__ __launch_bounds__(kThreads) void clip_count_kernel(int64_t nf, const double *__restrict__ verts,
                                                               const int64_t *__restrict__ facets, ClipBox b,
                                                               int32_t *__restrict__ vcnt, int32_t *__restrict__ fcnt,
                                                               unsigned long long *__restrict__ stats) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nf; t += int64_t(gridDim.x) * kThreads) {
        double out[kClipMaxPoints][3];
        int corner[kClipMaxPoints];
        bool all_in;
        const int n = clip_facet(verts, facets, t, b, out, corner, &all_in);
        vcnt[t] = n;
        fcnt[t] = n ? n - 2 : 0;
        if (!n) atomicAdd(&stats[kFinOutside], 1ull); // counts only: nothing is placed by them
        else if (!all_in) atomicAdd(&stats[kFinStraddling], 1ull);
    }
}

// The polygon's points appended unwelded and fanned as (0, k - 1, k) (aabb_clipping.rs:95-101).  esrc: the source vertex
// a point is a kept copy of, -1 for a point made on a plane.
__global__ __launch_bounds__(kThreads) void clip_emit_kernel(int64_t nf, const double *__restrict__ verts,
                                                              const int64_t *__restrict__ facets, ClipBox b,
                                                              const int32_t *__restrict__ voff, const int32_t *__restrict__ foff,
                                                              double *__restrict__ ev, int32_t *__restrict__ esrc,
                                                              int32_t *__restrict__ ef) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nf; t += int64_t(gridDim.x) * kThreads) {
        double out[kClipMaxPoints][3];
        int corner[kClipMaxPoints];
        bool all_in;
        const int n = clip_facet(verts, facets, t, b, out, corner, &all_in);
        const int32_t vo = voff[t], fo = foff[t];
        for (int k = 0; k < n; ++k) {
            for (int a = 0; a < 3; ++a) ev[3 * int64_t(vo + k) + a] = out[k][a];
            esrc[vo + k] = corner[k] < 0 ? -1 : static_cast<int32_t>(facets[3 * t + corner[k]]);
        }
        for (int k = 2; k < n; ++k) {
            ef[3 * int64_t(fo + k - 2)] = vo;
            ef[3 * int64_t(fo + k - 2) + 1] = vo + k - 1;
            ef[3 * int64_t(fo + k - 2) + 2] = vo + k;
        }
    }
}

// ---- weld.  The kept copies of one source vertex are bit-equal, hence linked: only the first copy of every source
// vertex and the points made on planes (the candidates) go through the spatial search, in emitted order.

__global__ __launch_bounds__(kThreads) void first_copy_kernel(int64_t ne, const int32_t *__restrict__ esrc, int32_t *__restrict__ first) {
    for (int64_t e = blockIdx.x * int64_t(kThreads) + threadIdx.x; e < ne; e += int64_t(gridDim.x) * kThreads)
        if (esrc[e] >= 0) atomicMin(&first[esrc[e]], static_cast<int32_t>(e));
}

__global__ __launch_bounds__(kThreads) void candidate_flags_kernel(int64_t ne, const int32_t *__restrict__ esrc,
                                                                    const int32_t *__restrict__ first, int32_t *__restrict__ cflag) {
    for (int64_t e = blockIdx.x * int64_t(kThreads) + threadIdx.x; e < ne; e += int64_t(gridDim.x) * kThreads)
        cflag[e] = (esrc[e] < 0 || first[esrc[e]] == e) ? 1 : 0;
}

// quantized_point_key (mesh_cleanup.rs:194-197): Rust's f64::round (half away from zero) and its saturating cast
__device__ __forceinline__ int64_t cell_of(double v, double cell) {
    const double q = round(v / cell);
    if (!(q == q)) return 0;
    if (q >= 9223372036854775808.0) return INT64_MAX;
    if (q <= -9223372036854775808.0) return INT64_MIN;
    return static_cast<int64_t>(q);
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) { // splitmix64 finaliser
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

__device__ __forceinline__ uint64_t cell_hash(int64_t qx, int64_t qy, int64_t qz) {
    return mix64(mix64(mix64(static_cast<uint64_t>(qx)) + static_cast<uint64_t>(qy)) + static_cast<uint64_t>(qz));
}

__global__ __launch_bounds__(kThreads) void candidates_kernel(int64_t ne, const int32_t *__restrict__ cflag,
                                                               const int32_t *__restrict__ cidx, const double *__restrict__ ev, double cell,
                                                               int32_t *__restrict__ cand, uint64_t *__restrict__ ckey,
                                                               int32_t *__restrict__ cval, int32_t *__restrict__ lab) {
    for (int64_t e = blockIdx.x * int64_t(kThreads) + threadIdx.x; e < ne; e += int64_t(gridDim.x) * kThreads) {
        if (!cflag[e]) continue;
        const int32_t c = cidx[e];
        cand[c] = static_cast<int32_t>(e);
        ckey[c] = cell_hash(cell_of(ev[3 * e], cell), cell_of(ev[3 * e + 1], cell), cell_of(ev[3 * e + 2], cell));
        cval[c] = c;
        lab[c] = c;
    }
}

__device__ __forceinline__ double dist2(const double *__restrict__ ev, int64_t p, int64_t q) {
    const double d0 = ev[3 * p] - ev[3 * q], d1 = ev[3 * p + 1] - ev[3 * q + 1], d2 = ev[3 * p + 2] - ev[3 * q + 2];
    return d0 * d0 + d1 * d1 + d2 * d2;
}

// lab[c] = the lowest label among the candidates linked to c (|p - q|^2 <= eps^2, the only thing that links two
// vertices: a hash collision costs a distance test).  Run with weld_jump_kernel until nothing changes, lab[c] is the
// lowest candidate of c's linked component.
__global__ __launch_bounds__(kThreads) void weld_hook_kernel(int64_t nc, const int32_t *__restrict__ cand, const double *__restrict__ ev,
                                                              const uint64_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                              double cell, double eps2, int32_t *lab, int32_t *__restrict__ changed) {
    for (int64_t c = blockIdx.x * int64_t(kThreads) + threadIdx.x; c < nc; c += int64_t(gridDim.x) * kThreads) {
        const int64_t p = cand[c];
        const int64_t q0 = cell_of(ev[3 * p], cell), q1 = cell_of(ev[3 * p + 1], cell), q2 = cell_of(ev[3 * p + 2], cell);
        const int32_t mine = __atomic_load_n(&lab[c], __ATOMIC_RELAXED);
        int32_t m = mine;
        for (int d = 0; d < 27; ++d) {
            const uint64_t h = cell_hash(static_cast<int64_t>(static_cast<uint64_t>(q0) + static_cast<uint64_t>(int64_t(d % 3 - 1))),
                                         static_cast<int64_t>(static_cast<uint64_t>(q1) + static_cast<uint64_t>(int64_t(d / 3 % 3 - 1))),
                                         static_cast<int64_t>(static_cast<uint64_t>(q2) + static_cast<uint64_t>(int64_t(d / 9 - 1))));
            int64_t lo = 0, hi = nc; // lower bound of h
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (skey[mid] < h) lo = mid + 1;
                else hi = mid;
            }
            for (int64_t i = lo; i < nc && skey[i] == h; ++i) {
                const int32_t o = sval[i];
                if (dist2(ev, p, cand[o]) <= eps2) m = min(m, __atomic_load_n(&lab[o], __ATOMIC_RELAXED));
            }
        }
        if (m < mine) {
            atomicMin(&lab[c], m);
            *changed = 1;
        }
    }
}

// lab[c] = the root of c: labels only ever fall and lab[c] <= c, so the walk ends
__global__ __launch_bounds__(kThreads) void weld_jump_kernel(int64_t nc, int32_t *lab) {
    for (int64_t c = blockIdx.x * int64_t(kThreads) + threadIdx.x; c < nc; c += int64_t(gridDim.x) * kThreads) {
        int32_t l = __atomic_load_n(&lab[c], __ATOMIC_RELAXED);
        for (;;) {
            const int32_t up = __atomic_load_n(&lab[l], __ATOMIC_RELAXED);
            if (up == l) break;
            l = up;
        }
        atomicMin(&lab[c], l);
    }
}

// rep[e]: the lowest-index emitted vertex of e's linked component; isrep: e is one.
__global__ __launch_bounds__(kThreads) void representatives_kernel(int64_t ne, const int32_t *__restrict__ esrc,
                                                                    const int32_t *__restrict__ first, const int32_t *__restrict__ cidx,
                                                                    const int32_t *__restrict__ cand, const int32_t *__restrict__ lab,
                                                                    const double *__restrict__ ev, double eps2, int32_t *__restrict__ rep,
                                                                    int32_t *__restrict__ isrep, unsigned long long *__restrict__ stats) {
    for (int64_t e = blockIdx.x * int64_t(kThreads) + threadIdx.x; e < ne; e += int64_t(gridDim.x) * kThreads) {
        const int32_t s = esrc[e];
        const int32_t r = cand[lab[cidx[s < 0 ? e : first[s]]]];
        rep[e] = r;
        isrep[e] = r == e ? 1 : 0;
        if (!(dist2(ev, e, r) <= eps2)) atomicAdd(&stats[kFinLoose], 1ull);
    }
}

// Welded ids in order of first appearance: a component appears first at its representative.
__global__ __launch_bounds__(kThreads) void welded_kernel(int64_t ne, const int32_t *__restrict__ rep, const int32_t *__restrict__ isrep,
                                                           const int32_t *__restrict__ rid, const double *__restrict__ ev,
                                                           double *__restrict__ wv, int32_t *__restrict__ wid) {
    for (int64_t e = blockIdx.x * int64_t(kThreads) + threadIdx.x; e < ne; e += int64_t(gridDim.x) * kThreads) {
        wid[e] = rid[rep[e]];
        if (isrep[e])
            for (int a = 0; a < 3; ++a) wv[3 * int64_t(rid[e]) + a] = ev[3 * e + a];
    }
}

// ---- facets

// collapsed (two equal welded ids), then tiny (|ab x ac|^2 <= eps^4 at the representatives) (mesh_cleanup.rs:57-81)
__global__ __launch_bounds__(kThreads) void facet_check_kernel(int64_t nef, const int32_t *__restrict__ ef, const int32_t *__restrict__ wid,
                                                                const double *__restrict__ wv, double eps4, int32_t *__restrict__ keep,
                                                                unsigned long long *__restrict__ stats) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nef; t += int64_t(gridDim.x) * kThreads) {
        const int64_t a = wid[ef[3 * t]], b = wid[ef[3 * t + 1]], c = wid[ef[3 * t + 2]];
        int32_t k = 1;
        if (a == b || b == c || a == c) {
            k = 0;
            atomicAdd(&stats[kFinCollapsed], 1ull);
        } else {
            double ab[3], ac[3];
            for (int x = 0; x < 3; ++x) {
                ab[x] = wv[3 * b + x] - wv[3 * a + x];
                ac[x] = wv[3 * c + x] - wv[3 * a + x];
            }
            const double n0 = ab[1] * ac[2] - ab[2] * ac[1], n1 = ab[2] * ac[0] - ab[0] * ac[2], n2 = ab[0] * ac[1] - ab[1] * ac[0];
            if (n0 * n0 + n1 * n1 + n2 * n2 <= eps4) {
                k = 0;
                atomicAdd(&stats[kFinTiny], 1ull);
            }
        }
        keep[t] = k;
    }
}

__device__ __forceinline__ void sorted_ids(const int32_t *__restrict__ ef, const int32_t *__restrict__ wid, int64_t t, uint32_t *s) {
    uint32_t a = wid[ef[3 * t]], b = wid[ef[3 * t + 1]], c = wid[ef[3 * t + 2]];
    if (a > b) { const uint32_t x = a; a = b; b = x; }
    if (b > c) { const uint32_t x = b; b = c; c = x; }
    if (a > b) { const uint32_t x = a; a = b; b = x; }
    s[0] = a;
    s[1] = b;
    s[2] = c;
}

// The surviving facets in order, keyed by the largest id of their sorted triple ...
__global__ __launch_bounds__(kThreads) void triple_high_kernel(int64_t nef, const int32_t *__restrict__ keep, const int32_t *__restrict__ sidx,
                                                                const int32_t *__restrict__ ef, const int32_t *__restrict__ wid,
                                                                uint32_t *__restrict__ key, int32_t *__restrict__ val) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nef; t += int64_t(gridDim.x) * kThreads) {
        if (!keep[t]) continue;
        uint32_t s[3];
        sorted_ids(ef, wid, t, s);
        key[sidx[t]] = s[2];
        val[sidx[t]] = static_cast<int32_t>(t);
    }
}

// ... then, in that order, by the two lower ids: after the second stable sort equal triples are adjacent, in facet order.
__global__ __launch_bounds__(kThreads) void triple_low_kernel(int64_t ns, const int32_t *__restrict__ val, const int32_t *__restrict__ ef,
                                                               const int32_t *__restrict__ wid, uint64_t *__restrict__ key) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < ns; i += int64_t(gridDim.x) * kThreads) {
        uint32_t s[3];
        sorted_ids(ef, wid, val[i], s);
        key[i] = uint64_t(s[0]) << 32 | s[1];
    }
}

// every facet of a run of equal triples but the first is a duplicate (mesh_cleanup.rs:83-87)
__global__ __launch_bounds__(kThreads) void duplicates_kernel(int64_t ns, const uint64_t *__restrict__ key, const int32_t *__restrict__ val,
                                                               const int32_t *__restrict__ ef, const int32_t *__restrict__ wid,
                                                               int32_t *__restrict__ keep, unsigned long long *__restrict__ stats) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x + 1; i < ns; i += int64_t(gridDim.x) * kThreads) {
        if (key[i] != key[i - 1]) continue;
        uint32_t s[3], p[3];
        sorted_ids(ef, wid, val[i], s);
        sorted_ids(ef, wid, val[i - 1], p);
        if (s[2] != p[2]) continue;
        keep[val[i]] = 0;
        atomicAdd(&stats[kFinDuplicate], 1ull);
    }
}

__global__ __launch_bounds__(kThreads) void use_count_kernel(int64_t nef, const int32_t *__restrict__ keep, const int32_t *__restrict__ ef,
                                                              const int32_t *__restrict__ wid, int32_t *__restrict__ use) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nef; t += int64_t(gridDim.x) * kThreads)
        if (keep[t])
            for (int a = 0; a < 3; ++a) atomicAdd(&use[wid[ef[3 * t + a]]], 1);
}

// A component of one facet (vertex connectivity, MIN_CONNECTED_COMPONENT_FACETS = 2, mesh_cleanup.rs:102-160) is a
// facet whose three vertices no other surviving facet uses.  The others record the first use of their vertices:
// 3 * facet + corner.
__global__ __launch_bounds__(kThreads) void lone_kernel(int64_t nef, const int32_t *__restrict__ keep, const int32_t *__restrict__ ef,
                                                         const int32_t *__restrict__ wid, const int32_t *__restrict__ use,
                                                         int32_t *__restrict__ kept, int32_t *__restrict__ first_use,
                                                         unsigned long long *__restrict__ stats) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nef; t += int64_t(gridDim.x) * kThreads) {
        int32_t k = keep[t];
        if (k) {
            const int32_t a = wid[ef[3 * t]], b = wid[ef[3 * t + 1]], c = wid[ef[3 * t + 2]];
            if (use[a] == 1 && use[b] == 1 && use[c] == 1) {
                k = 0;
                atomicAdd(&stats[kFinLone], 1ull);
            } else {
                atomicMin(&first_use[a], static_cast<int32_t>(3 * t));
                atomicMin(&first_use[b], static_cast<int32_t>(3 * t + 1));
                atomicMin(&first_use[c], static_cast<int32_t>(3 * t + 2));
            }
        }
        kept[t] = k;
    }
}

// compact_kept_facets (mesh_cleanup.rs:166-191): final ids in order of first use.  pos[3 * facet + corner] = 1 where a
// vertex is first used; its scan is the final id.
__global__ __launch_bounds__(kThreads) void first_use_flags_kernel(int64_t nw, const int32_t *__restrict__ first_use, int32_t *__restrict__ pos) {
    for (int64_t v = blockIdx.x * int64_t(kThreads) + threadIdx.x; v < nw; v += int64_t(gridDim.x) * kThreads)
        if (first_use[v] != kNone) pos[first_use[v]] = 1;
}

__global__ __launch_bounds__(kThreads) void out_vertices_kernel(int64_t nw, const int32_t *__restrict__ first_use, const int32_t *__restrict__ pidx,
                                                                 const double *__restrict__ wv, double *__restrict__ out) {
    for (int64_t v = blockIdx.x * int64_t(kThreads) + threadIdx.x; v < nw; v += int64_t(gridDim.x) * kThreads) {
        if (first_use[v] == kNone) continue;
        const int64_t o = pidx[first_use[v]];
        for (int a = 0; a < 3; ++a) out[3 * o + a] = wv[3 * v + a];
    }
}

__global__ __launch_bounds__(kThreads) void out_facets_kernel(int64_t nef, const int32_t *__restrict__ kept, const int32_t *__restrict__ fidx,
                                                               const int32_t *__restrict__ ef, const int32_t *__restrict__ wid,
                                                               const int32_t *__restrict__ first_use, const int32_t *__restrict__ pidx,
                                                               int64_t *__restrict__ out) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nef; t += int64_t(gridDim.x) * kThreads) {
        if (!kept[t]) continue;
        for (int a = 0; a < 3; ++a) out[3 * int64_t(fidx[t]) + a] = pidx[first_use[wid[ef[3 * t + a]]]];
    }
}

} // namespace

bool make_clip_box(const double *extents, ClipBox *out, std::string *err) {
    if (!extents) {
        *err = "isosurface: extents must not be null";
        return false;
    }
    for (int a = 0; a < 6; ++a)
        if (!std::isfinite(extents[a])) {
            *err = "isosurface: extents must be finite";
            return false;
        }
    double d2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        if (extents[a + 3] < extents[a]) {
            *err = "isosurface: inverted extents (max < min on axis " + std::to_string(a) + ")";
            return false;
        }
        out->lo[a] = extents[a];
        out->hi[a] = extents[a + 3];
        const double d = extents[a + 3] - extents[a];
        d2 = d2 + d * d;
    }
    out->eps = 1.0e-10 * std::max(std::sqrt(d2), 1.0);
    return true;
}

bool finish_fits(int64_t n_vertices, int64_t n_facets, std::string *err) {
    if (n_vertices < 0 || n_facets < 0) {
        *err = "isosurface: negative mesh size";
        return false;
    }
    if (n_facets > kFinishMaxFacets || n_vertices > kFinishMaxVertices) {
        *err = "isosurface: a mesh of " + std::to_string(n_vertices) + " vertices and " + std::to_string(n_facets) +
               " facets is too large to clip and clean: vertex and corner ids are packed in 32 bits (at most " +
               std::to_string(kFinishMaxFacets) + " facets; use a coarser resolution or finish = raw)";
        return false;
    }
    return true;
}

int finish_device(const double *d_vertices, int64_t nv, const int64_t *d_facets, int64_t nf, const ClipBox &box, hipStream_t st,
                  Mesh *mesh, std::string *err, int close_mode, double close_resolution) {
#define FIN_HIP(x)                                                                               \
    do {                                                                                         \
        hipError_t e_ = (x);                                                                     \
        if (e_ != hipSuccess) {                                                                  \
            *err = std::string("isosurface finish: ") + #x + ": " + hipGetErrorString(e_);      \
            return BBFMM_DEVICE_ERROR;                                                           \
        }                                                                                        \
    } while (0)
    if (!finish_fits(nv, nf, err)) return BBFMM_BAD_ARGUMENT;
    mesh->vertices.clear();
    mesh->facets.clear();
    for (int q = 0; q < kFinStats; ++q) mesh->finish_stats[q] = 0;
    mesh->finish_stats[kFinFacetsIn] = nf;
    if (nf == 0) return BBFMM_OK;
    Pool pool;
    unsigned long long *d_stats = nullptr;
    int32_t *d_changed = nullptr;
    FIN_HIP(pool.get(&d_stats, kFinStats));
    FIN_HIP(pool.get(&d_changed, 1));
    FIN_HIP(hipMemsetAsync(d_stats, 0, kFinStats * sizeof(unsigned long long), st));
    void *scan_tmp = nullptr;
    size_t scan_cap = 0;
    // out = exclusive scan of in[0..n), *total its sum (n < 2^31 and so is the sum, see finish_fits)
    auto scan = [&](const int32_t *in, int32_t *out, int64_t n, int64_t *total) -> int {
        *total = 0;
        if (n == 0) return BBFMM_OK;
        size_t bytes = 0;
        FIN_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, int32_t(0), static_cast<size_t>(n), rocprim::plus<int32_t>(), st));
        if (bytes > scan_cap) {
            pool.put(static_cast<uint8_t *>(scan_tmp));
            uint8_t *p = nullptr;
            FIN_HIP(pool.get(&p, bytes));
            scan_tmp = p;
            scan_cap = bytes;
        }
        FIN_HIP(rocprim::exclusive_scan(scan_tmp, bytes, in, out, int32_t(0), static_cast<size_t>(n), rocprim::plus<int32_t>(), st));
        int32_t last[2] = {0, 0};
        FIN_HIP(hipMemcpyAsync(&last[0], out + n - 1, 4, hipMemcpyDeviceToHost, st));
        FIN_HIP(hipMemcpyAsync(&last[1], in + n - 1, 4, hipMemcpyDeviceToHost, st));
        FIN_HIP(hipStreamSynchronize(st));
        *total = int64_t(last[0]) + last[1];
        return BBFMM_OK;
    };
    int rc = BBFMM_OK;
    auto download_stats = [&]() -> int {
        unsigned long long h[kFinStats];
        FIN_HIP(hipMemcpyAsync(h, d_stats, sizeof(h), hipMemcpyDeviceToHost, st));
        FIN_HIP(hipStreamSynchronize(st));
        for (int q = kFinFacetsIn + 1; q < kFinStats; ++q)
            if (q != kFinEmitted && q != kFinWelded) mesh->finish_stats[q] = static_cast<int64_t>(h[q]);
        return BBFMM_OK;
    };

    // ---- clip: count, scan, emit
    int32_t *vcnt = nullptr, *fcnt = nullptr, *voff = nullptr, *foff = nullptr;
    FIN_HIP(pool.get(&vcnt, static_cast<size_t>(nf)));
    FIN_HIP(pool.get(&fcnt, static_cast<size_t>(nf)));
    FIN_HIP(pool.get(&voff, static_cast<size_t>(nf)));
    FIN_HIP(pool.get(&foff, static_cast<size_t>(nf)));
    clip_count_kernel<<<grid_for(nf), kThreads, 0, st>>>(nf, d_vertices, d_facets, box, vcnt, fcnt, d_stats);
    FIN_HIP(hipGetLastError());
    int64_t ne = 0, nef = 0;
    if ((rc = scan(vcnt, voff, nf, &ne)) != BBFMM_OK) return rc;
    if ((rc = scan(fcnt, foff, nf, &nef)) != BBFMM_OK) return rc;
    mesh->finish_stats[kFinEmitted] = ne;
    if (ne == 0) return download_stats();
    double *ev = nullptr;
    int32_t *esrc = nullptr, *ef = nullptr;
    FIN_HIP(pool.get(&ev, 3 * static_cast<size_t>(ne)));
    FIN_HIP(pool.get(&esrc, static_cast<size_t>(ne)));
    FIN_HIP(pool.get(&ef, 3 * static_cast<size_t>(nef)));
    clip_emit_kernel<<<grid_for(nf), kThreads, 0, st>>>(nf, d_vertices, d_facets, box, voff, foff, ev, esrc, ef);
    FIN_HIP(hipGetLastError());
    FIN_HIP(hipStreamSynchronize(st));
    pool.put(vcnt);
    pool.put(fcnt);
    pool.put(voff);
    pool.put(foff);

    // ---- weld
    const int ge = grid_for(ne);
    const double cell = std::max(box.eps, 1.0e-12), eps2 = box.eps * box.eps;
    int32_t *first = nullptr, *cflag = nullptr, *cidx = nullptr;
    FIN_HIP(pool.get(&first, static_cast<size_t>(nv)));
    FIN_HIP(pool.get(&cflag, static_cast<size_t>(ne)));
    FIN_HIP(pool.get(&cidx, static_cast<size_t>(ne)));
    FIN_HIP(hipMemsetAsync(first, 0x7f, static_cast<size_t>(std::max<int64_t>(nv, 1)) * sizeof(int32_t), st));
    first_copy_kernel<<<ge, kThreads, 0, st>>>(ne, esrc, first);
    FIN_HIP(hipGetLastError());
    candidate_flags_kernel<<<ge, kThreads, 0, st>>>(ne, esrc, first, cflag);
    FIN_HIP(hipGetLastError());
    int64_t nc = 0;
    if ((rc = scan(cflag, cidx, ne, &nc)) != BBFMM_OK) return rc;
    int32_t *cand = nullptr, *cval = nullptr, *sval = nullptr, *lab = nullptr;
    uint64_t *ckey = nullptr, *skey = nullptr;
    uint8_t *sort_tmp = nullptr;
    FIN_HIP(pool.get(&cand, static_cast<size_t>(nc)));
    FIN_HIP(pool.get(&cval, static_cast<size_t>(nc)));
    FIN_HIP(pool.get(&sval, static_cast<size_t>(nc)));
    FIN_HIP(pool.get(&lab, static_cast<size_t>(nc)));
    FIN_HIP(pool.get(&ckey, static_cast<size_t>(nc)));
    FIN_HIP(pool.get(&skey, static_cast<size_t>(nc)));
    candidates_kernel<<<ge, kThreads, 0, st>>>(ne, cflag, cidx, ev, cell, cand, ckey, cval, lab);
    FIN_HIP(hipGetLastError());
    size_t sort_bytes = 0;
    FIN_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, ckey, skey, cval, sval, static_cast<size_t>(nc), 0, 64, st));
    FIN_HIP(pool.get(&sort_tmp, sort_bytes));
    FIN_HIP(rocprim::radix_sort_pairs(sort_tmp, sort_bytes, ckey, skey, cval, sval, static_cast<size_t>(nc), 0, 64, st));
    for (;;) { // to the fixed point: two rounds where every group is within eps of its first vertex
        int32_t changed = 0;
        FIN_HIP(hipMemsetAsync(d_changed, 0, sizeof(int32_t), st));
        weld_hook_kernel<<<grid_for(nc), kThreads, 0, st>>>(nc, cand, ev, skey, sval, cell, eps2, lab, d_changed);
        FIN_HIP(hipGetLastError());
        weld_jump_kernel<<<grid_for(nc), kThreads, 0, st>>>(nc, lab);
        FIN_HIP(hipGetLastError());
        FIN_HIP(hipMemcpyAsync(&changed, d_changed, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        FIN_HIP(hipStreamSynchronize(st));
        if (!changed) break;
    }
    int32_t *rep = nullptr, *isrep = nullptr, *rid = nullptr, *wid = nullptr;
    FIN_HIP(pool.get(&rep, static_cast<size_t>(ne)));
    FIN_HIP(pool.get(&isrep, static_cast<size_t>(ne)));
    FIN_HIP(pool.get(&rid, static_cast<size_t>(ne)));
    FIN_HIP(pool.get(&wid, static_cast<size_t>(ne)));
    representatives_kernel<<<ge, kThreads, 0, st>>>(ne, esrc, first, cidx, cand, lab, ev, eps2, rep, isrep, d_stats);
    FIN_HIP(hipGetLastError());
    int64_t nw = 0;
    if ((rc = scan(isrep, rid, ne, &nw)) != BBFMM_OK) return rc;
    mesh->finish_stats[kFinWelded] = ne - nw;
    double *wv = nullptr;
    FIN_HIP(pool.get(&wv, 3 * static_cast<size_t>(nw)));
    welded_kernel<<<ge, kThreads, 0, st>>>(ne, rep, isrep, rid, ev, wv, wid);
    FIN_HIP(hipGetLastError());
    FIN_HIP(hipStreamSynchronize(st));
    for (int32_t *p : {first, cflag, cidx, cand, cval, sval, lab, rep, isrep, rid, esrc}) pool.put(p);
    pool.put(ckey);
    pool.put(skey);
    pool.put(sort_tmp);
    pool.put(ev);

    // ---- facets: collapsed and tiny, duplicates, lone
    const int gf = grid_for(nef);
    int32_t *keep = nullptr, *sidx = nullptr;
    FIN_HIP(pool.get(&keep, static_cast<size_t>(nef)));
    FIN_HIP(pool.get(&sidx, static_cast<size_t>(nef)));
    facet_check_kernel<<<gf, kThreads, 0, st>>>(nef, ef, wid, wv, (box.eps * box.eps) * (box.eps * box.eps), keep, d_stats);
    FIN_HIP(hipGetLastError());
    int64_t ns = 0;
    if ((rc = scan(keep, sidx, nef, &ns)) != BBFMM_OK) return rc;
    if (ns > 1) {
        uint32_t *k32 = nullptr, *k32o = nullptr;
        uint64_t *k64 = nullptr, *k64o = nullptr;
        int32_t *v0 = nullptr, *v1 = nullptr;
        const size_t m = static_cast<size_t>(ns);
        FIN_HIP(pool.get(&k32, m));
        FIN_HIP(pool.get(&k32o, m));
        FIN_HIP(pool.get(&k64, m));
        FIN_HIP(pool.get(&k64o, m));
        FIN_HIP(pool.get(&v0, m));
        FIN_HIP(pool.get(&v1, m));
        size_t b32 = 0, b64 = 0;
        FIN_HIP(rocprim::radix_sort_pairs(nullptr, b32, k32, k32o, v0, v1, m, 0, 32, st));
        FIN_HIP(rocprim::radix_sort_pairs(nullptr, b64, k64, k64o, v1, v0, m, 0, 64, st));
        FIN_HIP(pool.get(&sort_tmp, std::max(b32, b64)));
        triple_high_kernel<<<gf, kThreads, 0, st>>>(nef, keep, sidx, ef, wid, k32, v0);
        FIN_HIP(hipGetLastError());
        FIN_HIP(rocprim::radix_sort_pairs(sort_tmp, b32, k32, k32o, v0, v1, m, 0, 32, st));
        triple_low_kernel<<<grid_for(ns), kThreads, 0, st>>>(ns, v1, ef, wid, k64);
        FIN_HIP(hipGetLastError());
        FIN_HIP(rocprim::radix_sort_pairs(sort_tmp, b64, k64, k64o, v1, v0, m, 0, 64, st));
        duplicates_kernel<<<grid_for(ns), kThreads, 0, st>>>(ns, k64o, v0, ef, wid, keep, d_stats);
        FIN_HIP(hipGetLastError());
        FIN_HIP(hipStreamSynchronize(st));
        pool.put(k32);
        pool.put(k32o);
        pool.put(k64);
        pool.put(k64o);
        pool.put(v0);
        pool.put(v1);
        pool.put(sort_tmp);
    }
    int32_t *use = nullptr, *first_use = nullptr, *kept = nullptr, *fidx = sidx, *pos = nullptr, *pidx = nullptr;
    FIN_HIP(pool.get(&use, static_cast<size_t>(nw)));
    FIN_HIP(pool.get(&first_use, static_cast<size_t>(nw)));
    FIN_HIP(pool.get(&kept, static_cast<size_t>(nef)));
    FIN_HIP(pool.get(&pos, 3 * static_cast<size_t>(nef)));
    FIN_HIP(pool.get(&pidx, 3 * static_cast<size_t>(nef)));
    FIN_HIP(hipMemsetAsync(use, 0, static_cast<size_t>(std::max<int64_t>(nw, 1)) * sizeof(int32_t), st));
    FIN_HIP(hipMemsetAsync(first_use, 0x7f, static_cast<size_t>(std::max<int64_t>(nw, 1)) * sizeof(int32_t), st));
    FIN_HIP(hipMemsetAsync(pos, 0, 3 * static_cast<size_t>(std::max<int64_t>(nef, 1)) * sizeof(int32_t), st));
    use_count_kernel<<<gf, kThreads, 0, st>>>(nef, keep, ef, wid, use);
    FIN_HIP(hipGetLastError());
    lone_kernel<<<gf, kThreads, 0, st>>>(nef, keep, ef, wid, use, kept, first_use, d_stats);
    FIN_HIP(hipGetLastError());
    first_use_flags_kernel<<<grid_for(nw), kThreads, 0, st>>>(nw, first_use, pos);
    FIN_HIP(hipGetLastError());
    int64_t nv_out = 0, nf_out = 0;
    if ((rc = scan(pos, pidx, 3 * nef, &nv_out)) != BBFMM_OK) return rc;
    if ((rc = scan(kept, fidx, nef, &nf_out)) != BBFMM_OK) return rc;
    double *ov = nullptr;
    int64_t *of = nullptr;
    FIN_HIP(pool.get(&ov, 3 * static_cast<size_t>(nv_out)));
    FIN_HIP(pool.get(&of, 3 * static_cast<size_t>(nf_out)));
    out_vertices_kernel<<<grid_for(nw), kThreads, 0, st>>>(nw, first_use, pidx, wv, ov);
    FIN_HIP(hipGetLastError());
    out_facets_kernel<<<gf, kThreads, 0, st>>>(nef, kept, fidx, ef, wid, first_use, pidx, of);
    FIN_HIP(hipGetLastError());
    if (close_mode == kFinishClosePositive || close_mode == kFinishCloseNegative) { // closed while still on the device
        if ((rc = download_stats()) != BBFMM_OK) return rc;
        for (int32_t *p : {keep, use, first_use, kept, fidx, pos, pidx, wid, ef}) pool.put(p);
        pool.put(wv);
        return closure_device(ov, nv_out, of, nf_out, box, close_resolution, close_mode, st, mesh, err);
    }
    mesh->vertices.resize(3 * static_cast<size_t>(nv_out));
    mesh->facets.resize(3 * static_cast<size_t>(nf_out));
    if (nv_out) FIN_HIP(hipMemcpyAsync(mesh->vertices.data(), ov, mesh->vertices.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (nf_out) FIN_HIP(hipMemcpyAsync(mesh->facets.data(), of, mesh->facets.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return download_stats();
#undef FIN_HIP
}

} // namespace iso
} // namespace bbfmm
