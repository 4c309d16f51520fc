// Boundary closure on the device (isosurface_closure.hpp; DESIGN.md "Boundary closure"): the open edges of the finished
// mesh and their face masks, the cut cells of the six cap grids, the regions of whole cells, the kept whole cells with
// their vertices, and the append of the band triangles that the host triangulated.  One thread per item, grid-stride;
// placement by rocPRIM scans and stable radix sorts; integer atomics only for minima over indices and for counts, so the
// result does not depend on thread order.
#include "isosurface_closure.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <map>
#include <tuple>
#include <unordered_map>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "closure_triangulate.hpp"
#include "ferreus_bbfmm_hip.h"

// cut and whole cells are decided by comparisons of lo - tol, hi + tol, g - tol and g + tol as written
#pragma clang fp contract(off)

namespace bbfmm {
namespace iso {

namespace {

constexpr int kThreads = 256;

int grid_for(int64_t n) {
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 4096)));
}

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
};

// The six cap grids.  Face f = 2 * axis + side (XMin, XMax, YMin, YMax, ZMin, ZMax); its u and v are the two other axes
// in ascending order (uv_axes); cell (i, j) of face f has the id off[f] + j * n[u] + i.
struct Caps {
    int32_t n[3];        // intervals per axis
    const double *g[3];  // n[a] + 1 coordinates per axis (device)
    int64_t off[7];      // first cell of every face; off[6]: all cells
    double lo[3], hi[3]; // the extents
    double eps, tol;
};

__host__ __device__ inline int face_u(int f) { return (f >> 1) == 0 ? 1 : 0; }
__host__ __device__ inline int face_v(int f) { return (f >> 1) == 2 ? 1 : 2; }
// ccw_is_outward (boundary_closure.rs:947-956)
__host__ __device__ inline bool face_ccw_outward(int f) { return ((f >> 1) == 1) != ((f & 1) == 1); }

// The cell across side s (0: v - 1, 1: u + 1, 2: v + 1, 3: u - 1) of cell (i, j) of face f: on the same face or, over a
// box edge, the cell of the adjacent face that shares that grid edge.
__host__ __device__ inline int64_t cell_across(const Caps &c, int f, int i, int j, int s) {
    const int ua = face_u(f), va = face_v(f), a = f >> 1;
    const int di = s == 1 ? 1 : (s == 3 ? -1 : 0), dj = s == 2 ? 1 : (s == 0 ? -1 : 0);
    const int ni = i + di, nj = j + dj;
    if (ni >= 0 && ni < c.n[ua] && nj >= 0 && nj < c.n[va]) return c.off[f] + int64_t(nj) * c.n[ua] + ni;
    // over the box edge: the face of the axis that was left, at the side that was left
    const int ax = di != 0 ? ua : va;
    const int g = 2 * ax + ((di > 0 || dj > 0) ? 1 : 0);
    int idx[3];
    idx[ua] = i;
    idx[va] = j;
    idx[a] = (f & 1) ? c.n[a] - 1 : 0;
    return c.off[g] + int64_t(idx[face_v(g)]) * c.n[face_u(g)] + idx[face_u(g)];
}

__host__ __device__ inline int face_of_cell(const Caps &c, int64_t cell) {
    int f = 0;
    while (f < 5 && cell >= c.off[f + 1]) ++f;
    return f;
}

// the smallest i in [0, n) with g[i + 1] + pad >= x (n: none); the largest i in [0, n) with g[i] - pad <= x (-1: none)
__device__ inline int first_cell(const double *__restrict__ g, int n, double pad, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g[mid + 1] + pad >= x) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
__device__ inline int last_cell(const double *__restrict__ g, int n, double pad, double x) {
    int lo = -1, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (g[mid] - pad <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ inline int vertex_mask(const double *__restrict__ verts, int64_t v, const Caps &c) {
    int m = 0;
    for (int a = 0; a < 3; ++a) {
        const double p = verts[3 * v + a];
        if (fabs(p - c.lo[a]) <= c.eps) m |= 1 << (2 * a);
        if (fabs(p - c.hi[a]) <= c.eps) m |= 1 << (2 * a + 1);
    }
    return m;
}

// ---- open edges

__global__ __launch_bounds__(kThreads) void edge_keys_kernel(int64_t nf, const int64_t *__restrict__ facets, uint64_t *__restrict__ key,
                                                              int32_t *__restrict__ val) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < 3 * nf; i += int64_t(gridDim.x) * kThreads) {
        const int64_t t = i / 3, k = i % 3;
        const uint64_t a = static_cast<uint64_t>(facets[3 * t + k]), b = static_cast<uint64_t>(facets[3 * t + (k + 1) % 3]);
        key[i] = a < b ? (a << 32 | b) : (b << 32 | a);
        val[i] = static_cast<int32_t>(i);
    }
}

// a run of one in the sorted keys is an open edge; the flag goes to its corner 3 t + k
__global__ __launch_bounds__(kThreads) void open_flags_kernel(int64_t n, const uint64_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                               int32_t *__restrict__ flag) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads) {
        const bool open = (i == 0 || skey[i - 1] != skey[i]) && (i == n - 1 || skey[i + 1] != skey[i]);
        flag[sval[i]] = open ? 1 : 0;
    }
}

// stats: [0, 6) open edges per face, [6] off the box, [7] the first of those (a minimum)
__global__ __launch_bounds__(kThreads) void open_edges_kernel(int64_t n, const int32_t *__restrict__ flag, const int32_t *__restrict__ oidx,
                                                               const int64_t *__restrict__ facets, const double *__restrict__ verts, Caps c,
                                                               int64_t *__restrict__ eab, int32_t *__restrict__ emask, double *__restrict__ exyz,
                                                               unsigned long long *__restrict__ stats) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads) {
        if (!flag[i]) continue;
        const int64_t e = oidx[i], t = i / 3, k = i % 3;
        const int64_t a = facets[3 * t + k], b = facets[3 * t + (k + 1) % 3];
        const int m = vertex_mask(verts, a, c) & vertex_mask(verts, b, c);
        eab[2 * e] = a;
        eab[2 * e + 1] = b;
        emask[e] = m;
        for (int x = 0; x < 3; ++x) {
            exyz[6 * e + x] = verts[3 * a + x];
            exyz[6 * e + 3 + x] = verts[3 * b + x];
        }
        for (int f = 0; f < 6; ++f)
            if (m & (1 << f)) atomicAdd(&stats[f], 1ull);
        if (m == 0) {
            atomicAdd(&stats[6], 1ull);
            atomicMin(&stats[7], static_cast<unsigned long long>(e));
        }
    }
}

// ---- cut cells

// every cell of the faces of an open edge that its bounding box, widened by tol, meets
__global__ __launch_bounds__(kThreads) void mark_edges_kernel(int64_t ne, const int32_t *__restrict__ emask, const double *__restrict__ exyz,
                                                               Caps c, int32_t *__restrict__ cut) {
    for (int64_t e = blockIdx.x * int64_t(kThreads) + threadIdx.x; e < ne; e += int64_t(gridDim.x) * kThreads) {
        const int m = emask[e];
        for (int f = 0; f < 6; ++f) {
            if (!(m & (1 << f))) continue;
            const int ua = face_u(f), va = face_v(f);
            const double pu = exyz[6 * e + ua], qu = exyz[6 * e + 3 + ua], pv = exyz[6 * e + va], qv = exyz[6 * e + 3 + va];
            const double ulo = fmin(pu, qu) - c.tol, uhi = fmax(pu, qu) + c.tol, vlo = fmin(pv, qv) - c.tol, vhi = fmax(pv, qv) + c.tol;
            const int i0 = first_cell(c.g[ua], c.n[ua], 0.0, ulo), i1 = last_cell(c.g[ua], c.n[ua], 0.0, uhi);
            const int j0 = first_cell(c.g[va], c.n[va], 0.0, vlo), j1 = last_cell(c.g[va], c.n[va], 0.0, vhi);
            for (int j = j0; j <= j1; ++j)
                for (int i = i0; i <= i1; ++i) cut[c.off[f] + int64_t(j) * c.n[ua] + i] = 1; // (the same value from every thread)
        }
    }
}

// a vertex on two or more faces cuts the cells of those faces that hold it (closed, widened by tol); pflag: it is one
__global__ __launch_bounds__(kThreads) void mark_vertices_kernel(int64_t nv, const double *__restrict__ verts, Caps c,
                                                                  int32_t *__restrict__ cut, int32_t *__restrict__ pflag) {
    for (int64_t v = blockIdx.x * int64_t(kThreads) + threadIdx.x; v < nv; v += int64_t(gridDim.x) * kThreads) {
        const int m = vertex_mask(verts, v, c);
        const bool many = __popc(m) >= 2;
        pflag[v] = many ? 1 : 0;
        if (!many) continue;
        for (int f = 0; f < 6; ++f) {
            if (!(m & (1 << f))) continue;
            const int ua = face_u(f), va = face_v(f);
            const double pu = verts[3 * v + ua], pv = verts[3 * v + va];
            const int i0 = first_cell(c.g[ua], c.n[ua], c.tol, pu), i1 = last_cell(c.g[ua], c.n[ua], c.tol, pu);
            const int j0 = first_cell(c.g[va], c.n[va], c.tol, pv), j1 = last_cell(c.g[va], c.n[va], c.tol, pv);
            for (int j = j0; j <= j1; ++j)
                for (int i = i0; i <= i1; ++i) cut[c.off[f] + int64_t(j) * c.n[ua] + i] = 1;
        }
    }
}

__global__ __launch_bounds__(kThreads) void perimeter_vertices_kernel(int64_t nv, const int32_t *__restrict__ pflag, const int32_t *__restrict__ pidx,
                                                                       const double *__restrict__ verts, Caps c, int64_t *__restrict__ pid,
                                                                       int32_t *__restrict__ pmask, double *__restrict__ pxyz) {
    for (int64_t v = blockIdx.x * int64_t(kThreads) + threadIdx.x; v < nv; v += int64_t(gridDim.x) * kThreads) {
        if (!pflag[v]) continue;
        const int64_t o = pidx[v];
        pid[o] = v;
        pmask[o] = vertex_mask(verts, v, c);
        for (int x = 0; x < 3; ++x) pxyz[3 * o + x] = verts[3 * v + x];
    }
}

__global__ __launch_bounds__(kThreads) void cut_list_kernel(int64_t nc, const int32_t *__restrict__ cut, const int32_t *__restrict__ cidx,
                                                             int32_t *__restrict__ list, int32_t *__restrict__ lab) {
    for (int64_t q = blockIdx.x * int64_t(kThreads) + threadIdx.x; q < nc; q += int64_t(gridDim.x) * kThreads) {
        if (cut[q]) list[cidx[q]] = static_cast<int32_t>(q);
        lab[q] = cut[q] ? -1 : static_cast<int32_t>(q);
    }
}

// ---- regions: the whole cells linked over grid edges, labelled with the lowest cell id of their component

__device__ inline int32_t region_root(int32_t *lab, int32_t x) { // labels only fall and lab[x] <= x, so the walk ends
    for (;;) {
        const int32_t up = __atomic_load_n(&lab[x], __ATOMIC_RELAXED);
        if (up == x) return x;
        x = up;
    }
}

// hook: the higher root of every linked pair goes under the lower one
__global__ __launch_bounds__(kThreads) void region_hook_kernel(int64_t nc, Caps c, int32_t *lab, int32_t *__restrict__ changed) {
    for (int64_t q = blockIdx.x * int64_t(kThreads) + threadIdx.x; q < nc; q += int64_t(gridDim.x) * kThreads) {
        if (__atomic_load_n(&lab[q], __ATOMIC_RELAXED) < 0) continue;
        const int f = face_of_cell(c, q);
        const int64_t r = q - c.off[f];
        const int i = static_cast<int>(r % c.n[face_u(f)]), j = static_cast<int>(r / c.n[face_u(f)]);
        for (int s = 0; s < 4; ++s) {
            const int64_t d = cell_across(c, f, i, j, s);
            if (d >= q || __atomic_load_n(&lab[d], __ATOMIC_RELAXED) < 0) continue; // every pair once, from its higher cell
            for (;;) {
                const int32_t ra = region_root(lab, static_cast<int32_t>(q)), rb = region_root(lab, static_cast<int32_t>(d));
                if (ra == rb) break;
                const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
                const int32_t old = atomicCAS(&lab[hi], hi, lo); // only a root is hooked: no link is ever lost
                *changed = 1;
                if (old == hi) break; // hi was a root and now hangs under lo
            }
        }
    }
}

// jump: every whole cell to its root
__global__ __launch_bounds__(kThreads) void region_jump_kernel(int64_t nc, int32_t *lab) {
    for (int64_t q = blockIdx.x * int64_t(kThreads) + threadIdx.x; q < nc; q += int64_t(gridDim.x) * kThreads) {
        if (__atomic_load_n(&lab[q], __ATOMIC_RELAXED) < 0) continue;
        atomicMin(&lab[q], region_root(lab, static_cast<int32_t>(q)));
    }
}

__global__ __launch_bounds__(kThreads) void region_count_kernel(int64_t nc, const int32_t *__restrict__ lab, unsigned long long *__restrict__ count) {
    for (int64_t q = blockIdx.x * int64_t(kThreads) + threadIdx.x; q < nc; q += int64_t(gridDim.x) * kThreads)
        if (lab[q] == q) atomicAdd(count, 1ull);
}

// the labels across the four sides of every cut cell (-1: a cut cell)
__global__ __launch_bounds__(kThreads) void cut_neighbours_kernel(int64_t ncut, const int32_t *__restrict__ list, Caps c,
                                                                   const int32_t *__restrict__ lab, int32_t *__restrict__ nbl) {
    for (int64_t x = blockIdx.x * int64_t(kThreads) + threadIdx.x; x < ncut; x += int64_t(gridDim.x) * kThreads) {
        const int64_t q = list[x];
        const int f = face_of_cell(c, q);
        const int64_t r = q - c.off[f];
        const int i = static_cast<int>(r % c.n[face_u(f)]), j = static_cast<int>(r / c.n[face_u(f)]);
        for (int s = 0; s < 4; ++s) nbl[4 * x + s] = lab[cell_across(c, f, i, j, s)];
    }
}

// ---- the kept whole cells

__global__ __launch_bounds__(kThreads) void region_flags_kernel(int64_t nk, const int32_t *__restrict__ kept_labels, int32_t *__restrict__ rk) {
    for (int64_t x = blockIdx.x * int64_t(kThreads) + threadIdx.x; x < nk; x += int64_t(gridDim.x) * kThreads) rk[kept_labels[x]] = 1;
}

__global__ __launch_bounds__(kThreads) void whole_kept_kernel(int64_t nc, const int32_t *__restrict__ lab, const int32_t *__restrict__ rk,
                                                               int32_t *__restrict__ wk) {
    for (int64_t q = blockIdx.x * int64_t(kThreads) + threadIdx.x; q < nc; q += int64_t(gridDim.x) * kThreads)
        wk[q] = (lab[q] >= 0 && rk[lab[q]]) ? 1 : 0;
}

struct CapBase {
    int64_t base[6]; // the first cap facet of whole cell q of face f is base[f] + 2 * widx[q]
    int64_t nv_mesh; // grid point (ix, iy, iz) has the provisional id nv_mesh + (iz * (n[1] + 1) + iy) * (n[0] + 1) + ix
};

__host__ __device__ inline int64_t grid_key(const Caps &c, int f, int gi, int gj) {
    int idx[3];
    idx[face_u(f)] = gi;
    idx[face_v(f)] = gj;
    idx[f >> 1] = (f & 1) ? c.n[f >> 1] : 0;
    return (int64_t(idx[2]) * (c.n[1] + 1) + idx[1]) * (int64_t(c.n[0]) + 1) + idx[0];
}

// two triangles per kept whole cell on the diagonal (i, j) - (i + 1, j + 1), wound outward, with provisional ids
__global__ __launch_bounds__(kThreads) void whole_facets_kernel(int64_t nc, const int32_t *__restrict__ wk, const int32_t *__restrict__ widx,
                                                                 Caps c, CapBase cb, int64_t *__restrict__ cap) {
    for (int64_t q = blockIdx.x * int64_t(kThreads) + threadIdx.x; q < nc; q += int64_t(gridDim.x) * kThreads) {
        if (!wk[q]) continue;
        const int f = face_of_cell(c, q);
        const int64_t r = q - c.off[f];
        const int i = static_cast<int>(r % c.n[face_u(f)]), j = static_cast<int>(r / c.n[face_u(f)]);
        const int64_t p00 = cb.nv_mesh + grid_key(c, f, i, j), p10 = cb.nv_mesh + grid_key(c, f, i + 1, j);
        const int64_t p11 = cb.nv_mesh + grid_key(c, f, i + 1, j + 1), p01 = cb.nv_mesh + grid_key(c, f, i, j + 1);
        int64_t *o = cap + 3 * (cb.base[f] + 2 * int64_t(widx[q]));
        const bool ccw = face_ccw_outward(f);
        o[0] = p00, o[1] = ccw ? p10 : p11, o[2] = ccw ? p11 : p10;
        o[3] = p00, o[4] = ccw ? p11 : p01, o[5] = ccw ? p01 : p11;
    }
}

// ---- final ids: the new vertices in order of first use by the cap facets

__global__ __launch_bounds__(kThreads) void corner_keys_kernel(int64_t n, const int64_t *__restrict__ cap, uint64_t *__restrict__ key,
                                                                int32_t *__restrict__ val) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads) {
        key[i] = static_cast<uint64_t>(cap[i]);
        val[i] = static_cast<int32_t>(i);
    }
}

// the sort is stable: the first corner of a run of equal keys is the first use of that grid point
__global__ __launch_bounds__(kThreads) void first_use_kernel(int64_t n, const uint64_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                              uint64_t nv_mesh, int32_t *__restrict__ pos) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads)
        if (skey[i] >= nv_mesh && (i == 0 || skey[i - 1] != skey[i])) pos[sval[i]] = 1;
}

__global__ __launch_bounds__(kThreads) void renumber_kernel(int64_t n, const uint64_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                             uint64_t nv_mesh, const int32_t *__restrict__ pidx, Caps c,
                                                             int64_t *__restrict__ cap_out, double *__restrict__ new_verts) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads) {
        const uint64_t k = skey[i];
        if (k < nv_mesh) {
            cap_out[sval[i]] = static_cast<int64_t>(k);
            continue;
        }
        int64_t lo = 0, hi = i; // the head of the run of k
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (skey[mid] < k) lo = mid + 1;
            else hi = mid;
        }
        const int64_t id = pidx[sval[lo]];
        cap_out[sval[i]] = static_cast<int64_t>(nv_mesh) + id;
        if (lo == i) {
            const int64_t g = static_cast<int64_t>(k - nv_mesh), w0 = int64_t(c.n[0]) + 1, w1 = int64_t(c.n[1]) + 1;
            new_verts[3 * id] = c.g[0][g % w0];
            new_verts[3 * id + 1] = c.g[1][(g / w0) % w1];
            new_verts[3 * id + 2] = c.g[2][g / (w0 * w1)];
        }
    }
}

// the facets of the mesh, corners 1 and 2 swapped for CloseNegative
__global__ __launch_bounds__(kThreads) void mesh_facets_kernel(int64_t nf, const int64_t *__restrict__ facets, int reverse, int64_t *__restrict__ out) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nf; t += int64_t(gridDim.x) * kThreads) {
        out[3 * t] = facets[3 * t];
        out[3 * t + 1] = facets[3 * t + (reverse ? 2 : 1)];
        out[3 * t + 2] = facets[3 * t + (reverse ? 1 : 2)];
    }
}

struct UnionFind {
    std::vector<int64_t> parent;
    int64_t make() {
        parent.push_back(static_cast<int64_t>(parent.size()));
        return static_cast<int64_t>(parent.size()) - 1;
    }
    int64_t find(int64_t x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    }
    void unite(int64_t a, int64_t b) {
        a = find(a), b = find(b);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }
};

struct PairHash {
    size_t operator()(const std::pair<int64_t, int64_t> &k) const {
        uint64_t x = static_cast<uint64_t>(k.first) * 0x9e3779b97f4a7c15ull ^ (static_cast<uint64_t>(k.second) + 0x7f4a7c15ull) * 0xbf58476d1ce4e5b9ull;
        x ^= x >> 31;
        return static_cast<size_t>(x);
    }
};

} // namespace

bool closure_axis(double lo, double hi, double resolution, double eps, std::vector<double> *out, std::string *err) {
    const double length = hi - lo;
    const double segs = std::max(std::ceil(length / std::max(resolution, eps)), 1.0);
    if (!(segs <= 2147483646.0)) {
        *err = "isosurface closure: the cap grid has too many intervals along an axis for this resolution";
        return false;
    }
    const int64_t n = static_cast<int64_t>(segs);
    out->resize(static_cast<size_t>(n) + 1);
    for (int64_t i = 0; i <= n; ++i) (*out)[static_cast<size_t>(i)] = i == n ? hi : lo + length * (static_cast<double>(i) / static_cast<double>(n));
    return true;
}

int closure_device(const double *d_vertices, int64_t nv, const int64_t *d_facets, int64_t nf, const ClipBox &box, double resolution,
                   int mode, hipStream_t st, Mesh *mesh, std::string *err) {
#define CLO_HIP(x)                                                                               \
    do {                                                                                         \
        hipError_t e_ = (x);                                                                     \
        if (e_ != hipSuccess) {                                                                  \
            *err = std::string("isosurface closure: ") + #x + ": " + hipGetErrorString(e_);     \
            return BBFMM_DEVICE_ERROR;                                                           \
        }                                                                                        \
    } while (0)
    for (int q = 0; q < kCloStats; ++q) mesh->closure_stats[q] = 0;
    if (mode != kFinishClosePositive && mode != kFinishCloseNegative) {
        *err = "isosurface closure: mode must be BBFMM_FINISH_CLOSE_POSITIVE or BBFMM_FINISH_CLOSE_NEGATIVE";
        return BBFMM_BAD_ARGUMENT;
    }
    if (!std::isfinite(resolution) || !(resolution > 0.0)) {
        *err = "isosurface closure: resolution must be finite and > 0";
        return BBFMM_BAD_ARGUMENT;
    }
    if (!finish_fits(nv, nf, err)) return BBFMM_BAD_ARGUMENT;
    // ---- the grids, refused before any work where a face has too many cells
    std::vector<double> axes[3];
    Caps caps;
    for (int a = 0; a < 3; ++a) {
        if (!closure_axis(box.lo[a], box.hi[a], resolution, box.eps, &axes[a], err)) return BBFMM_BAD_ARGUMENT;
        caps.n[a] = static_cast<int32_t>(axes[a].size() - 1);
        caps.lo[a] = box.lo[a];
        caps.hi[a] = box.hi[a];
    }
    caps.eps = box.eps;
    caps.tol = 1.0e-9 * resolution;
    caps.off[0] = 0;
    for (int f = 0; f < 6; ++f) {
        const int64_t cells = int64_t(caps.n[face_u(f)]) * caps.n[face_v(f)];
        if (cells > 2147483647ll) {
            *err = "isosurface closure: face " + std::to_string(f) + " of the extents has " + std::to_string(cells) +
                   " cap cells at this resolution, more than 2^31 - 1 (use a coarser resolution)";
            return BBFMM_BAD_ARGUMENT;
        }
        caps.off[f + 1] = caps.off[f] + cells;
    }
    const int64_t nc = caps.off[6];
    const int64_t n_grid = (int64_t(caps.n[0]) + 1) * (int64_t(caps.n[1]) + 1);
    if (nc > 2147483647ll || n_grid > (int64_t(1) << 62) / (int64_t(caps.n[2]) + 1)) {
        *err = "isosurface closure: the six faces of the extents have " + std::to_string(nc) +
               " cap cells at this resolution, more than 2^31 - 1 (cell ids are 32-bit; use a coarser resolution)";
        return BBFMM_BAD_ARGUMENT;
    }
    auto unchanged = [&]() -> int { // the mesh as it is
        mesh->vertices.resize(3 * static_cast<size_t>(nv));
        mesh->facets.resize(3 * static_cast<size_t>(nf));
        if (nv && d_vertices) CLO_HIP(hipMemcpyAsync(mesh->vertices.data(), d_vertices, mesh->vertices.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        if (nf) CLO_HIP(hipMemcpyAsync(mesh->facets.data(), d_facets, mesh->facets.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        CLO_HIP(hipStreamSynchronize(st));
        return BBFMM_OK;
    };
    if (nf == 0) return unchanged();
    Pool pool;
    void *scan_tmp = nullptr;
    size_t scan_cap = 0;
    auto scan = [&](const int32_t *in, int32_t *out, int64_t n, int64_t *total) -> int {
        *total = 0;
        if (n == 0) return BBFMM_OK;
        size_t bytes = 0;
        CLO_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, int32_t(0), static_cast<size_t>(n), rocprim::plus<int32_t>(), st));
        if (bytes > scan_cap) {
            uint8_t *p = nullptr;
            CLO_HIP(pool.get(&p, bytes));
            scan_tmp = p;
            scan_cap = bytes;
        }
        CLO_HIP(rocprim::exclusive_scan(scan_tmp, bytes, in, out, int32_t(0), static_cast<size_t>(n), rocprim::plus<int32_t>(), st));
        int32_t last[2] = {0, 0};
        CLO_HIP(hipMemcpyAsync(&last[0], out + n - 1, 4, hipMemcpyDeviceToHost, st));
        CLO_HIP(hipMemcpyAsync(&last[1], in + n - 1, 4, hipMemcpyDeviceToHost, st));
        CLO_HIP(hipStreamSynchronize(st));
        *total = int64_t(last[0]) + last[1];
        return BBFMM_OK;
    };
    auto sort64 = [&](uint64_t *kin, uint64_t *kout, int32_t *vin, int32_t *vout, int64_t n) -> int {
        size_t bytes = 0;
        uint8_t *tmp = nullptr;
        CLO_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, static_cast<size_t>(n), 0, 64, st));
        CLO_HIP(pool.get(&tmp, bytes));
        CLO_HIP(rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, static_cast<size_t>(n), 0, 64, st));
        return BBFMM_OK;
    };
    int rc = BBFMM_OK;
    int64_t *cs = mesh->closure_stats;

    // ---- open edges: three sorted-pair keys per facet, sorted; a run of one is open
    const int64_t n3 = 3 * nf;
    uint64_t *ekey = nullptr, *eskey = nullptr;
    int32_t *eval = nullptr, *esval = nullptr, *oflag = nullptr, *oidx = nullptr;
    CLO_HIP(pool.get(&ekey, static_cast<size_t>(n3)));
    CLO_HIP(pool.get(&eskey, static_cast<size_t>(n3)));
    CLO_HIP(pool.get(&eval, static_cast<size_t>(n3)));
    CLO_HIP(pool.get(&esval, static_cast<size_t>(n3)));
    CLO_HIP(pool.get(&oflag, static_cast<size_t>(n3)));
    CLO_HIP(pool.get(&oidx, static_cast<size_t>(n3)));
    edge_keys_kernel<<<grid_for(n3), kThreads, 0, st>>>(nf, d_facets, ekey, eval);
    CLO_HIP(hipGetLastError());
    if ((rc = sort64(ekey, eskey, eval, esval, n3)) != BBFMM_OK) return rc;
    open_flags_kernel<<<grid_for(n3), kThreads, 0, st>>>(n3, eskey, esval, oflag);
    CLO_HIP(hipGetLastError());
    int64_t ne = 0;
    if ((rc = scan(oflag, oidx, n3, &ne)) != BBFMM_OK) return rc;
    if (ne == 0) return unchanged();
    int64_t *eab = nullptr;
    int32_t *emask = nullptr;
    double *exyz = nullptr;
    unsigned long long *d_stats = nullptr;
    CLO_HIP(pool.get(&eab, 2 * static_cast<size_t>(ne)));
    CLO_HIP(pool.get(&emask, static_cast<size_t>(ne)));
    CLO_HIP(pool.get(&exyz, 6 * static_cast<size_t>(ne)));
    CLO_HIP(pool.get(&d_stats, 16));
    {
        unsigned long long init[16] = {0, 0, 0, 0, 0, 0, 0, ~0ull, 0, 0, 0, 0, 0, 0, 0, 0};
        CLO_HIP(hipMemcpyAsync(d_stats, init, sizeof(init), hipMemcpyHostToDevice, st));
        CLO_HIP(hipStreamSynchronize(st));
    }
    double *d_axes = nullptr;
    {
        const size_t na = axes[0].size() + axes[1].size() + axes[2].size();
        CLO_HIP(pool.get(&d_axes, na));
        size_t o = 0;
        for (int a = 0; a < 3; ++a) {
            CLO_HIP(hipMemcpyAsync(d_axes + o, axes[a].data(), axes[a].size() * sizeof(double), hipMemcpyHostToDevice, st));
            caps.g[a] = d_axes + o;
            o += axes[a].size();
        }
    }
    open_edges_kernel<<<grid_for(n3), kThreads, 0, st>>>(n3, oflag, oidx, d_facets, d_vertices, caps, eab, emask, exyz, d_stats);
    CLO_HIP(hipGetLastError());
    std::vector<int64_t> h_eab(2 * static_cast<size_t>(ne));
    std::vector<int32_t> h_emask(static_cast<size_t>(ne));
    std::vector<double> h_exyz(6 * static_cast<size_t>(ne));
    unsigned long long h_stats[16];
    CLO_HIP(hipMemcpyAsync(h_stats, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, st));
    CLO_HIP(hipMemcpyAsync(h_eab.data(), eab, h_eab.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    CLO_HIP(hipMemcpyAsync(h_emask.data(), emask, h_emask.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    CLO_HIP(hipMemcpyAsync(h_exyz.data(), exyz, h_exyz.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    CLO_HIP(hipStreamSynchronize(st));
    for (int f = 0; f < 6; ++f) cs[kCloOpen + f] = static_cast<int64_t>(h_stats[f]);
    cs[kCloOffBox] = static_cast<int64_t>(h_stats[6]);
    if (h_stats[6] > 0) {
        const size_t e = static_cast<size_t>(h_stats[7]);
        *err = "isosurface closure: " + std::to_string(h_stats[6]) + " open edge(s) of the mesh do not lie on a face of the extents, the first from vertex " +
               std::to_string(h_eab[2 * e]) + " to vertex " + std::to_string(h_eab[2 * e + 1]) +
               " (the closure takes a mesh that is open only where it was clipped)";
        return BBFMM_BAD_ARGUMENT;
    }

    // ---- cut cells, the vertices on box edges, the compacted lists
    int32_t *cut = nullptr, *cidx = nullptr, *lab = nullptr, *pflag = nullptr, *pidx = nullptr;
    CLO_HIP(pool.get(&cut, static_cast<size_t>(nc)));
    CLO_HIP(pool.get(&cidx, static_cast<size_t>(nc)));
    CLO_HIP(pool.get(&lab, static_cast<size_t>(nc)));
    CLO_HIP(pool.get(&pflag, static_cast<size_t>(nv)));
    CLO_HIP(pool.get(&pidx, static_cast<size_t>(nv)));
    CLO_HIP(hipMemsetAsync(cut, 0, static_cast<size_t>(nc) * sizeof(int32_t), st));
    mark_edges_kernel<<<grid_for(ne), kThreads, 0, st>>>(ne, emask, exyz, caps, cut);
    CLO_HIP(hipGetLastError());
    mark_vertices_kernel<<<grid_for(nv), kThreads, 0, st>>>(nv, d_vertices, caps, cut, pflag);
    CLO_HIP(hipGetLastError());
    int64_t ncut = 0, nper = 0;
    if ((rc = scan(cut, cidx, nc, &ncut)) != BBFMM_OK) return rc;
    if ((rc = scan(pflag, pidx, nv, &nper)) != BBFMM_OK) return rc;
    int32_t *cut_list = nullptr, *nbl = nullptr, *pmask = nullptr, *d_changed = nullptr;
    int64_t *pid = nullptr;
    double *pxyz = nullptr;
    CLO_HIP(pool.get(&cut_list, static_cast<size_t>(ncut)));
    CLO_HIP(pool.get(&nbl, 4 * static_cast<size_t>(ncut)));
    CLO_HIP(pool.get(&pmask, static_cast<size_t>(nper)));
    CLO_HIP(pool.get(&pid, static_cast<size_t>(nper)));
    CLO_HIP(pool.get(&pxyz, 3 * static_cast<size_t>(nper)));
    CLO_HIP(pool.get(&d_changed, 1));
    cut_list_kernel<<<grid_for(nc), kThreads, 0, st>>>(nc, cut, cidx, cut_list, lab);
    CLO_HIP(hipGetLastError());
    perimeter_vertices_kernel<<<grid_for(nv), kThreads, 0, st>>>(nv, pflag, pidx, d_vertices, caps, pid, pmask, pxyz);
    CLO_HIP(hipGetLastError());
    // ---- regions
    for (int round = 0; round < 64; ++round) { // one round hooks everything; the next one finds nothing left
        int32_t changed = 0;
        CLO_HIP(hipMemsetAsync(d_changed, 0, sizeof(int32_t), st));
        region_hook_kernel<<<grid_for(nc), kThreads, 0, st>>>(nc, caps, lab, d_changed);
        CLO_HIP(hipGetLastError());
        region_jump_kernel<<<grid_for(nc), kThreads, 0, st>>>(nc, lab);
        CLO_HIP(hipGetLastError());
        CLO_HIP(hipMemcpyAsync(&changed, d_changed, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        CLO_HIP(hipStreamSynchronize(st));
        if (!changed) break;
    }
    region_count_kernel<<<grid_for(nc), kThreads, 0, st>>>(nc, lab, d_stats + 8);
    CLO_HIP(hipGetLastError());
    cut_neighbours_kernel<<<grid_for(ncut), kThreads, 0, st>>>(ncut, cut_list, caps, lab, nbl);
    CLO_HIP(hipGetLastError());
    std::vector<int32_t> h_cut(static_cast<size_t>(ncut)), h_nbl(4 * static_cast<size_t>(ncut)), h_pmask(static_cast<size_t>(nper));
    std::vector<int64_t> h_pid(static_cast<size_t>(nper));
    std::vector<double> h_pxyz(3 * static_cast<size_t>(nper));
    CLO_HIP(hipMemcpyAsync(h_stats, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, st));
    if (ncut) CLO_HIP(hipMemcpyAsync(h_cut.data(), cut_list, h_cut.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (ncut) CLO_HIP(hipMemcpyAsync(h_nbl.data(), nbl, h_nbl.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (nper) CLO_HIP(hipMemcpyAsync(h_pmask.data(), pmask, h_pmask.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (nper) CLO_HIP(hipMemcpyAsync(h_pid.data(), pid, h_pid.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (nper) CLO_HIP(hipMemcpyAsync(h_pxyz.data(), pxyz, h_pxyz.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    CLO_HIP(hipStreamSynchronize(st));
    cs[kCloRegions] = static_cast<int64_t>(h_stats[8]);

    // ---- the band on the host: one triangulation per face, then the selection over band triangles and regions
    const auto t_host = std::chrono::steady_clock::now();
    Caps hc = caps; // the host's copy reads the axes from the host
    for (int a = 0; a < 3; ++a) hc.g[a] = axes[a].data();
    std::vector<int64_t> band[6];       // per face: 3 provisional ids per triangle, counter-clockwise in (u, v)
    std::vector<int64_t> tri_first(7, 0); // the first band triangle of every face among all of them
    std::unordered_map<std::pair<int64_t, int64_t>, int, PairHash> open_set; // sorted ids of the open edges
    for (int64_t e = 0; e < ne; ++e)
        open_set.emplace(std::make_pair(std::min(h_eab[2 * e], h_eab[2 * e + 1]), std::max(h_eab[2 * e], h_eab[2 * e + 1])), 1);
    std::vector<int64_t> cut_begin(7, 0);
    for (int f = 0; f < 6; ++f)
        cut_begin[f + 1] = std::lower_bound(h_cut.begin(), h_cut.end(), caps.off[f + 1], [](int32_t a, int64_t b) { return int64_t(a) < b; }) - h_cut.begin();
    for (int f = 0; f < 6; ++f) {
        cs[kCloCut + f] = cut_begin[f + 1] - cut_begin[f];
        const int ua = face_u(f), va = face_v(f);
        std::unordered_map<int64_t, int64_t> local; // mesh vertex -> point of this face
        std::vector<double> pts;
        std::vector<int64_t> ids, edges;
        auto point_of = [&](int64_t v, const double *xyz) {
            auto it = local.find(v);
            if (it != local.end()) return it->second;
            const int64_t p = static_cast<int64_t>(ids.size());
            local.emplace(v, p);
            ids.push_back(v);
            pts.push_back(xyz[ua]);
            pts.push_back(xyz[va]);
            return p;
        };
        for (int64_t e = 0; e < ne; ++e)
            if (h_emask[e] & (1 << f)) {
                const int64_t a = point_of(h_eab[2 * e], &h_exyz[6 * e]), b = point_of(h_eab[2 * e + 1], &h_exyz[6 * e + 3]);
                edges.push_back(a);
                edges.push_back(b);
            }
        for (int64_t p = 0; p < nper; ++p)
            if (h_pmask[p] & (1 << f)) point_of(h_pid[p], &h_pxyz[3 * p]);
        std::vector<int32_t> fcut(h_cut.begin() + cut_begin[f], h_cut.begin() + cut_begin[f + 1]);
        for (int32_t &q : fcut) q -= static_cast<int32_t>(caps.off[f]);
        closure::Band B;
        B.nu = caps.n[ua];
        B.nv = caps.n[va];
        B.gu = axes[ua].data();
        B.gv = axes[va].data();
        B.points = pts.data();
        B.n_points = static_cast<int64_t>(ids.size());
        B.edges = edges.data();
        B.n_edges = static_cast<int64_t>(edges.size() / 2);
        B.cut = fcut.data();
        B.n_cut = static_cast<int64_t>(fcut.size());
        B.tol = caps.tol;
        B.key_cell = std::max(box.eps, 1.0e-12);
        std::string terr;
        if (!closure::triangulate_band(&B, &terr)) {
            *err = "isosurface " + terr + " (face " + std::to_string(f) + " of the extents)";
            return BBFMM_BAD_ARGUMENT;
        }
        cs[kCloBandPoints] += static_cast<int64_t>(B.id.size());
        cs[kCloBandDropped] += B.dropped;
        cs[kCloConstraintFlips] += B.constraint_flips;
        cs[kCloLawsonFlips] += B.lawson_flips;
        const int64_t gw = int64_t(B.nu) + 1;
        band[f].resize(B.tri.size());
        for (size_t q = 0; q < B.tri.size(); ++q) {
            const int64_t id = B.id[static_cast<size_t>(B.tri[q])];
            band[f][q] = id >= 0 ? ids[static_cast<size_t>(id)] : nv + grid_key(hc, f, static_cast<int>((-1 - id) % gw), static_cast<int>((-1 - id) / gw));
        }
        tri_first[f + 1] = tri_first[f] + static_cast<int64_t>(B.tri.size() / 3);
    }
    const int64_t n_band = tri_first[6];
    // elements: the band triangles, then one per region label met on the rim
    UnionFind uf;
    for (int64_t t = 0; t < n_band; ++t) uf.make();
    std::unordered_map<int32_t, int64_t> region_el;
    auto region_of = [&](int32_t label) {
        auto it = region_el.find(label);
        if (it != region_el.end()) return it->second;
        const int64_t el = uf.make();
        region_el.emplace(label, el);
        return el;
    };
    std::unordered_map<std::pair<int64_t, int64_t>, int64_t, PairHash> edge_tri; // an edge that is no open edge -> a triangle on it
    std::map<std::tuple<int, int64_t, int64_t>, int64_t> open_side;             // (face, from, to) of an open edge -> its triangle there
    for (int f = 0; f < 6; ++f)
        for (size_t q = 0; q < band[f].size() / 3; ++q) {
            const int64_t t = tri_first[f] + static_cast<int64_t>(q);
            for (int k = 0; k < 3; ++k) {
                const int64_t a = band[f][3 * q + k], b = band[f][3 * q + (k + 1) % 3];
                const auto key = std::make_pair(std::min(a, b), std::max(a, b));
                if (a < nv && b < nv && open_set.count(key)) {
                    open_side[std::make_tuple(f, a, b)] = t;
                    continue;
                }
                auto ins = edge_tri.emplace(key, t);
                if (!ins.second) uf.unite(ins.first->second, t);
            }
        }
    for (int64_t x = 0; x < ncut; ++x) { // a band triangle and a region meet through the grid edge's whole cell
        const int64_t q = h_cut[static_cast<size_t>(x)];
        const int f = face_of_cell(hc, q);
        const int64_t r = q - hc.off[f];
        const int i = static_cast<int>(r % hc.n[face_u(f)]), j = static_cast<int>(r / hc.n[face_u(f)]);
        const int ends[4][4] = {{i, j, i + 1, j}, {i + 1, j, i + 1, j + 1}, {i, j + 1, i + 1, j + 1}, {i, j, i, j + 1}};
        for (int s = 0; s < 4; ++s) {
            const int32_t label = h_nbl[4 * static_cast<size_t>(x) + s];
            if (label < 0) continue;
            const int64_t a = nv + grid_key(hc, f, ends[s][0], ends[s][1]), b = nv + grid_key(hc, f, ends[s][2], ends[s][3]);
            auto it = edge_tri.find(std::make_pair(std::min(a, b), std::max(a, b)));
            if (it == edge_tri.end()) {
                *err = "isosurface closure: internal: the rim of the band of face " + std::to_string(f) + " is not an edge of its triangulation";
                return BBFMM_BAD_ARGUMENT;
            }
            uf.unite(it->second, region_of(label));
        }
    }
    // seeds: on every face of an open edge (a, b), the triangle that holds (b, a) when wound outward
    std::vector<uint8_t> seeded(uf.parent.size(), 0);
    for (int64_t e = 0; e < ne; ++e)
        for (int f = 0; f < 6; ++f) {
            if (!(h_emask[e] & (1 << f))) continue;
            const int64_t a = h_eab[2 * e], b = h_eab[2 * e + 1];
            auto it = face_ccw_outward(f) ? open_side.find(std::make_tuple(f, b, a)) : open_side.find(std::make_tuple(f, a, b));
            if (it != open_side.end()) seeded[static_cast<size_t>(uf.find(it->second))] = 1;
        }
    for (int64_t e = 0; e < ne; ++e)
        for (int f = 0; f < 6; ++f) {
            if (!(h_emask[e] & (1 << f))) continue;
            const int64_t a = h_eab[2 * e], b = h_eab[2 * e + 1];
            auto it = face_ccw_outward(f) ? open_side.find(std::make_tuple(f, a, b)) : open_side.find(std::make_tuple(f, b, a));
            if (it != open_side.end() && seeded[static_cast<size_t>(uf.find(it->second))]) ++cs[kCloConflicts];
        }
    const bool positive = mode == kFinishClosePositive;
    std::vector<int32_t> kept_labels;
    for (const auto &re : region_el)
        if ((seeded[static_cast<size_t>(uf.find(re.second))] != 0) == positive) kept_labels.push_back(re.first);
    std::sort(kept_labels.begin(), kept_labels.end());
    std::vector<int64_t> band_out[6]; // the kept band triangles, wound outward
    for (int f = 0; f < 6; ++f)
        for (size_t q = 0; q < band[f].size() / 3; ++q) {
            if ((seeded[static_cast<size_t>(uf.find(tri_first[f] + static_cast<int64_t>(q)))] != 0) != positive) continue;
            const bool ccw = face_ccw_outward(f);
            band_out[f].push_back(band[f][3 * q]);
            band_out[f].push_back(band[f][3 * q + (ccw ? 1 : 2)]);
            band_out[f].push_back(band[f][3 * q + (ccw ? 2 : 1)]);
            ++cs[kCloBandKept];
        }
    cs[kCloBandHostUs] = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_host).count();

    // ---- the kept whole cells, placed by a scan; the cap facets per face: its whole cells, then its band
    int32_t *rk = cidx, *wk = cut, *widx = nullptr, *d_kept = nullptr; // (cut and cidx are free again)
    CLO_HIP(pool.get(&widx, static_cast<size_t>(nc)));
    CLO_HIP(pool.get(&d_kept, kept_labels.size()));
    CLO_HIP(hipMemsetAsync(rk, 0, static_cast<size_t>(nc) * sizeof(int32_t), st));
    if (!kept_labels.empty()) {
        CLO_HIP(hipMemcpyAsync(d_kept, kept_labels.data(), kept_labels.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        region_flags_kernel<<<grid_for(static_cast<int64_t>(kept_labels.size())), kThreads, 0, st>>>(static_cast<int64_t>(kept_labels.size()), d_kept, rk);
        CLO_HIP(hipGetLastError());
    }
    whole_kept_kernel<<<grid_for(nc), kThreads, 0, st>>>(nc, lab, rk, wk);
    CLO_HIP(hipGetLastError());
    int64_t n_whole = 0;
    if ((rc = scan(wk, widx, nc, &n_whole)) != BBFMM_OK) return rc;
    int32_t w_at[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int f = 1; f < 6; ++f) CLO_HIP(hipMemcpyAsync(&w_at[f], widx + caps.off[f], sizeof(int32_t), hipMemcpyDeviceToHost, st));
    CLO_HIP(hipStreamSynchronize(st));
    w_at[6] = static_cast<int32_t>(n_whole);
    CapBase cb;
    cb.nv_mesh = nv;
    int64_t n_cap = 0, band_at[6];
    for (int f = 0; f < 6; ++f) {
        const int64_t wf = int64_t(w_at[f + 1]) - w_at[f];
        cs[kCloWholeKept + f] = wf;
        cb.base[f] = n_cap - 2 * int64_t(w_at[f]);
        band_at[f] = n_cap + 2 * wf;
        n_cap = band_at[f] + static_cast<int64_t>(band_out[f].size() / 3);
    }
    if (3 * n_cap > 2147483647ll || nv + 3 * n_cap > kFinishMaxVertices) {
        *err = "isosurface closure: " + std::to_string(n_cap) + " cap facets: their corners are counted in 32 bits (use a coarser resolution)";
        return BBFMM_BAD_ARGUMENT;
    }
    const int64_t n3c = 3 * n_cap;
    int64_t *cap = nullptr, *out_f = nullptr;
    CLO_HIP(pool.get(&cap, static_cast<size_t>(n3c)));
    CLO_HIP(pool.get(&out_f, 3 * static_cast<size_t>(nf + n_cap)));
    whole_facets_kernel<<<grid_for(nc), kThreads, 0, st>>>(nc, wk, widx, caps, cb, cap);
    CLO_HIP(hipGetLastError());
    for (int f = 0; f < 6; ++f)
        if (!band_out[f].empty())
            CLO_HIP(hipMemcpyAsync(cap + 3 * band_at[f], band_out[f].data(), band_out[f].size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    mesh_facets_kernel<<<grid_for(nf), kThreads, 0, st>>>(nf, d_facets, positive ? 0 : 1, out_f);
    CLO_HIP(hipGetLastError());
    int64_t n_new = 0;
    double *new_v = nullptr;
    if (n_cap > 0) {
        uint64_t *ckey = nullptr, *cskey = nullptr;
        int32_t *cval = nullptr, *csval = nullptr, *pos = nullptr, *posx = nullptr;
        CLO_HIP(pool.get(&ckey, static_cast<size_t>(n3c)));
        CLO_HIP(pool.get(&cskey, static_cast<size_t>(n3c)));
        CLO_HIP(pool.get(&cval, static_cast<size_t>(n3c)));
        CLO_HIP(pool.get(&csval, static_cast<size_t>(n3c)));
        CLO_HIP(pool.get(&pos, static_cast<size_t>(n3c)));
        CLO_HIP(pool.get(&posx, static_cast<size_t>(n3c)));
        corner_keys_kernel<<<grid_for(n3c), kThreads, 0, st>>>(n3c, cap, ckey, cval);
        CLO_HIP(hipGetLastError());
        if ((rc = sort64(ckey, cskey, cval, csval, n3c)) != BBFMM_OK) return rc;
        CLO_HIP(hipMemsetAsync(pos, 0, static_cast<size_t>(n3c) * sizeof(int32_t), st));
        first_use_kernel<<<grid_for(n3c), kThreads, 0, st>>>(n3c, cskey, csval, static_cast<uint64_t>(nv), pos);
        CLO_HIP(hipGetLastError());
        if ((rc = scan(pos, posx, n3c, &n_new)) != BBFMM_OK) return rc;
        CLO_HIP(pool.get(&new_v, 3 * static_cast<size_t>(n_new)));
        renumber_kernel<<<grid_for(n3c), kThreads, 0, st>>>(n3c, cskey, csval, static_cast<uint64_t>(nv), posx, caps, out_f + 3 * nf, new_v);
        CLO_HIP(hipGetLastError());
    }
    cs[kCloVerticesAdded] = n_new;
    mesh->vertices.resize(3 * static_cast<size_t>(nv + n_new));
    mesh->facets.resize(3 * static_cast<size_t>(nf + n_cap));
    if (nv) CLO_HIP(hipMemcpyAsync(mesh->vertices.data(), d_vertices, 3 * static_cast<size_t>(nv) * sizeof(double), hipMemcpyDeviceToHost, st));
    if (n_new) CLO_HIP(hipMemcpyAsync(mesh->vertices.data() + 3 * nv, new_v, 3 * static_cast<size_t>(n_new) * sizeof(double), hipMemcpyDeviceToHost, st));
    CLO_HIP(hipMemcpyAsync(mesh->facets.data(), out_f, mesh->facets.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    CLO_HIP(hipStreamSynchronize(st));
    return BBFMM_OK;
#undef CLO_HIP
}

} // namespace iso
} // namespace bbfmm
