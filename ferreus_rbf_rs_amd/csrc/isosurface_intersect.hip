// The self-intersection detector on the device (isosurface.hpp, self_intersections_device): the set of
// get_intersecting_triangles (ferreus_rmt/src/mesh_intersections.rs:163-208), with a uniform grid over the facets'
// bounding boxes in place of its R-tree.  One thread per facet, grid-stride, no LDS; placement by a rocPRIM scan and one
// stable radix sort; the flags are plain stores of one value and the integer atomics only count, so the result does not
// depend on thread order.
//
// Broad phase: h is the largest side of a kept facet's bounding box (one reduction), widened by 2^-10 so that the
// rounding of the quotients below cannot part two boxes that touch; a facet's cell is floor((box_min - lo) / h) per axis,
// clamped to +-2^40 (monotone, so cells of overlapping boxes still differ by at most 1 per axis).  Two boxes can overlap
// only if box_min differs by at most the larger side, hence by at most 1 cell per axis: thread a probes the 27 cells
// around its own by binary search over the sorted 64-bit cell keys and takes the entries b > a that lie in the probed
// cell (a key collision costs this comparison, never a pair, and no pair is met twice) and whose boxes overlap on closed
// intervals (locate_in_envelope_intersecting).  Narrow phase, in the same kernel: the six corners are loaded only for
// those pairs and go through triangle_pair (isosurface_intersect.hpp).
#include "isosurface.hpp"
#include "isosurface_intersect.hpp"

#include <algorithm>
#include <cmath>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>

#include "ferreus_bbfmm_hip.h"

// the quotients (box_min - lo) / h are a subtraction and then a division, as the restatement of the grid computes them
#pragma clang fp contract(off)

namespace bbfmm {
namespace iso {

namespace {

constexpr int kThreads = 256;
constexpr int64_t kCellClamp = int64_t(1) << 40;

int grid_for(int64_t n) {
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 4096)));
}

// Device allocations of one self_intersections_device() call, freed on every exit.
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

struct Grid {
    double lo[3];
    double h;
};

// keep[t] = every corner of facet t inside the box (facet_fully_inside_aabb, aabb_clipping.rs:108-129)
__global__ __launch_bounds__(kThreads) void inside_kernel(int64_t nf, const double *__restrict__ verts, const int64_t *__restrict__ facets,
                                                           ClipBox b, int32_t *__restrict__ keep) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nf; t += int64_t(gridDim.x) * kThreads) {
        bool in = true;
        for (int k = 0; k < 3; ++k) {
            const double *p = verts + 3 * facets[3 * t + k];
            for (int plane = 0; plane < 6; ++plane) in = in && clip_inside_plane(p, plane, b);
        }
        keep[t] = in ? 1 : 0;
    }
}

// The kept facets in facet order (kept[c] = t), their boxes (lo, hi) and the largest side of each.
__global__ __launch_bounds__(kThreads) void boxes_kernel(int64_t nf, const double *__restrict__ verts, const int64_t *__restrict__ facets,
                                                          const int32_t *__restrict__ keep, const int32_t *__restrict__ kidx,
                                                          int32_t *__restrict__ kept, double *__restrict__ box, double *__restrict__ side) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nf; t += int64_t(gridDim.x) * kThreads) {
        if (keep && !keep[t]) continue;
        const int64_t c = keep ? kidx[t] : t;
        double lo[3], hi[3];
        for (int k = 0; k < 3; ++k) {
            const double *p = verts + 3 * facets[3 * t + k];
            for (int a = 0; a < 3; ++a) {
                lo[a] = k == 0 || p[a] < lo[a] ? p[a] : lo[a];
                hi[a] = k == 0 || p[a] > hi[a] ? p[a] : hi[a];
            }
        }
        double s = 0.0;
        for (int a = 0; a < 3; ++a) {
            box[6 * c + a] = lo[a];
            box[6 * c + 3 + a] = hi[a];
            const double d = hi[a] - lo[a];
            s = d > s ? d : s;
        }
        kept[c] = static_cast<int32_t>(t);
        side[c] = s;
    }
}

__device__ __forceinline__ int64_t grid_cell(double v, double lo, double h) {
    const double q = floor((v - lo) / h);
    if (!(q == q)) return 0;
    if (q >= static_cast<double>(kCellClamp)) return kCellClamp;
    if (q <= -static_cast<double>(kCellClamp)) return -kCellClamp;
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

__global__ __launch_bounds__(kThreads) void cell_keys_kernel(int64_t nk, const double *__restrict__ box, Grid g, uint64_t *__restrict__ key,
                                                              int32_t *__restrict__ val) {
    for (int64_t c = blockIdx.x * int64_t(kThreads) + threadIdx.x; c < nk; c += int64_t(gridDim.x) * kThreads) {
        key[c] = cell_hash(grid_cell(box[6 * c], g.lo[0], g.h), grid_cell(box[6 * c + 1], g.lo[1], g.h),
                           grid_cell(box[6 * c + 2], g.lo[2], g.h));
        val[c] = static_cast<int32_t>(c);
    }
}

// the boxes in sorted order: a probe reads contiguous memory
__global__ __launch_bounds__(kThreads) void sorted_boxes_kernel(int64_t nk, const int32_t *__restrict__ sval, const double *__restrict__ box,
                                                                 double *__restrict__ sbox) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < 6 * nk; i += int64_t(gridDim.x) * kThreads)
        sbox[i] = box[6 * int64_t(sval[i / 6]) + i % 6];
}

// sval: from the kept index to the facet (same order, so b > a means the same)
__global__ __launch_bounds__(kThreads) void facet_values_kernel(int64_t nk, const int32_t *__restrict__ kept, int32_t *__restrict__ sval) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < nk; i += int64_t(gridDim.x) * kThreads) sval[i] = kept[sval[i]];
}

__device__ __forceinline__ int64_t lower_bound(const uint64_t *__restrict__ skey, int64_t n, uint64_t h) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skey[mid] < h) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t neighbour_hash(const int64_t q[3], int d) {
    return cell_hash(q[0] + (d % 3 - 1), q[1] + (d / 3 % 3 - 1), q[2] + (d / 9 - 1));
}

// The work of the pair kernel before it runs: per facet the entries under the keys of its 27 cells.
__global__ __launch_bounds__(kThreads) void probe_estimate_kernel(int64_t nk, const uint64_t *__restrict__ skey, const double *__restrict__ sbox,
                                                                   Grid g, unsigned long long *__restrict__ total) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < nk; i += int64_t(gridDim.x) * kThreads) {
        const int64_t q[3] = {grid_cell(sbox[6 * i], g.lo[0], g.h), grid_cell(sbox[6 * i + 1], g.lo[1], g.h),
                              grid_cell(sbox[6 * i + 2], g.lo[2], g.h)};
        unsigned long long n = 0;
        for (int d = 0; d < 27; ++d) {
            const uint64_t h = neighbour_hash(q, d);
            const int64_t b = lower_bound(skey, nk, h);
            if (b < nk && skey[b] == h) n += static_cast<unsigned long long>((h == ~uint64_t(0) ? nk : lower_bound(skey, nk, h + 1)) - b);
        }
        atomicAdd(total, n); // a count only
    }
}

__device__ __forceinline__ Tri3 load_triangle(const double *__restrict__ verts, const int64_t id[3]) {
    Tri3 t;
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) t.p[k].x[a] = verts[3 * id[k] + a];
    return t;
}

// Broad and narrow phase (see the head of the file).  Entry i of the sorted arrays is facet a = sval[i].
__global__ __launch_bounds__(kThreads) void pairs_kernel(int64_t nk, const uint64_t *__restrict__ skey, const int32_t *__restrict__ sval,
                                                          const double *__restrict__ sbox, Grid g, const double *__restrict__ verts, const int64_t *__restrict__ facets,
                                                          uint8_t *__restrict__ tri_flag, unsigned long long *__restrict__ counts) {
    for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < nk; i += int64_t(gridDim.x) * kThreads) {
        const int32_t a = sval[i];
        double ba[6];
        for (int x = 0; x < 6; ++x) ba[x] = sbox[6 * i + x];
        const int64_t q[3] = {grid_cell(ba[0], g.lo[0], g.h), grid_cell(ba[1], g.lo[1], g.h), grid_cell(ba[2], g.lo[2], g.h)};
        const int64_t ia[3] = {facets[3 * int64_t(a)], facets[3 * int64_t(a) + 1], facets[3 * int64_t(a) + 2]};
        Tri3 A;
        bool have_a = false;
        unsigned long long n_box = 0, n_moller = 0, n_true = 0;
        for (int d = 0; d < 27; ++d) {
            const int64_t qd[3] = {q[0] + (d % 3 - 1), q[1] + (d / 3 % 3 - 1), q[2] + (d / 9 - 1)};
            const uint64_t h = cell_hash(qd[0], qd[1], qd[2]);
            for (int64_t j = lower_bound(skey, nk, h); j < nk && skey[j] == h; ++j) {
                const int32_t b = sval[j];
                if (b <= a) continue;
                const double *bb = sbox + 6 * j;
                if (grid_cell(bb[0], g.lo[0], g.h) != qd[0] || grid_cell(bb[1], g.lo[1], g.h) != qd[1] ||
                    grid_cell(bb[2], g.lo[2], g.h) != qd[2])
                    continue; // another cell under the same key
                if (!(ba[0] <= bb[3] && bb[0] <= ba[3] && ba[1] <= bb[4] && bb[1] <= ba[4] && ba[2] <= bb[5] && bb[2] <= ba[5])) continue;
                ++n_box;
                if (!have_a) {
                    A = load_triangle(verts, ia);
                    have_a = true;
                }
                const int64_t ib[3] = {facets[3 * int64_t(b)], facets[3 * int64_t(b) + 1], facets[3 * int64_t(b) + 2]};
                const Tri3 B = load_triangle(verts, ib);
                int stage;
                const bool hit = triangle_pair(A, ia, B, ib, &stage);
                if (stage > kPairMoller) ++n_moller;
                if (hit) {
                    ++n_true;
                    tri_flag[a] = 1; // plain stores of one value
                    tri_flag[b] = 1;
                }
            }
        }
        if (n_box) atomicAdd(&counts[kIsectBoxPairs], n_box); // counts only
        if (n_moller) atomicAdd(&counts[kIsectMoller], n_moller);
        if (n_true) atomicAdd(&counts[kIsectTrue], n_true);
    }
}

__global__ __launch_bounds__(kThreads) void count_flags_kernel(int64_t nf, const uint8_t *__restrict__ tri_flag, unsigned long long *__restrict__ n) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < nf; t += int64_t(gridDim.x) * kThreads)
        if (tri_flag[t]) atomicAdd(n, 1ull); // a count only
}

} // namespace

int self_intersections_device(const double *d_vertices, int64_t nv, const int64_t *d_facets, int64_t nf, const ClipBox *box,
                              hipStream_t st, uint8_t *d_tri_flag, int64_t *stats, std::string *err) {
#define ISECT_HIP(x)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) {                                                                       \
            *err = std::string("isosurface self-intersections: ") + #x + ": " + hipGetErrorString(e_); \
            return BBFMM_DEVICE_ERROR;                                                                \
        }                                                                                             \
    } while (0)
    for (int q = 0; q < kIsectStats; ++q) stats[q] = 0;
    if (nv < 0 || nf < 0 || nf > kFinishMaxFacets) {
        *err = "isosurface self-intersections: a mesh of " + std::to_string(nf) + " facets is too large to search (at most " +
               std::to_string(kFinishMaxFacets) + ": facet ids are sorted as 32-bit values)";
        return BBFMM_BAD_ARGUMENT;
    }
    if (nf == 0) return BBFMM_OK;
    ISECT_HIP(hipMemsetAsync(d_tri_flag, 0, static_cast<size_t>(nf), st));
    Pool pool;
    unsigned long long *d_counts = nullptr; // kIsectStats counters and the estimate
    ISECT_HIP(pool.get(&d_counts, kIsectStats + 1));
    ISECT_HIP(hipMemsetAsync(d_counts, 0, (kIsectStats + 1) * sizeof(unsigned long long), st));

    // ---- inside filter: the kept facets, in facet order
    int32_t *keep = nullptr, *kidx = nullptr;
    int64_t nk = nf;
    if (box) {
        ISECT_HIP(pool.get(&keep, static_cast<size_t>(nf)));
        ISECT_HIP(pool.get(&kidx, static_cast<size_t>(nf)));
        inside_kernel<<<grid_for(nf), kThreads, 0, st>>>(nf, d_vertices, d_facets, *box, keep);
        ISECT_HIP(hipGetLastError());
        size_t bytes = 0;
        uint8_t *tmp = nullptr;
        ISECT_HIP(rocprim::exclusive_scan(nullptr, bytes, keep, kidx, int32_t(0), static_cast<size_t>(nf), rocprim::plus<int32_t>(), st));
        ISECT_HIP(pool.get(&tmp, bytes));
        ISECT_HIP(rocprim::exclusive_scan(tmp, bytes, keep, kidx, int32_t(0), static_cast<size_t>(nf), rocprim::plus<int32_t>(), st));
        int32_t last[2] = {0, 0};
        ISECT_HIP(hipMemcpyAsync(&last[0], kidx + nf - 1, 4, hipMemcpyDeviceToHost, st));
        ISECT_HIP(hipMemcpyAsync(&last[1], keep + nf - 1, 4, hipMemcpyDeviceToHost, st));
        ISECT_HIP(hipStreamSynchronize(st));
        pool.put(tmp);
        nk = int64_t(last[0]) + last[1];
    }
    stats[kIsectKept] = nk;
    if (nk < 2) return BBFMM_OK;

    // ---- boxes and the cell size
    int32_t *kept = nullptr;
    double *bx = nullptr, *side = nullptr, *d_h = nullptr;
    ISECT_HIP(pool.get(&kept, static_cast<size_t>(nk)));
    ISECT_HIP(pool.get(&bx, 6 * static_cast<size_t>(nk)));
    ISECT_HIP(pool.get(&side, static_cast<size_t>(nk)));
    ISECT_HIP(pool.get(&d_h, 1));
    boxes_kernel<<<grid_for(nf), kThreads, 0, st>>>(nf, d_vertices, d_facets, keep, kidx, kept, bx, side);
    ISECT_HIP(hipGetLastError());
    Grid g;
    {
        size_t bytes = 0;
        uint8_t *tmp = nullptr;
        ISECT_HIP(rocprim::reduce(nullptr, bytes, side, d_h, 0.0, static_cast<size_t>(nk), rocprim::maximum<double>(), st));
        ISECT_HIP(pool.get(&tmp, bytes));
        ISECT_HIP(rocprim::reduce(tmp, bytes, side, d_h, 0.0, static_cast<size_t>(nk), rocprim::maximum<double>(), st));
        double h = 0.0;
        ISECT_HIP(hipMemcpyAsync(&h, d_h, sizeof(double), hipMemcpyDeviceToHost, st));
        ISECT_HIP(hipStreamSynchronize(st));
        pool.put(tmp);
        if (!std::isfinite(h)) {
            *err = "isosurface self-intersections: the mesh has a vertex that is not finite";
            return BBFMM_BAD_ARGUMENT;
        }
        g.h = h > 0.0 ? h * (1.0 + 1.0 / 1024.0) : 1.0; // all kept facets are points: any grid will do
        for (int a = 0; a < 3; ++a) g.lo[a] = box ? box->lo[a] : 0.0;
    }
    pool.put(side);
    pool.put(keep);
    pool.put(kidx);

    // ---- sort by cell key
    uint64_t *ckey = nullptr, *skey = nullptr;
    int32_t *cval = nullptr, *sval = nullptr;
    double *sbox = nullptr;
    uint8_t *sort_tmp = nullptr;
    ISECT_HIP(pool.get(&ckey, static_cast<size_t>(nk)));
    ISECT_HIP(pool.get(&skey, static_cast<size_t>(nk)));
    ISECT_HIP(pool.get(&cval, static_cast<size_t>(nk)));
    ISECT_HIP(pool.get(&sval, static_cast<size_t>(nk)));
    cell_keys_kernel<<<grid_for(nk), kThreads, 0, st>>>(nk, bx, g, ckey, cval);
    ISECT_HIP(hipGetLastError());
    size_t sort_bytes = 0;
    ISECT_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, ckey, skey, cval, sval, static_cast<size_t>(nk), 0, 64, st));
    ISECT_HIP(pool.get(&sort_tmp, sort_bytes));
    ISECT_HIP(rocprim::radix_sort_pairs(sort_tmp, sort_bytes, ckey, skey, cval, sval, static_cast<size_t>(nk), 0, 64, st));
    ISECT_HIP(pool.get(&sbox, 6 * static_cast<size_t>(nk)));
    sorted_boxes_kernel<<<grid_for(6 * nk), kThreads, 0, st>>>(nk, sval, bx, sbox);
    ISECT_HIP(hipGetLastError());
    facet_values_kernel<<<grid_for(nk), kThreads, 0, st>>>(nk, kept, sval);
    ISECT_HIP(hipGetLastError());

    // ---- a grid that makes the probe quadratic is refused before any pair is tested
    probe_estimate_kernel<<<grid_for(nk), kThreads, 0, st>>>(nk, skey, sbox, g, d_counts + kIsectStats);
    ISECT_HIP(hipGetLastError());
    unsigned long long estimate = 0;
    ISECT_HIP(hipMemcpyAsync(&estimate, d_counts + kIsectStats, sizeof(estimate), hipMemcpyDeviceToHost, st));
    ISECT_HIP(hipStreamSynchronize(st));
    pool.put(ckey);
    pool.put(cval);
    pool.put(sort_tmp);
    pool.put(bx);
    pool.put(kept);
    const unsigned long long bound = static_cast<unsigned long long>(std::max<int64_t>(kIsectPairFloor, kIsectPairsPerFacet * nk));
    if (estimate > bound) {
        *err = "isosurface self-intersections: the largest facet (bounding box side " + std::to_string(g.h) + ") sets a grid on which " +
               std::to_string(nk) + " facets meet " + std::to_string(estimate) + " candidates in the 27 cells around them, more than " +
               std::to_string(bound) + ": the search would be quadratic (split the large facets or remove them)";
        return BBFMM_BAD_ARGUMENT;
    }

    pairs_kernel<<<grid_for(nk), kThreads, 0, st>>>(nk, skey, sval, sbox, g, d_vertices, d_facets, d_tri_flag, d_counts);
    ISECT_HIP(hipGetLastError());
    count_flags_kernel<<<grid_for(nf), kThreads, 0, st>>>(nf, d_tri_flag, d_counts + kIsectTriangles);
    ISECT_HIP(hipGetLastError());
    unsigned long long h_counts[kIsectStats];
    ISECT_HIP(hipMemcpyAsync(h_counts, d_counts, sizeof(h_counts), hipMemcpyDeviceToHost, st));
    ISECT_HIP(hipStreamSynchronize(st));
    for (int q = kIsectBoxPairs; q <= kIsectTriangles; ++q) stats[q] = static_cast<int64_t>(h_counts[q]);
    return BBFMM_OK;
#undef ISECT_HIP
}

} // namespace iso
} // namespace bbfmm
