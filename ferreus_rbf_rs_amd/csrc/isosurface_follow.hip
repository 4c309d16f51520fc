// Following the surface (Request::follow == kFollowSurface; DESIGN.md "Following the surface", numpy restatement:
// tests/isosurface_follow_restatement.py).  The box of E is cut into bricks of B x B x B nodes; seeds are projected onto
// the level set (seed_projection.rs:29-130) and the bricks that hold the corners of their cells are the first frontier.  A round
// evaluates the nodes of E of the frontier's bricks into the resident field (NaN where nothing was evaluated) and marks
// every brick within the halo of the ends of a crossed edge whose two ends are known; the marked bricks not yet visited
// are the next frontier.  The visited set is the closure of the seed bricks under that rule, whatever the order.  Then
// every isovalue goes through the dense extraction of isosurface.hip on the bricks visited for it.
// One thread per node of a brick list, i fastest within a brick; placement by rocPRIM exclusive scans, marks are plain
// stores of 1, no atomics.
#include "isosurface.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <limits>

#include <rocprim/device/device_scan.hpp>

#include "ferreus_bbfmm_hip.h"

// world(ijk) = lo + ijk * spacing as node_coords_kernel computes it: a multiply and then an add, no fused multiply-add.
#pragma clang fp contract(off)

namespace bbfmm {
namespace iso {

namespace {

constexpr int kThreads = 256;
constexpr int64_t kChunkNodes = int64_t(1) << 21; // box nodes of the bricks of one field evaluation

struct Grid {
    int32_t ni, nj, nk;
    int64_t P;    // ni * nj
    int32_t B, B3; // brick side, nodes per brick
    int32_t nbx, nby, nbz;
    int64_t lo[3]; // ijk of box entry (0, 0, 0)
    double lo_world[3], spacing[3];
    const int32_t *e_rows; // per row of the box: i range [begin, end] of E
};

__host__ __device__ inline int32_t brick_of(const Grid &g, int32_t i, int32_t j, int32_t k) {
    return ((k / g.B) * g.nby + j / g.B) * g.nbx + i / g.B;
}

__device__ __forceinline__ double world(const Grid &g, int a, int64_t ijk) { return g.lo_world[a] + static_cast<double>(ijk) * g.spacing[a]; }

// node t of a brick list: its box coordinates; false outside the box (partial bricks at the high ends)
__device__ __forceinline__ bool list_node(const Grid &g, const int32_t *__restrict__ list, int64_t t, int32_t *i, int32_t *j, int32_t *k) {
    const int32_t b = list[t / g.B3], l = static_cast<int32_t>(t % g.B3);
    const int32_t bi = b % g.nbx, bj = (b / g.nbx) % g.nby, bk = b / (g.nbx * g.nby);
    *i = bi * g.B + l % g.B;
    *j = bj * g.B + (l / g.B) % g.B;
    *k = bk * g.B + l / (g.B * g.B);
    return *i < g.ni && *j < g.nj && *k < g.nk;
}

__device__ __forceinline__ bool inside(double v) { return v < -kInsideEps; }

__global__ __launch_bounds__(kThreads) void fill_nan_kernel(int64_t n, double *__restrict__ f) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < n; t += int64_t(gridDim.x) * kThreads) f[t] = __builtin_nan("");
}

// the next frontier (marked and not visited) and its bricks that still need their values
__global__ __launch_bounds__(kThreads) void brick_select_kernel(int32_t nbr, const uint8_t *__restrict__ marked, const uint8_t *__restrict__ visited,
                                                                 const uint8_t *__restrict__ evaluated, int32_t *__restrict__ flag_f,
                                                                 int32_t *__restrict__ flag_e) {
    for (int32_t b = blockIdx.x * kThreads + threadIdx.x; b < nbr; b += gridDim.x * kThreads) {
        const int32_t f = marked[b] && !visited[b] ? 1 : 0;
        flag_f[b] = f;
        flag_e[b] = f && !evaluated[b] ? 1 : 0;
    }
}

// both lists in brick order; counts[0..2): their lengths
__global__ __launch_bounds__(kThreads) void brick_compact_kernel(int32_t nbr, const int32_t *__restrict__ flag_f, const int32_t *__restrict__ idx_f,
                                                                  const int32_t *__restrict__ flag_e, const int32_t *__restrict__ idx_e,
                                                                  int32_t *__restrict__ list_f, int32_t *__restrict__ list_e,
                                                                  uint8_t *__restrict__ visited, uint8_t *__restrict__ evaluated,
                                                                  int32_t *__restrict__ counts) {
    for (int32_t b = blockIdx.x * kThreads + threadIdx.x; b < nbr; b += gridDim.x * kThreads) {
        if (flag_f[b]) {
            list_f[idx_f[b]] = b;
            visited[b] = 1;
        }
        if (flag_e[b]) {
            list_e[idx_e[b]] = b;
            evaluated[b] = 1;
        }
        if (b == nbr - 1) {
            counts[0] = idx_f[b] + flag_f[b];
            counts[1] = idx_e[b] + flag_e[b];
        }
    }
}

// flag[t] = node t of the list is in E (sample points only)
__global__ __launch_bounds__(kThreads) void follow_flags_kernel(Grid g, const int32_t *__restrict__ list, int64_t n, int32_t *__restrict__ flag) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < n; t += int64_t(gridDim.x) * kThreads) {
        int32_t i, j, k;
        int32_t fl = 0;
        if (list_node(g, list, t, &i, &j, &k)) {
            const bool even = ((i + j + k + g.lo[0] + g.lo[1] + g.lo[2]) & 1) == 0;
            const int64_t row = int64_t(k) * g.nj + j;
            fl = even && i >= g.e_rows[2 * row] && i <= g.e_rows[2 * row + 1] ? 1 : 0;
        }
        flag[t] = fl;
    }
}

// the compacted world coordinates of the flagged nodes (SoA), as node_coords_kernel of isosurface.hip
__global__ __launch_bounds__(kThreads) void follow_coords_kernel(Grid g, const int32_t *__restrict__ list, int64_t n, const int32_t *__restrict__ flag,
                                                                  const int32_t *__restrict__ idx, double *__restrict__ x0, double *__restrict__ x1,
                                                                  double *__restrict__ x2) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < n; t += int64_t(gridDim.x) * kThreads) {
        if (!flag[t]) continue;
        int32_t i, j, k;
        list_node(g, list, t, &i, &j, &k);
        const int32_t o = idx[t];
        x0[o] = world(g, 0, g.lo[0] + i);
        x1[o] = world(g, 1, g.lo[1] + j);
        x2[o] = world(g, 2, g.lo[2] + k);
    }
}

// the values of the flagged nodes into the resident field: the evaluated value plus the drift as field_kernel adds it,
// or the caller's value (src, over the box)
__global__ __launch_bounds__(kThreads) void follow_scatter_kernel(Grid g, const int32_t *__restrict__ list, int64_t n, const int32_t *__restrict__ flag,
                                                                   const int32_t *__restrict__ idx, const double *__restrict__ vals,
                                                                   const double *__restrict__ src, bool drift, double a, double b0, double b1,
                                                                   double b2, double *__restrict__ f) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < n; t += int64_t(gridDim.x) * kThreads) {
        if (!flag[t]) continue;
        int32_t i, j, k;
        list_node(g, list, t, &i, &j, &k);
        const int64_t node = int64_t(k) * g.P + int64_t(j) * g.ni + i;
        double v;
        if (src) {
            v = src[node];
        } else {
            v = vals[idx[t]];
            if (drift) {
                const double d = a + b0 * world(g, 0, g.lo[0] + i) + b1 * world(g, 1, g.lo[1] + j) + b2 * world(g, 2, g.lo[2] + k);
                v = v + d;
            }
        }
        f[node] = v;
    }
}

// every brick that holds a node within the halo of node (i, j, k)
__device__ __forceinline__ void mark_halo(const Grid &g, int32_t i, int32_t j, int32_t k, uint8_t *__restrict__ marked) {
    const int32_t i0 = max(i - kFollowHalo[0], 0) / g.B, i1 = min(i + kFollowHalo[0], g.ni - 1) / g.B;
    const int32_t j0 = max(j - kFollowHalo[1], 0) / g.B, j1 = min(j + kFollowHalo[1], g.nj - 1) / g.B;
    const int32_t k0 = max(k - kFollowHalo[2], 0) / g.B, k1 = min(k + kFollowHalo[2], g.nk - 1) / g.B;
    for (int32_t bk = k0; bk <= k1; ++bk)
        for (int32_t bj = j0; bj <= j1; ++bj)
            for (int32_t bi = i0; bi <= i1; ++bi) marked[(bk * g.nby + bj) * g.nbx + bi] = 1;
}

// One thread per node of the frontier's bricks (already visited).  All 14 edges of the node are looked at, the 7 it owns
// and the 7 its neighbours own into it, so that every edge with an end in the frontier and the other end in a visited
// brick is seen in the round that completes it.
__global__ __launch_bounds__(kThreads) void follow_mark_kernel(Grid g, const int32_t *__restrict__ list, int64_t n, const double *__restrict__ f,
                                                                double iso, const uint8_t *__restrict__ visited, uint8_t *__restrict__ marked) {
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < n; t += int64_t(gridDim.x) * kThreads) {
        int32_t i, j, k;
        if (!list_node(g, list, t, &i, &j, &k)) continue;
        const double gp = f[int64_t(k) * g.P + int64_t(j) * g.ni + i] - iso;
        if (!isfinite(gp)) continue; // not in E
        const bool inp = inside(gp);
        bool crossed = false;
        for (int e = 0; e < 14; ++e) {
            const int32_t qi = i + kEdgeDeltas[e][0], qj = j + kEdgeDeltas[e][1], qk = k + kEdgeDeltas[e][2];
            if (qi < 0 || qi >= g.ni || qj < 0 || qj >= g.nj || qk < 0 || qk >= g.nk) continue;
            if (!visited[brick_of(g, qi, qj, qk)]) continue; // (evaluated for another isovalue perhaps: not known to this one)
            const double gq = f[int64_t(qk) * g.P + int64_t(qj) * g.ni + qi] - iso;
            if (!isfinite(gq) || inside(gq) == inp) continue;
            crossed = true;
            mark_halo(g, qi, qj, qk, marked);
        }
        if (crossed) mark_halo(g, i, j, k, marked);
    }
}

// the field on the bricks visited for one isovalue, NaN elsewhere
__global__ __launch_bounds__(kThreads) void follow_mask_kernel(Grid g, const double *__restrict__ f, const uint8_t *__restrict__ visited,
                                                                double *__restrict__ out) {
    const int64_t n = g.P * g.nk;
    for (int64_t t = blockIdx.x * int64_t(kThreads) + threadIdx.x; t < n; t += int64_t(gridDim.x) * kThreads) {
        const int32_t k = static_cast<int32_t>(t / g.P), j = static_cast<int32_t>((t % g.P) / g.ni), i = static_cast<int32_t>(t % g.ni);
        out[t] = visited[brick_of(g, i, j, k)] ? f[t] : __builtin_nan("");
    }
}

// ---- seeds

struct SeedBox {
    double lo[3], hi[3]; // the extents
};

// the positions of the active seeds, compacted; with h > 0 the 7 samples of the central differences per seed
// (seed_projection.rs:151-163): the point, then +h and -h along each axis
__global__ __launch_bounds__(kThreads) void seed_gather_kernel(int32_t n, const int32_t *__restrict__ act, const double *__restrict__ sx0,
                                                                const double *__restrict__ sx1, const double *__restrict__ sx2, double h,
                                                                double *__restrict__ x0, double *__restrict__ x1, double *__restrict__ x2) {
    for (int32_t t = blockIdx.x * kThreads + threadIdx.x; t < n; t += gridDim.x * kThreads) {
        const int32_t s = act[t];
        const double p[3] = {sx0[s], sx1[s], sx2[s]};
        if (!(h > 0.0)) {
            x0[t] = p[0];
            x1[t] = p[1];
            x2[t] = p[2];
            continue;
        }
        for (int q = 0; q < 7; ++q) {
            double c[3] = {p[0], p[1], p[2]};
            if (q > 0) c[(q - 1) / 2] = (q & 1) ? c[(q - 1) / 2] + h : c[(q - 1) / 2] - h;
            x0[7 * int64_t(t) + q] = c[0];
            x1[7 * int64_t(t) + q] = c[1];
            x2[7 * int64_t(t) + q] = c[2];
        }
    }
}

// values and central-difference gradients from the 7 samples (seed_projection.rs:171-175)
__global__ __launch_bounds__(kThreads) void seed_differences_kernel(int32_t n, const double *__restrict__ v7, double h, double *__restrict__ vals,
                                                                     double *__restrict__ grad) {
    for (int32_t t = blockIdx.x * kThreads + threadIdx.x; t < n; t += gridDim.x * kThreads) {
        vals[t] = v7[7 * int64_t(t)];
        for (int a = 0; a < 3; ++a) grad[int64_t(a) * n + t] = (v7[7 * int64_t(t) + 1 + 2 * a] - v7[7 * int64_t(t) + 2 + 2 * a]) / (2.0 * h);
    }
}

// One Newton step per active seed (seed_projection.rs:91-118).  keep[t] = the seed stays active; *any_ok = a step was taken.
__global__ __launch_bounds__(kThreads) void seed_newton_kernel(int32_t n, const int32_t *__restrict__ act, const double *__restrict__ vals,
                                                                const double *__restrict__ grad, bool drift, double da, double db0, double db1,
                                                                double db2, double iso, SeedBox box, double *__restrict__ sx0,
                                                                double *__restrict__ sx1, double *__restrict__ sx2, int32_t *__restrict__ keep,
                                                                int32_t *__restrict__ any_ok) {
    for (int32_t t = blockIdx.x * kThreads + threadIdx.x; t < n; t += gridDim.x * kThreads) {
        const int32_t s = act[t];
        double x[3] = {sx0[s], sx1[s], sx2[s]};
        double v = vals[t], gr[3] = {grad[t], grad[int64_t(n) + t], grad[2 * int64_t(n) + t]};
        if (drift) {
            v = v + (da + db0 * x[0] + db1 * x[1] + db2 * x[2]);
            gr[0] += db0;
            gr[1] += db1;
            gr[2] += db2;
        }
        const double fxi = v - iso;
        if (fabs(fxi) < kSeedTol) {
            keep[t] = 0;
            continue;
        }
        const double g2 = gr[0] * gr[0] + gr[1] * gr[1] + gr[2] * gr[2];
        if (g2 >= kSeedG2Min) {
            const double scale = fxi / g2;
            for (int a = 0; a < 3; ++a) x[a] -= scale * gr[a];
            *any_ok = 1; // a plain store of a constant
        }
        for (int a = 0; a < 3; ++a) x[a] = fmin(fmax(x[a], box.lo[a]), box.hi[a]);
        sx0[s] = x[0];
        sx1[s] = x[1];
        sx2[s] = x[2];
        keep[t] = 1;
    }
}

__global__ __launch_bounds__(kThreads) void seed_compact_kernel(int32_t n, const int32_t *__restrict__ act, const int32_t *__restrict__ keep,
                                                                 const int32_t *__restrict__ idx, int32_t *__restrict__ out, int32_t *__restrict__ counts) {
    for (int32_t t = blockIdx.x * kThreads + threadIdx.x; t < n; t += gridDim.x * kThreads) {
        if (keep[t]) out[idx[t]] = act[t];
        if (t == n - 1) counts[0] = idx[t] + keep[t];
    }
}

// The bricks of every seed's cell are marked: the cell of world_to_ijk (lattice.rs:98-121) is the parallelepiped of
// U, V, W at that origin, whose 8 corners are the origin and the far ends of its 7 owned edges (get_edge_points::<8>).
// Every edge of the cell is a lattice edge between two of them, so a surface through the cell crosses a known edge.
__global__ __launch_bounds__(kThreads) void seed_mark_kernel(Grid g, int32_t n, const double *__restrict__ sx0, const double *__restrict__ sx1,
                                                              const double *__restrict__ sx2, uint8_t *__restrict__ marked) {
    for (int32_t t = blockIdx.x * kThreads + threadIdx.x; t < n; t += gridDim.x * kThreads) {
        const double p[3] = {(sx0[t] - g.lo_world[0]) / g.spacing[0], (sx1[t] - g.lo_world[1]) / g.spacing[1],
                             (sx2[t] - g.lo_world[2]) / g.spacing[2]};
        int64_t c[3];
        seed_cell(p, c);
        for (int q = 0; q < 8; ++q) {
            const int64_t i = c[0] - g.lo[0] + (q ? kEdgeDeltas[q - 1][0] : 0), j = c[1] - g.lo[1] + (q ? kEdgeDeltas[q - 1][1] : 0),
                          k = c[2] - g.lo[2] + (q ? kEdgeDeltas[q - 1][2] : 0);
            if (i < 0 || i >= g.ni || j < 0 || j >= g.nj || k < 0 || k >= g.nk) continue;
            marked[brick_of(g, static_cast<int32_t>(i), static_cast<int32_t>(j), static_cast<int32_t>(k))] = 1;
        }
    }
}

int grid_for(int64_t n) { return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 4096))); }

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

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

#define ISO_HIP(x)                                                                       \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) {                                                          \
            *err = std::string("isosurface: ") + #x + ": " + hipGetErrorString(e_);     \
            return BBFMM_DEVICE_ERROR;                                                   \
        }                                                                                \
    } while (0)

} // namespace

int extract_follow(const Lattice &lat, const FieldFn &field, const Request &req, hipStream_t st, std::vector<Mesh> *meshes,
                   std::string *err) {
    const int64_t ni = lat.dims[0], nj = lat.dims[1], nk = lat.dims[2], P = ni * nj, box = P * nk;
    const int n_iso = req.n_iso;
    const bool cluster = req.cluster != kClusterNone;
    // everything is checked before any work
    if (cluster && req.cluster != kClusterAverage && req.cluster != kClusterCurvature) {
        *err = "isosurface: unknown cluster method " + std::to_string(req.cluster);
        return BBFMM_BAD_ARGUMENT;
    }
    if (req.finish < kFinishRaw || req.finish > kFinishCloseNegative) {
        *err = "isosurface: unknown finish " + std::to_string(req.finish);
        return BBFMM_BAD_ARGUMENT;
    }
    if (req.self_intersections != kSelfIntersectionsIgnore && req.self_intersections != kSelfIntersectionsRollback) {
        *err = "isosurface: unknown self-intersection handling " + std::to_string(req.self_intersections);
        return BBFMM_BAD_ARGUMENT;
    }
    if (req.d_field_in) {
        *err = "isosurface: follow=surface takes its field from the evaluator or from a host array";
        return BBFMM_BAD_ARGUMENT;
    }
    if (!req.host_field && !field) {
        *err = "isosurface: follow=surface needs a field";
        return BBFMM_BAD_ARGUMENT;
    }
    if (req.n_seeds < 0 || (req.n_seeds > 0 && (!req.seeds || req.seeds_ld < req.n_seeds))) {
        *err = "isosurface: follow=surface needs n_seeds >= 0 seeds with seeds_ld >= n_seeds";
        return BBFMM_BAD_ARGUMENT;
    }
    ClipBox ext;
    if (!make_clip_box(req.extents, &ext, err)) return BBFMM_BAD_ARGUMENT;
    int B = 8;
    if (const char *env = std::getenv("BBFMM_ISO_BRICK")) {
        B = !std::strcmp(env, "4") ? 4 : !std::strcmp(env, "8") ? 8 : !std::strcmp(env, "16") ? 16 : 0;
        if (!B) {
            *err = std::string("isosurface: BBFMM_ISO_BRICK must be 4, 8 or 16, got '") + env + "'";
            return BBFMM_BAD_ARGUMENT;
        }
    }
    Grid g;
    g.ni = static_cast<int32_t>(ni);
    g.nj = static_cast<int32_t>(nj);
    g.nk = static_cast<int32_t>(nk);
    g.P = P;
    g.B = B;
    g.B3 = B * B * B;
    g.nbx = static_cast<int32_t>((ni + B - 1) / B);
    g.nby = static_cast<int32_t>((nj + B - 1) / B);
    g.nbz = static_cast<int32_t>((nk + B - 1) / B);
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = lat.lo[a];
        g.lo_world[a] = lat.lo_world[a];
        g.spacing[a] = lat.spacing[a];
    }
    const int64_t nbr64 = int64_t(g.nbx) * g.nby * g.nbz;
    if (nbr64 >= (int64_t(1) << 31)) {
        *err = "isosurface: lattice too large for these extents and resolution";
        return BBFMM_BAD_ARGUMENT;
    }
    const int32_t nbr = static_cast<int32_t>(nbr64);
    const int64_t chunk_bricks = std::max<int64_t>(1, kChunkNodes / g.B3), chunk_nodes = chunk_bricks * g.B3;

    // The field over the box (8 bytes per node; once more for the caller's values, once more for the masked copy of
    // several isovalues), the brick table, one chunk, and what the dense extraction of it then takes.
    {
        size_t free_b = 0, total_b = 0;
        ISO_HIP(hipMemGetInfo(&free_b, &total_b));
        const double fields = 8.0 * static_cast<double>(box) * (1 + (req.host_field ? 1 : 0) + (n_iso > 1 ? 1 : 0));
        const double bricks = static_cast<double>(nbr) * (17.0 + 2.0 * n_iso), chunk = static_cast<double>(chunk_nodes) * (8 + 5 * 8 + 128);
        const double dense = (cluster ? (req.cluster == kClusterCurvature ? 48.0 : 40.0) * static_cast<double>(nk + 2) * static_cast<double>(P) : 0.0) +
                             std::min(static_cast<double>(req.budget_bytes > 0 ? req.budget_bytes : (int64_t(1) << 31)),
                                      64.0 * static_cast<double>(box));
        const double need = fields + bricks + chunk + dense;
        if (need > static_cast<double>(free_b)) {
            *err = "isosurface: follow=surface keeps the field of the " + std::to_string(ni) + " x " + std::to_string(nj) + " x " +
                   std::to_string(nk) + " lattice box on the device, about " + std::to_string(static_cast<int64_t>(need / 1048576.0)) +
                   " MiB with the extraction; " + std::to_string(free_b / 1048576) +
                   " MiB are free (use a coarser resolution or smaller extents)";
            return BBFMM_BAD_ARGUMENT;
        }
    }

    // ---- seeds: clamped to the extents, one per lattice cell, the first of each (seed_projection.rs:44-60); an open
    // hash table of the cells' box indices
    const auto t_dedupe = std::chrono::steady_clock::now();
    std::vector<double> sp[3];
    {
        size_t cap = 16;
        while (cap < 2 * static_cast<size_t>(req.n_seeds)) cap <<= 1;
        std::vector<uint64_t> table(cap, 0); // key + 1, 0: free
        for (int64_t s = 0; s < req.n_seeds; ++s) {
            double p[3], q[3];
            bool ok = true;
            for (int a = 0; a < 3; ++a) {
                const double v = req.seeds[a * req.seeds_ld + s];
                if (!std::isfinite(v)) ok = false;
                p[a] = std::min(std::max(v, ext.lo[a]), ext.hi[a]);
                q[a] = (p[a] - lat.lo_world[a]) / lat.spacing[a];
            }
            if (!ok) {
                *err = "isosurface: seed " + std::to_string(s) + " is not finite";
                return BBFMM_BAD_ARGUMENT;
            }
            int64_t c[3];
            seed_cell(q, c);
            const int64_t i = c[0] - lat.lo[0], j = c[1] - lat.lo[1], k = c[2] - lat.lo[2];
            if (i < 0 || i >= ni || j < 0 || j >= nj || k < 0 || k >= nk) continue; // (a cell of a clamped point lies in the box)
            const uint64_t key = static_cast<uint64_t>(k * P + j * ni + i) + 1;
            size_t slot = static_cast<size_t>((key * 0x9E3779B97F4A7C15ull) >> 20) & (cap - 1);
            while (table[slot] != 0 && table[slot] != key) slot = (slot + 1) & (cap - 1);
            if (table[slot] == key) continue;
            table[slot] = key;
            for (int a = 0; a < 3; ++a) sp[a].push_back(p[a]);
        }
    }
    const double dedupe_ms = ms_since(t_dedupe);
    const int64_t n_cells64 = static_cast<int64_t>(sp[0].size());
    if (n_cells64 >= (int64_t(1) << 28)) {
        *err = "isosurface: more than 2^28 distinct seed cells";
        return BBFMM_BAD_ARGUMENT;
    }
    const int32_t n_cells = static_cast<int32_t>(n_cells64);

    Pool pool;
    int32_t *d_erows = nullptr;
    ISO_HIP(pool.get(&d_erows, lat.e_rows.size()));
    ISO_HIP(hipMemcpyAsync(d_erows, lat.e_rows.data(), lat.e_rows.size() * 4, hipMemcpyHostToDevice, st));
    g.e_rows = d_erows;
    double *f = nullptr, *src = nullptr, *masked = nullptr;
    ISO_HIP(pool.get(&f, static_cast<size_t>(box)));
    fill_nan_kernel<<<grid_for(box), kThreads, 0, st>>>(box, f);
    ISO_HIP(hipGetLastError());
    if (req.host_field) {
        ISO_HIP(pool.get(&src, static_cast<size_t>(box)));
        ISO_HIP(hipMemcpyAsync(src, req.host_field, static_cast<size_t>(box) * sizeof(double), hipMemcpyHostToDevice, st));
    }
    // brick table
    uint8_t *evaluated = nullptr, *marked = nullptr;
    std::vector<uint8_t *> visited(n_iso, nullptr);
    int32_t *flag_f = nullptr, *idx_f = nullptr, *flag_e = nullptr, *idx_e = nullptr, *list_f = nullptr, *list_e = nullptr, *counts = nullptr;
    ISO_HIP(pool.get(&evaluated, static_cast<size_t>(nbr)));
    ISO_HIP(pool.get(&marked, static_cast<size_t>(nbr)));
    ISO_HIP(hipMemsetAsync(evaluated, 0, static_cast<size_t>(nbr), st));
    for (int q = 0; q < n_iso; ++q) {
        ISO_HIP(pool.get(&visited[q], static_cast<size_t>(nbr)));
        ISO_HIP(hipMemsetAsync(visited[q], 0, static_cast<size_t>(nbr), st));
    }
    ISO_HIP(pool.get(&flag_f, static_cast<size_t>(nbr)));
    ISO_HIP(pool.get(&idx_f, static_cast<size_t>(nbr)));
    ISO_HIP(pool.get(&flag_e, static_cast<size_t>(nbr)));
    ISO_HIP(pool.get(&idx_e, static_cast<size_t>(nbr)));
    ISO_HIP(pool.get(&list_f, static_cast<size_t>(nbr)));
    ISO_HIP(pool.get(&list_e, static_cast<size_t>(nbr)));
    ISO_HIP(pool.get(&counts, 4));
    // one chunk of nodes
    int32_t *nflag = nullptr, *nidx = nullptr;
    double *xs[3] = {nullptr, nullptr, nullptr}, *vals = nullptr;
    ISO_HIP(pool.get(&nflag, static_cast<size_t>(chunk_nodes)));
    ISO_HIP(pool.get(&nidx, static_cast<size_t>(chunk_nodes)));
    if (!req.host_field) {
        for (auto &x : xs) ISO_HIP(pool.get(&x, static_cast<size_t>(chunk_nodes / 2 + 8)));
        ISO_HIP(pool.get(&vals, static_cast<size_t>(chunk_nodes / 2 + 8)));
    }
    // seeds on the device
    const bool project = !req.host_field && n_cells > 0;
    const bool differences = project && !req.grad;
    double *sx[3] = {nullptr, nullptr, nullptr}, *sx0[3] = {nullptr, nullptr, nullptr}, *ax[3] = {nullptr, nullptr, nullptr};
    double *svals = nullptr, *sgrad = nullptr, *sv7 = nullptr;
    int32_t *act = nullptr, *act2 = nullptr, *keep = nullptr, *kidx = nullptr;
    for (int a = 0; a < 3; ++a) {
        ISO_HIP(pool.get(&sx[a], static_cast<size_t>(n_cells)));
        ISO_HIP(pool.get(&sx0[a], static_cast<size_t>(n_cells)));
        if (n_cells) ISO_HIP(hipMemcpyAsync(sx0[a], sp[a].data(), static_cast<size_t>(n_cells) * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (project) {
        const size_t per = differences ? 7 : 1;
        for (auto &x : ax) ISO_HIP(pool.get(&x, per * n_cells));
        ISO_HIP(pool.get(&svals, static_cast<size_t>(n_cells)));
        ISO_HIP(pool.get(&sgrad, 3 * static_cast<size_t>(n_cells)));
        if (differences) ISO_HIP(pool.get(&sv7, 7 * static_cast<size_t>(n_cells)));
        ISO_HIP(pool.get(&act, static_cast<size_t>(n_cells)));
        ISO_HIP(pool.get(&act2, static_cast<size_t>(n_cells)));
        ISO_HIP(pool.get(&keep, static_cast<size_t>(n_cells)));
        ISO_HIP(pool.get(&kidx, static_cast<size_t>(n_cells)));
    }
    size_t scan_bytes = 0, b2 = 0;
    ISO_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, nflag, nidx, int32_t(0), static_cast<size_t>(chunk_nodes), rocprim::plus<int32_t>(), st));
    ISO_HIP(rocprim::exclusive_scan(nullptr, b2, flag_f, idx_f, int32_t(0), static_cast<size_t>(std::max<int32_t>(nbr, std::max<int32_t>(n_cells, 1))),
                                    rocprim::plus<int32_t>(), st));
    scan_bytes = std::max(scan_bytes, b2);
    void *scan_tmp = nullptr;
    ISO_HIP(pool.get(reinterpret_cast<uint8_t **>(&scan_tmp), scan_bytes));
    int32_t *h_counts = nullptr;
    ISO_HIP(hipHostMalloc(reinterpret_cast<void **>(&h_counts), 4 * sizeof(int32_t)));
    struct PinnedFree {
        int32_t *p;
        ~PinnedFree() { (void)hipHostFree(p); }
    } pin_guard{h_counts};
    ISO_HIP(hipStreamSynchronize(st)); // (pageable sources)

    const bool drift = req.drift != nullptr && !req.host_field;
    const double da = drift ? req.drift[0] : 0, db0 = drift ? req.drift[1] : 0, db1 = drift ? req.drift[2] : 0, db2 = drift ? req.drift[3] : 0;
    SeedBox sbox;
    for (int a = 0; a < 3; ++a) {
        sbox.lo[a] = ext.lo[a];
        sbox.hi[a] = ext.hi[a];
    }
    // central_difference_step (seed_projection.rs:181-190)
    const double cd_h = std::max(std::fabs(std::min({lat.spacing[0], lat.spacing[1], lat.spacing[2]})), 1.0e-4) * 1.0e-4;

    meshes->assign(n_iso, Mesh());
    std::vector<double> seed_ms(n_iso, 0.0), wave_ms(n_iso, 0.0);
    for (int q = 0; q < n_iso; ++q) {
        const auto t_seed = std::chrono::steady_clock::now();
        const double iso = req.isovalues[q];
        Mesh &mesh = (*meshes)[q];
        mesh.follow_stats[kFolSeeds] = req.n_seeds;
        mesh.follow_stats[kFolCells] = n_cells;
        mesh.follow_stats[kFolNodesE] = lat.n_nodes;
        ISO_HIP(hipMemsetAsync(marked, 0, static_cast<size_t>(nbr), st));
        for (int a = 0; a < 3; ++a)
            if (n_cells) ISO_HIP(hipMemcpyAsync(sx[a], sx0[a], static_cast<size_t>(n_cells) * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (project) {
            std::vector<int32_t> all(static_cast<size_t>(n_cells));
            for (int32_t s = 0; s < n_cells; ++s) all[s] = s;
            ISO_HIP(hipMemcpyAsync(act, all.data(), all.size() * 4, hipMemcpyHostToDevice, st));
            ISO_HIP(hipStreamSynchronize(st));
            int32_t n_act = n_cells;
            for (int step = 0; step < kSeedNewtonSteps && n_act > 0; ++step) {
                const int gs = grid_for(n_act);
                seed_gather_kernel<<<gs, kThreads, 0, st>>>(n_act, act, sx[0], sx[1], sx[2], differences ? cd_h : 0.0, ax[0], ax[1], ax[2]);
                ISO_HIP(hipGetLastError());
                int rc;
                if (differences) {
                    if ((rc = field(ax[0], ax[1], ax[2], 7 * int64_t(n_act), sv7)) != BBFMM_OK) return rc;
                    seed_differences_kernel<<<gs, kThreads, 0, st>>>(n_act, sv7, cd_h, svals, sgrad);
                    ISO_HIP(hipGetLastError());
                } else if ((rc = req.grad(ax[0], ax[1], ax[2], n_act, svals, sgrad)) != BBFMM_OK) {
                    return rc;
                }
                ++mesh.follow_stats[kFolNewton];
                ISO_HIP(hipMemsetAsync(counts + 1, 0, sizeof(int32_t), st));
                seed_newton_kernel<<<gs, kThreads, 0, st>>>(n_act, act, svals, sgrad, drift, da, db0, db1, db2, iso, sbox, sx[0], sx[1], sx[2],
                                                            keep, counts + 1);
                ISO_HIP(hipGetLastError());
                size_t bytes = scan_bytes;
                ISO_HIP(rocprim::exclusive_scan(scan_tmp, bytes, keep, kidx, int32_t(0), static_cast<size_t>(n_act), rocprim::plus<int32_t>(), st));
                seed_compact_kernel<<<gs, kThreads, 0, st>>>(n_act, act, keep, kidx, act2, counts);
                ISO_HIP(hipGetLastError());
                ISO_HIP(hipMemcpyAsync(h_counts, counts, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
                ISO_HIP(hipStreamSynchronize(st));
                std::swap(act, act2);
                n_act = h_counts[0];
                if (!h_counts[1]) break; // no step was taken
            }
        }
        if (n_cells) {
            seed_mark_kernel<<<grid_for(n_cells), kThreads, 0, st>>>(g, n_cells, sx[0], sx[1], sx[2], marked);
            ISO_HIP(hipGetLastError());
        }
        ISO_HIP(hipStreamSynchronize(st));
        seed_ms[q] = ms_since(t_seed) + (q == 0 ? dedupe_ms : 0.0);

        // ---- rounds
        const auto t_wave = std::chrono::steady_clock::now();
        const int gb = grid_for(nbr);
        for (;;) {
            brick_select_kernel<<<gb, kThreads, 0, st>>>(nbr, marked, visited[q], evaluated, flag_f, flag_e);
            ISO_HIP(hipGetLastError());
            size_t bytes = scan_bytes;
            ISO_HIP(rocprim::exclusive_scan(scan_tmp, bytes, flag_f, idx_f, int32_t(0), static_cast<size_t>(nbr), rocprim::plus<int32_t>(), st));
            bytes = scan_bytes;
            ISO_HIP(rocprim::exclusive_scan(scan_tmp, bytes, flag_e, idx_e, int32_t(0), static_cast<size_t>(nbr), rocprim::plus<int32_t>(), st));
            brick_compact_kernel<<<gb, kThreads, 0, st>>>(nbr, flag_f, idx_f, flag_e, idx_e, list_f, list_e, visited[q], evaluated, counts);
            ISO_HIP(hipGetLastError());
            ISO_HIP(hipMemcpyAsync(h_counts, counts, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            ISO_HIP(hipStreamSynchronize(st));
            const int64_t n_front = h_counts[0], n_eval = h_counts[1];
            if (n_front == 0) break;
            if (mesh.follow_stats[kFolRounds] == 0) mesh.follow_stats[kFolSeedBricks] = n_front;
            ++mesh.follow_stats[kFolRounds];
            for (int64_t c0 = 0; c0 < n_eval; c0 += chunk_bricks) {
                const int64_t nb = std::min(chunk_bricks, n_eval - c0), n = nb * g.B3;
                const int gn = grid_for(n);
                follow_flags_kernel<<<gn, kThreads, 0, st>>>(g, list_e + c0, n, nflag);
                ISO_HIP(hipGetLastError());
                bytes = scan_bytes;
                ISO_HIP(rocprim::exclusive_scan(scan_tmp, bytes, nflag, nidx, int32_t(0), static_cast<size_t>(n), rocprim::plus<int32_t>(), st));
                if (!req.host_field) {
                    ISO_HIP(hipMemcpyAsync(&h_counts[2], nidx + n - 1, 4, hipMemcpyDeviceToHost, st));
                    ISO_HIP(hipMemcpyAsync(&h_counts[3], nflag + n - 1, 4, hipMemcpyDeviceToHost, st));
                    ISO_HIP(hipStreamSynchronize(st));
                    const int64_t m = int64_t(h_counts[2]) + h_counts[3];
                    if (m == 0) continue;
                    follow_coords_kernel<<<gn, kThreads, 0, st>>>(g, list_e + c0, n, nflag, nidx, xs[0], xs[1], xs[2]);
                    ISO_HIP(hipGetLastError());
                    const int rc = field(xs[0], xs[1], xs[2], m, vals);
                    if (rc != BBFMM_OK) return rc;
                }
                follow_scatter_kernel<<<gn, kThreads, 0, st>>>(g, list_e + c0, n, nflag, nidx, vals, src, drift, da, db0, db1, db2, f);
                ISO_HIP(hipGetLastError());
            }
            follow_mark_kernel<<<grid_for(n_front * g.B3), kThreads, 0, st>>>(g, list_f, n_front * g.B3, f, iso, visited[q], marked);
            ISO_HIP(hipGetLastError());
        }
        wave_ms[q] = ms_since(t_wave);
        // the bricks visited for this isovalue and their nodes of E
        std::vector<uint8_t> h_vis(static_cast<size_t>(nbr));
        ISO_HIP(hipMemcpyAsync(h_vis.data(), visited[q], h_vis.size(), hipMemcpyDeviceToHost, st));
        ISO_HIP(hipStreamSynchronize(st));
        const int64_t par0 = lat.lo[0] + lat.lo[1] + lat.lo[2];
        mesh.follow_dims[0] = B;
        mesh.follow_dims[1] = g.nbx;
        mesh.follow_dims[2] = g.nby;
        mesh.follow_dims[3] = g.nbz;
        mesh.follow_bricks = h_vis;
        for (int32_t b = 0; b < nbr; ++b) {
            if (!h_vis[b]) continue;
            ++mesh.follow_stats[kFolBricks];
            const int64_t bi = b % g.nbx, bj = (b / g.nbx) % g.nby, bk = b / (g.nbx * g.nby);
            for (int64_t k = bk * B; k < std::min<int64_t>(nk, (bk + 1) * B); ++k)
                for (int64_t j = bj * B; j < std::min<int64_t>(nj, (bj + 1) * B); ++j) {
                    const int64_t row = k * nj + j;
                    int64_t lo = std::max<int64_t>(lat.e_rows[2 * row], bi * B), hi = std::min<int64_t>(lat.e_rows[2 * row + 1], (bi + 1) * B - 1);
                    if ((lo + j + k + par0) & 1) ++lo;
                    if (lo <= hi) mesh.follow_stats[kFolNodes] += (hi - lo) / 2 + 1;
                }
        }
    }
    if (req.d_field_out) ISO_HIP(hipMemcpyAsync(req.d_field_out, f, static_cast<size_t>(box) * sizeof(double), hipMemcpyDeviceToDevice, st));

    // ---- the dense extraction of each isovalue on the bricks visited for it
    // the working arrays of the wavefront are not needed any more
    pool.put(src);
    pool.put(nflag);
    pool.put(nidx);
    for (auto &x : xs) pool.put(x);
    pool.put(vals);
    for (auto &x : ax) pool.put(x);
    pool.put(sv7);
    if (n_iso > 1) ISO_HIP(pool.get(&masked, static_cast<size_t>(box)));
    for (int q = 0; q < n_iso; ++q) {
        const auto t_ext = std::chrono::steady_clock::now();
        if (n_iso > 1) {
            follow_mask_kernel<<<grid_for(box), kThreads, 0, st>>>(g, f, visited[q], masked);
            ISO_HIP(hipGetLastError());
        }
        Request sub;
        sub.isovalues = req.isovalues + q;
        sub.n_iso = 1;
        sub.d_field_in = n_iso > 1 ? masked : f;
        sub.budget_bytes = req.budget_bytes;
        sub.cluster = req.cluster;
        sub.finish = req.finish;
        sub.extents = req.extents;
        sub.self_intersections = req.self_intersections;
        std::vector<Mesh> one;
        const int rc = extract(lat, FieldFn(), sub, st, &one, err);
        if (rc != BBFMM_OK) return rc;
        Mesh &mesh = (*meshes)[q];
        std::memcpy(one[0].follow_stats, mesh.follow_stats, sizeof(mesh.follow_stats));
        std::memcpy(one[0].follow_dims, mesh.follow_dims, sizeof(mesh.follow_dims));
        one[0].follow_bricks = std::move(mesh.follow_bricks);
        one[0].follow_ms[0] = seed_ms[q];
        one[0].follow_ms[1] = wave_ms[q];
        one[0].follow_ms[2] = ms_since(t_ext);
        mesh = std::move(one[0]);
    }
    return BBFMM_OK;
#undef ISO_HIP
}

} // namespace iso
} // namespace bbfmm
