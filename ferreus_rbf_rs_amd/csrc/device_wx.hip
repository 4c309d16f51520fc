// W and X lists: M2P, P2L and their fused unordered-pair pass (targets = sources), with launchers and job-size knobs.
#include "device_direct.hpp"

namespace bbfmm {

// Stage the Chebyshev nodes of `cell` (scale_cheb_nodes_to_cell, chebyshev.rs:951-968) and
// its coefficients as a source tile (n <= DIRECT_TILE assumed per chunk).
template <int KB>
__device__ inline void stage_nodes(SrcTile<KB> &tile, const DevCheb *chp, int P1, int P2, int j0, int cnt, double cx,
                                   double cy, double cz, double half, int d, const double *coef, int64_t coef_stride,
                                   int kb, int tid, int nthreads) {
    for (int j = tid; j < cnt; j += nthreads) {
        const int I = j0 + j;
        const int i2 = I % P2, i1 = (I / P2) % P1, i0 = I / (P2 * P1);
        const double x = cx + half * chp->nodes[i0];
        const double y = d > 1 ? cy + half * chp->nodes[i1] : 0.0;
        const double z = d > 2 ? cz + half * chp->nodes[i2] : 0.0;
        tile.xy[j] = make_double2(x, y);
        tile.zs[j] = z;
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) tile.w[kk][j] = (kk < kb && coef) ? coef[kk * coef_stride + I] : 0.0;
    }
}

// multipole_to_particle (bbfmm.rs:1254-1355).  One workgroup per (target leaf, chunk of its W
// list); chunks of one leaf add into the same targets with hardware f64 atomics.
template <int KID, bool GRAD, int KB>
__global__ __launch_bounds__(256) void m2p_kernel(KernelSpec ks, const DevCheb *__restrict__ chp,
                                                  const int32_t *__restrict__ tgt_begin,
                                                  const int32_t *__restrict__ tgt_end,
                                                  const int64_t *__restrict__ w_begin,
                                                  const int64_t *__restrict__ w_end,
                                                  const int32_t *__restrict__ w_cells,
                                                  const double *__restrict__ centers,
                                                  const double *__restrict__ lengths, Xyz tgt, int64_t n_tgt, int k0,
                                                  int kb, int64_t C, const double *__restrict__ M,
                                                  double *__restrict__ out, double *__restrict__ grad, int fixed_plan) {
    __shared__ SrcTile<KB> tile;
    __shared__ double red[256];
    const int p = chp->p, d = chp->d, n = chp->n, n_pad = chp->n_pad;
    int P0, P1, P2;
    axis_sizes(p, d, P0, P1, P2);
    const int tid = threadIdx.x;
    const int job = blockIdx.x;
    const int t0 = tgt_begin[job], t1 = tgt_end[job];
    const int64_t r0 = w_begin[job], r1 = w_end[job]; // a chunk of the leaf's W list
    const TargetPlan tp = plan_targets(t1 - t0, fixed_plan);
    for (int tc = t0; tc < t1; tc += tp.n_c) {
        const int nt = min(tp.n_c, t1 - tc);
        const int ti = tid % tp.pairs, sl = tid / tp.pairs;
        const bool part = sl < tp.S && ti < nt;
        const bool two = ti + tp.pairs < nt;
        double t[2][3] = {{0, 0, 0}, {0, 0, 0}};
        if (part) {
            const int ia = tc + ti, ib = two ? ia + tp.pairs : ia;
            t[0][0] = tgt.x[ia], t[0][1] = tgt.y[ia], t[0][2] = tgt.z[ia];
            t[1][0] = tgt.x[ib], t[1][1] = tgt.y[ib], t[1][2] = tgt.z[ib];
        }
        double acc[2][KB], gacc[2][KB][3];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) acc[h][kk] = gacc[h][kk][0] = gacc[h][kk][1] = gacc[h][kk][2] = 0.0;
        for (int64_t r = r0; r < r1; ++r) {
            const int wc = w_cells[r];
            const double half = lengths[wc] * 0.5;
            const double cx = centers[wc * 3], cy = centers[wc * 3 + 1], cz = centers[wc * 3 + 2];
            const double *coef = M + ((int64_t)k0 * C + wc) * n_pad;
            for (int j0 = 0; j0 < n; j0 += DIRECT_TILE) {
                const int cnt = min(DIRECT_TILE, n - j0);
                __syncthreads();
                stage_nodes(tile, chp, P1, P2, j0, cnt, cx, cy, cz, half, d, coef, C * n_pad, kb, tid, 256);
                __syncthreads();
                if (part) direct_tile<KID, GRAD, KB>(ks, tile, cnt, sl, tp.S, t, acc, gacc);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool wr = part && sl == 0 && (h == 0 || two);
            const int64_t it = tc + ti + h * tp.pairs;
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) {
                if (kk >= kb) break;
                const double v = slice_reduce(acc[h][kk], red, ti, sl, tp.S, tp.pairs, part);
                if (wr) unsafeAtomicAdd(&out[(int64_t)(k0 + kk) * n_tgt + it], v);
                if (GRAD) {
                    for (int a = 0; a < d; ++a) {
                        const double g = slice_reduce(gacc[h][kk][a], red, ti, sl, tp.S, tp.pairs, part);
                        if (wr) unsafeAtomicAdd(&grad[((int64_t)(k0 + kk) * d + a) * n_tgt + it], g);
                    }
                }
            }
        }
    }
}

// multipole_to_particle and particle_to_local in one pass when targets = sources (one rhs): X = W^T
// (linear_tree.rs:388-392), so the values phi(x_t, node) of a leaf's points against the Chebyshev nodes of its
// W cells are exactly the values P2L needs for those cells' X lists.  Same scheme as p2p_sym_kernel with the
// nodes of the W cells as columns: row sums (x M_W[node]) are M2P (bbfmm.rs:1254-1355), column sums (x w_t)
// are P2L (bbfmm.rs:1001-1048), added to L with f64 atomics after M2L stage 2 has assigned it.
struct WxJobs {
    int n_jobs;
    const int32_t *tgt_begin, *tgt_end; // rows of job i (sorted source positions, at most SYM_WAVES * SYM_TR, one leaf)
    const int64_t *w_range;             // 2 per job: the leaf's range in w_cells
    const int32_t *w_cells;
};

// KB right-hand sides per pass like p2p_sym_kernel: rhs k reads ws + k * ldw and M + k * C * n_pad, adds to
// out + k * ldo and L + k * C * n_pad.
template <int KID, int KB>
__global__ __launch_bounds__(64 * SYM_WAVES) void wx_sym_kernel(KernelSpec ks, WxJobs jobs, const DevCheb *__restrict__ chp,
                                                               const double *__restrict__ centers,
                                                               const double *__restrict__ lengths, Xyz src,
                                                               const double *__restrict__ ws, int64_t ldw, int kb,
                                                               const double *__restrict__ M, double *__restrict__ L,
                                                               int64_t ld_ml, double *__restrict__ out, int64_t ldo,
                                                               int out_off, int out_n) {
    constexpr int T = sym_tile<KB>();
    constexpr int TRP = sym_rows_pass<KB>();
    __shared__ SymTile<KB> tile;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int job = blockIdx.x;
    const int p = chp->p, d = chp->d, n = chp->n, n_pad = chp->n_pad;
    int P0, P1, P2;
    axis_sizes(p, d, P0, P1, P2);
    const int t0 = jobs.tgt_begin[job], t1 = jobs.tgt_end[job];
    const int rpw = (t1 - t0 + SYM_WAVES - 1) / SYM_WAVES;
    const int r_lo = min(t0 + wave * rpw, t1);
    const int nr = min(rpw, t1 - r_lo);
    double racc[SYM_TR][KB];
#pragma unroll
    for (int r = 0; r < SYM_TR; ++r)
#pragma unroll
        for (int k = 0; k < KB; ++k) racc[r][k] = 0.0;
    const int64_t q0 = jobs.w_range[2 * job], q1 = jobs.w_range[2 * job + 1];
    const int64_t total = (q1 - q0) * n;
    for (int64_t base = 0; base < total; base += T) {
        const int fill = static_cast<int>(min<int64_t>(T, total - base));
        __syncthreads();
        for (int j = tid; j < fill; j += 64 * SYM_WAVES) {
            const int64_t P = base + j;
            const int ci = static_cast<int>(P / n), I = static_cast<int>(P - static_cast<int64_t>(ci) * n);
            const int cell = jobs.w_cells[q0 + ci];
            const double half = lengths[cell] * 0.5;
            const int i2 = I % P2, i1 = (I / P2) % P1, i0 = I / (P2 * P1); // scale_cheb_nodes_to_cell, chebyshev.rs:951-968
            tile.x[j] = centers[cell * 3] + half * chp->nodes[i0];
            tile.y[j] = d > 1 ? centers[cell * 3 + 1] + half * chp->nodes[i1] : 0.0;
            tile.z[j] = d > 2 ? centers[cell * 3 + 2] + half * chp->nodes[i2] : 0.0;
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                tile.w[k][j] = M[min(k, kb - 1) * ld_ml + static_cast<int64_t>(cell) * n_pad + I];
                tile.col[k][j] = 0.0;
            }
            tile.cidx[j] = cell * n_pad + I;
        }
        __syncthreads();
#pragma unroll
        for (int pp = 0; pp < SYM_TR; pp += TRP) {
            if (pp < nr) { // wave-uniform
                double tx[TRP], ty[TRP], tz[TRP], tw[TRP][KB];
#pragma unroll
                for (int r = 0; r < TRP; ++r) {
                    const int g = min(r_lo + min(pp + r, nr - 1), t1 - 1);
                    tx[r] = src.x[g], ty[r] = src.y[g], tz[r] = src.z[g];
#pragma unroll
                    for (int k = 0; k < KB; ++k) tw[r][k] = keep_if(pp + r < nr, ws[min(k, kb - 1) * ldw + g]);
                }
                for (int j = lane; j < fill; j += 64) {
                    const double xs = tile.x[j], ys = tile.y[j], zs = tile.z[j];
                    double wj[KB], csum[KB];
#pragma unroll
                    for (int k = 0; k < KB; ++k) wj[k] = tile.w[k][j], csum[k] = 0.0;
#pragma unroll
                    for (int r = 0; r < TRP; ++r) {
                        if (pp + r < SYM_TR) { // (rows past nr: clamped copies with weight 0, their row sums are dropped)
                            const double dx = tx[r] - xs, dy = ty[r] - ys, dz = tz[r] - zs;
                            const double v = kernel_value_r2<KID>(ks, dx * dx + dy * dy + dz * dz);
#pragma unroll
                            for (int k = 0; k < KB; ++k) {
                                racc[pp + r < SYM_TR ? pp + r : 0][k] += v * wj[k];
                                csum[k] += v * tw[r][k];
                            }
                        }
                    }
#pragma unroll
                    for (int k = 0; k < KB; ++k)
                        if (k < kb) unsafeAtomicAdd(&tile.col[k][j], csum[k]);
                }
            }
        }
        __syncthreads();
        for (int j = tid; j < fill; j += 64 * SYM_WAVES) {
#pragma unroll
            for (int k = 0; k < KB; ++k)
                if (k < kb) unsafeAtomicAdd(&L[k * ld_ml + tile.cidx[j]], tile.col[k][j]);
        }
    }
#pragma unroll
    for (int r = 0; r < SYM_TR; ++r) {
        if (r < nr) {
            // (a partition's output holds its own rows only: out_off = first owned row; the rows of a leaf outside are
            // here for their column sums -- P2L into the partition's cells -- alone)
            const int o = r_lo + r - out_off;
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                if (k < kb) {
                    const double s = wave_sum(racc[r][k]);
                    if (lane == 0 && o >= 0 && o < out_n) unsafeAtomicAdd(&out[k * ldo + o], s);
                }
            }
        }
    }
}

// The fused M2P + P2L pass for ONE right-hand side on whole leaves (round 6): like p2p_sym3_kernel with the Chebyshev nodes
// of a chunk of the leaf's W cells as columns.  A job = (all rows of a leaf -- up to wx_sym3_rows_per_job(), bigger ones in
// equal parts) x (a chunk of its W list): the nodes of a cell are staged and their column sums flushed to L once per leaf
// instead of once per 48 rows, and no padded row is evaluated.
template <int KID, int MAXR>
__global__ __launch_bounds__(64 * SYM_WAVES) void wx_sym3_kernel(KernelSpec ks, WxJobs jobs, const DevCheb *__restrict__ chp,
                                                                const double *__restrict__ centers,
                                                                const double *__restrict__ lengths, Xyz src,
                                                                const double *__restrict__ ws, const double *__restrict__ M,
                                                                double *__restrict__ L, double *__restrict__ out, int out_off,
                                                                int out_n) {
    constexpr int T = sym_tile<1>();
    __shared__ SymTile<1> tile;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int job = blockIdx.x;
    const int p = chp->p, d = chp->d, n = chp->n, n_pad = chp->n_pad;
    int P0, P1, P2;
    axis_sizes(p, d, P0, P1, P2);
    const int t0 = jobs.tgt_begin[job], t1 = jobs.tgt_end[job];
    const int rows = t1 - t0, base_r = rows / SYM_WAVES, extra = rows - base_r * SYM_WAVES;
    const int nr = base_r + (wave < extra ? 1 : 0);
    const int r_lo = t0 + wave * base_r + min(wave, extra); // sorted source position of the wave's first row
    const int64_t q0 = jobs.w_range[2 * job], q1 = jobs.w_range[2 * job + 1];
    const int64_t total = (q1 - q0) * n;
    for (int64_t base = 0; base < total; base += T) {
        const int fill = static_cast<int>(min<int64_t>(T, total - base));
        __syncthreads();
        for (int j = tid; j < fill; j += 64 * SYM_WAVES) {
            const int64_t P = base + j;
            const int ci = static_cast<int>(P / n), I = static_cast<int>(P - static_cast<int64_t>(ci) * n);
            const int cell = jobs.w_cells[q0 + ci];
            const double half = lengths[cell] * 0.5;
            const int i2 = I % P2, i1 = (I / P2) % P1, i0 = I / (P2 * P1); // scale_cheb_nodes_to_cell, chebyshev.rs:951-968
            tile.x[j] = centers[cell * 3] + half * chp->nodes[i0];
            tile.y[j] = d > 1 ? centers[cell * 3 + 1] + half * chp->nodes[i1] : 0.0;
            tile.z[j] = d > 2 ? centers[cell * 3 + 2] + half * chp->nodes[i2] : 0.0;
            tile.w[0][j] = M[static_cast<int64_t>(cell) * n_pad + I];
            tile.col[0][j] = 0.0;
            tile.cidx[j] = cell * n_pad + I;
        }
        __syncthreads();
        // (a partition's output holds its own rows only: out_off = first owned row; the rows of a leaf outside are here for
        // their column sums -- P2L into the partition's cells -- alone)
        sym3_rows<KID, MAXR, true>(ks, tile, fill, lane, r_lo, r_lo - out_off, nr, src, ws, out, 0, out_n);
        __syncthreads();
        for (int j = tid; j < fill; j += 64 * SYM_WAVES) unsafeAtomicAdd(&L[tile.cidx[j]], tile.col[0][j]);
    }
}

// particle_to_local (bbfmm.rs:1001-1048).  One workgroup per cell with an X list; the
// targets are the cell's Chebyshev nodes.
template <int KID, int KB>
__global__ __launch_bounds__(256) void p2l_kernel(KernelSpec ks, const DevCheb *__restrict__ chp,
                                                  const int32_t *__restrict__ cells,
                                                  const int64_t *__restrict__ run_ptr,
                                                  const int32_t *__restrict__ runs,
                                                  const double *__restrict__ centers,
                                                  const double *__restrict__ lengths, Xyz src,
                                                  const double *__restrict__ ws, int64_t N, int k0, int kb, int64_t C,
                                                  double *__restrict__ L) {
    __shared__ SrcTile<KB> tile;
    __shared__ double red[256];
    const int p = chp->p, d = chp->d, n = chp->n, n_pad = chp->n_pad;
    int P0, P1, P2;
    axis_sizes(p, d, P0, P1, P2);
    const int tid = threadIdx.x;
    const int job = blockIdx.x;
    const int cell = cells[job];
    const double half = lengths[cell] * 0.5;
    const double cx = centers[cell * 3], cy = centers[cell * 3 + 1], cz = centers[cell * 3 + 2];
    const int64_t r0 = run_ptr[job], r1 = run_ptr[job + 1];
    const TargetPlan tp = plan_targets(n);
    for (int tc = 0; tc < n; tc += tp.n_c) {
        const int nt = min(tp.n_c, n - tc);
        const int ti = tid % tp.pairs, sl = tid / tp.pairs;
        const bool part = sl < tp.S && ti < nt;
        const bool two = ti + tp.pairs < nt;
        double t[2][3] = {{0, 0, 0}, {0, 0, 0}};
        if (part) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int I = tc + ti + ((h && two) ? tp.pairs : 0);
                const int i2 = I % P2, i1 = (I / P2) % P1, i0 = I / (P2 * P1);
                t[h][0] = cx + half * chp->nodes[i0];
                t[h][1] = d > 1 ? cy + half * chp->nodes[i1] : 0.0;
                t[h][2] = d > 2 ? cz + half * chp->nodes[i2] : 0.0;
            }
        }
        double acc[2][KB], gacc[2][KB][3];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) acc[h][kk] = 0.0;
        for (int64_t r = r0; r < r1; ++r) {
            const int sb = runs[2 * r], se = runs[2 * r + 1];
            for (int base = sb; base < se; base += DIRECT_TILE) {
                const int cnt = min(DIRECT_TILE, se - base);
                __syncthreads();
                for (int j = tid; j < cnt; j += 256) {
                    tile.xy[j] = make_double2(src.x[base + j], src.y[base + j]);
                    tile.zs[j] = src.z[base + j];
#pragma unroll
                    for (int kk = 0; kk < KB; ++kk)
                        tile.w[kk][j] = kk < kb ? ws[(int64_t)(k0 + kk) * N + base + j] : 0.0;
                }
                __syncthreads();
                if (part) direct_tile<KID, false, KB>(ks, tile, cnt, sl, tp.S, t, acc, gacc);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool wr = part && sl == 0 && (h == 0 || two);
#pragma unroll
            for (int kk = 0; kk < KB; ++kk) {
                if (kk >= kb) break;
                const double v = slice_reduce(acc[h][kk], red, ti, sl, tp.S, tp.pairs, part);
                if (wr) L[((int64_t)(k0 + kk) * C + cell) * n_pad + tc + ti + h * tp.pairs] += v;
            }
        }
    }
}

// ------------------------------------------------------------------ launchers and job-size knobs
int wx_sym_rows_per_job() { return SYM_WAVES * SYM_TR; }
// rows per whole-leaf job of the one-rhs fused pass (BBFMM_WX_SYM_LEAF=<rows>; 0: none, the chunk jobs serve one rhs too)
int wx_sym3_rows_per_job() {
    static const int v = sym3_rows_knob("BBFMM_WX_SYM_LEAF", 256);
    return v;
}

void launch_wx_sym(const KernelSpec &ks, const ChebRef &ch, int n_jobs, const int32_t *tgt_begin, const int32_t *tgt_end,
                   const int64_t *w_range, int n_leaf_jobs, const int32_t *l_tgt_begin, const int32_t *l_tgt_end,
                   const int64_t *l_w_range, const int32_t *w_cells, const double *centers, const double *lengths,
                   const double *const *src_xyz, const double *w_sorted, int64_t ldw, int K, const double *M, double *L,
                   int64_t ld_ml, double *out_sorted, int64_t ldo, int out_off, int out_n, hipStream_t s) {
    if (n_jobs == 0) return;
    const WxJobs jobs{n_jobs, tgt_begin, tgt_end, w_range, w_cells};
    const WxJobs ljobs{n_leaf_jobs, l_tgt_begin, l_tgt_end, l_w_range, w_cells};
    dispatch_kernel_id(ks.id, [&](auto idc) {
        constexpr int ID = decltype(idc)::value;
        for (int k0 = 0; k0 < K; k0 += kSymMaxRhs) { // (an 8-slot instance would be bound by its LDS traffic)
            const int kb = std::min(kSymMaxRhs, K - k0);
#define WX_GO(KBV)                                                                                                    \
    hipLaunchKernelGGL((wx_sym_kernel<ID, KBV>), dim3(n_jobs), dim3(64 * SYM_WAVES), 0, s, ks, jobs, ch.dev, centers,    \
                       lengths, make_xyz(src_xyz), w_sorted + static_cast<int64_t>(k0) * ldw, ldw, kb,                 \
                       M + static_cast<int64_t>(k0) * ld_ml, L + static_cast<int64_t>(k0) * ld_ml, ld_ml,               \
                       out_sorted + static_cast<int64_t>(k0) * ldo, ldo, out_off, out_n)
            if (kb == 1 && n_leaf_jobs > 0 && p2p_sym3_max_rows_per_pass() == 8) // one rhs: whole leaves (the same rows and W cells as the chunk jobs)
                hipLaunchKernelGGL((wx_sym3_kernel<ID, 8>), dim3(n_leaf_jobs), dim3(64 * SYM_WAVES), 0, s, ks, ljobs, ch.dev, centers, lengths,
                                   make_xyz(src_xyz), w_sorted + static_cast<int64_t>(k0) * ldw, M + static_cast<int64_t>(k0) * ld_ml,
                                   L + static_cast<int64_t>(k0) * ld_ml, out_sorted + static_cast<int64_t>(k0) * ldo, out_off, out_n);
            else if (kb == 1 && n_leaf_jobs > 0)
                hipLaunchKernelGGL((wx_sym3_kernel<ID, 6>), dim3(n_leaf_jobs), dim3(64 * SYM_WAVES), 0, s, ks, ljobs, ch.dev, centers, lengths,
                                   make_xyz(src_xyz), w_sorted + static_cast<int64_t>(k0) * ldw, M + static_cast<int64_t>(k0) * ld_ml,
                                   L + static_cast<int64_t>(k0) * ld_ml, out_sorted + static_cast<int64_t>(k0) * ldo, out_off, out_n);
            else if (kb == 1) WX_GO(1);
            else if (kb == 2) WX_GO(2);
            else WX_GO(4);
#undef WX_GO
        }
    });
}

void launch_m2p(const KernelSpec &ks, const ChebRef &ch, int n_jobs, const int32_t *tgt_begin,
                const int32_t *tgt_end, const int64_t *w_begin, const int64_t *w_end,
                const int32_t *w_cells, const double *centers,
                const double *lengths, const double *const *tgt_xyz, int64_t n_tgt, int K, int64_t C,
                const double *M, double *out_sorted, double *grad_sorted, hipStream_t s, bool fixed_plan) {
    if (n_jobs == 0) return;
    dispatch_kernel_id(ks.id, [&](auto idc) {
        constexpr int ID = decltype(idc)::value;
        for (int k0 = 0; k0 < K; k0 += DIRECT_KB) {
            const int kb = std::min(DIRECT_KB, K - k0);
            auto go = [&](auto grad, auto kbv) {
                hipLaunchKernelGGL((m2p_kernel<ID, decltype(grad)::value, decltype(kbv)::value>), dim3(n_jobs), dim3(256), 0, s, ks, ch.dev,
                                   tgt_begin, tgt_end, w_begin, w_end, w_cells, centers, lengths, make_xyz(tgt_xyz), n_tgt, k0, kb, C, M,
                                   out_sorted, grad_sorted, fixed_plan ? 1 : 0);
            };
            if (grad_sorted && kb == 1) go(std::true_type{}, int_c<1>{});
            else if (grad_sorted) go(std::true_type{}, int_c<DIRECT_KB>{});
            else if (kb == 1) go(std::false_type{}, int_c<1>{});
            else go(std::false_type{}, int_c<DIRECT_KB>{});
        }
    });
}

void launch_p2l(const KernelSpec &ks, const ChebRef &ch, int n_jobs, const int32_t *cells, const int64_t *run_ptr,
                const int32_t *runs, const double *centers, const double *lengths, const double *const *src_xyz,
                const double *w_sorted, int64_t N, int K, int64_t C, double *L, hipStream_t s) {
    if (n_jobs == 0) return;
    dispatch_kernel_id(ks.id, [&](auto idc) {
        constexpr int ID = decltype(idc)::value;
        for (int k0 = 0; k0 < K; k0 += DIRECT_KB) {
            const int kb = std::min(DIRECT_KB, K - k0);
            auto go = [&](auto kbv) {
                hipLaunchKernelGGL((p2l_kernel<ID, decltype(kbv)::value>), dim3(n_jobs), dim3(256), 0, s, ks, ch.dev, cells, run_ptr, runs,
                                   centers, lengths, make_xyz(src_xyz), w_sorted, N, k0, kb, C, L);
            };
            if (kb == 1) go(int_c<1>{});
            else go(int_c<DIRECT_KB>{});
        }
    });
}

} // namespace bbfmm
