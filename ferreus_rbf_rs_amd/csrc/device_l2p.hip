// L2P: the local expansion of a leaf evaluated at its targets, with its launcher.
#include "device_common.hpp"

namespace bbfmm {

// ------------------------------------------------------------------ L2P
// local_to_particle (bbfmm.rs:1358-1440): y[t] += S(x_t) . L_leaf, optionally gradients
// (dS scaled by 2/length, chebyshev.rs:862-869).  One wave per leaf, one lane per target; the
// 1-D factors live in registers (order P is a template parameter), L_leaf is broadcast from LDS.
constexpr int L2P_WAVES = 4;
template <int P, int D> constexpr int l2p_waves() { return D == 3 && P > 12 ? (P > 14 ? 1 : 2) : L2P_WAVES; } // P^3 doubles of LDS per wave

// Waves per SIMD the value kernel is compiled for: with the factor rows pure multiply-adds the scheduler otherwise spreads
// the three axes over 255 registers at orders 9 and 11 (119 and 137 with the divisions in between).
template <int P, bool GRAD> constexpr int l2p_min_waves() { return GRAD ? 1 : P <= 10 ? 4 : P == 11 ? 3 : P <= 14 ? 2 : 1; }

template <int P, int D, bool GRAD>
__global__ __launch_bounds__((64 * l2p_waves<P, D>()), (l2p_min_waves<P, GRAD>())) void l2p_kernel(const DevCheb *__restrict__ chp, int n_jobs,
                                                             const int32_t *__restrict__ leaf_cells,
                                                             const int32_t *__restrict__ tgt_begin,
                                                             const int32_t *__restrict__ tgt_end,
                                                             const double *__restrict__ centers,
                                                             const double *__restrict__ lengths, Xyz tgt,
                                                             int64_t n_tgt, int K, int64_t C,
                                                             const double *__restrict__ L,
                                                             double *__restrict__ out, double *__restrict__ grad,
                                                             const int32_t *__restrict__ perm, double *__restrict__ user_out,
                                                             int64_t ldo) {
    constexpr int P1 = D > 1 ? P : 1, P2 = D > 2 ? P : 1, N = P * P1 * P2;
    constexpr int WAVES = l2p_waves<P, D>();
    __shared__ double s_L[WAVES][N];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // Values only: the table entries q[j][k] (2 T_k(node_j) / p) come through the scalar cache as SGPR operands -- staged in LDS the
    // compiler kept all P^2 of them in vector registers across the three axes (166 -> 102 VGPRs at order 7, L2P 0.98 ->
    // 0.81 ms at 10M points).  With gradients the kernel is out of registers either way and keeps the LDS copy.
    // (A matrix-pipe version like p2m_mfma_kernel -- sixteen points per v_mfma_f64_4x4x4, the coefficients as B operands
    // in registers -- was built and measured: 0.92 ms at order 7, 1.84 ms against 1.42 at order 9, ahead only with eight
    // right-hand sides (4.3 against 5.1 ms).  Not kept.)
    __shared__ double s_q_lds[GRAD ? P * P : 1];
    if constexpr (GRAD) {
        for (int i = tid; i < P * P; i += 64 * WAVES) s_q_lds[i] = chp->q[i];
        __syncthreads();
    }
    const double *__restrict__ s_q = GRAD ? s_q_lds : chp->q;
    const int job = blockIdx.x * WAVES + wave;
    if (job >= n_jobs) return; // whole wave; no block barrier below
    const int n_pad = chp->n_pad;
    const int cell = leaf_cells[job];
    const int b = tgt_begin[job], e = tgt_end[job];
    const double r = 1.0 / (lengths[cell] * 0.5); // one division per leaf, none per point
    const double cc[3] = {centers[cell * 3 + 0], centers[cell * 3 + 1], centers[cell * 3 + 2]};
    double *Lw = s_L[wave];
    for (int base = b; base < e; base += 64) {
        const int t = base + lane;
        const bool valid = t < e;
        double S0[P], S1[P1], S2[P2], D0[P], D1[P1], D2[P2];
        {
            const double x0 = valid ? (tgt.x[t] - cc[0]) * r : 0.0; // chebyshev.rs:841-845
            cheb_S_reg<P, GRAD>(x0, s_q, S0, D0);
            if (D > 1) {
                const double x1 = valid ? (tgt.y[t] - cc[1]) * r : 0.0;
                double s[P], d[P];
                cheb_S_reg<P, GRAD>(x1, s_q, s, d);
#pragma unroll
                for (int j = 0; j < P1; ++j) { S1[j] = s[j]; D1[j] = d[j]; }
            } else {
                S1[0] = 1.0;
                D1[0] = 0.0;
            }
            if (D > 2) {
                const double x2 = valid ? (tgt.z[t] - cc[2]) * r : 0.0;
                double s[P], d[P];
                cheb_S_reg<P, GRAD>(x2, s_q, s, d);
#pragma unroll
                for (int j = 0; j < P2; ++j) { S2[j] = s[j]; D2[j] = d[j]; }
            } else {
                S2[0] = 1.0;
                D2[0] = 0.0;
            }
        }
        const double gs = r; // 2 / len: the same correctly rounded quotient (len / 2 is exact)
        for (int k = 0; k < K; ++k) {
            const double *Lc = L + ((int64_t)k * C + cell) * n_pad;
            // wave-private LDS slice: in-order LDS ops of one wave need no barrier, only the wait
            for (int I = lane; I < N; I += 64) Lw[I] = Lc[I];
            __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0)
            double y = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
#pragma unroll
            for (int a = 0; a < P; ++a) {
                double ua = 0.0, uay = 0.0, uaz = 0.0;
#pragma unroll
                for (int bb = 0; bb < P1; ++bb) {
                    double t0 = 0.0, t0z = 0.0;
#pragma unroll
                    for (int c = 0; c < P2; ++c) {
                        const double lv = Lw[(a * P1 + bb) * P2 + c];
                        t0 += S2[c] * lv;
                        if (GRAD) t0z += D2[c] * lv;
                    }
                    ua += S1[bb] * t0;
                    if (GRAD) {
                        uay += D1[bb] * t0;
                        uaz += S1[bb] * t0z;
                    }
                }
                y += S0[a] * ua;
                if (GRAD) {
                    gx += D0[a] * ua;
                    gy += S0[a] * uay;
                    gz += S0[a] * uaz;
                }
            }
            if (valid) {
                // (perm: the sum goes to the caller's row of user_out instead of back to the sorted array -- the same one add.
                // Values only: the gradient kernels are out of registers as they are and take no perm.)
                if (!GRAD && perm) user_out[(int64_t)k * ldo + perm[t]] = out[(int64_t)k * n_tgt + t] + y;
                else out[(int64_t)k * n_tgt + t] += y;
                if (GRAD) {
                    grad[((int64_t)k * D + 0) * n_tgt + t] += gx * gs;
                    if (D > 1) grad[((int64_t)k * D + 1) * n_tgt + t] += gy * gs;
                    if (D > 2) grad[((int64_t)k * D + 2) * n_tgt + t] += gz * gs;
                }
            }
        }
    }
}

template <int P, int D>
static void l2p_launch_pd(const ChebRef &ch, int n_jobs, const int32_t *leaf_cells, const int32_t *tgt_begin,
                          const int32_t *tgt_end, const double *centers, const double *lengths, Xyz tgt,
                          int64_t n_tgt, int K, int64_t C, const double *L, double *out_sorted, double *grad_sorted,
                          hipStream_t s, const int32_t *perm, double *user_out, int64_t ldo) {
    constexpr int WAVES = l2p_waves<P, D>();
    const int blocks = (n_jobs + WAVES - 1) / WAVES;
    if (grad_sorted)
        hipLaunchKernelGGL((l2p_kernel<P, D, true>), dim3(blocks), dim3(64 * WAVES), 0, s, ch.dev, n_jobs,
                           leaf_cells, tgt_begin, tgt_end, centers, lengths, tgt, n_tgt, K, C, L, out_sorted,
                           grad_sorted, perm, user_out, ldo);
    else
        hipLaunchKernelGGL((l2p_kernel<P, D, false>), dim3(blocks), dim3(64 * WAVES), 0, s, ch.dev, n_jobs,
                           leaf_cells, tgt_begin, tgt_end, centers, lengths, tgt, n_tgt, K, C, L, out_sorted,
                           grad_sorted, perm, user_out, ldo);
}

template <int P>
static void l2p_launch_p(const ChebRef &ch, int n_jobs, const int32_t *leaf_cells, const int32_t *tgt_begin,
                         const int32_t *tgt_end, const double *centers, const double *lengths, Xyz tgt, int64_t n_tgt,
                         int K, int64_t C, const double *L, double *out_sorted, double *grad_sorted, hipStream_t s,
                         const int32_t *perm, double *user_out, int64_t ldo) {
    if (ch.d == 3) {
        l2p_launch_pd<P, 3>(ch, n_jobs, leaf_cells, tgt_begin, tgt_end, centers, lengths, tgt, n_tgt, K, C, L, out_sorted, grad_sorted, s, perm, user_out, ldo);
    } else if (ch.d == 2) {
        l2p_launch_pd<P, 2>(ch, n_jobs, leaf_cells, tgt_begin, tgt_end, centers, lengths, tgt, n_tgt, K, C, L, out_sorted, grad_sorted, s, perm, user_out, ldo);
    } else {
        l2p_launch_pd<P, 1>(ch, n_jobs, leaf_cells, tgt_begin, tgt_end, centers, lengths, tgt, n_tgt, K, C, L, out_sorted, grad_sorted, s, perm, user_out, ldo);
    }
}

bool l2p_order_supported(int p, int d) { return p >= 2 && p <= kMaxOrder && d >= 1 && d <= 3; }

// ------------------------------------------------------------------ L2P over runs of leaves
// The one-leaf kernel above gives a wave one leaf: with 38 targets in a leaf, 59 % of the lanes are live in the factor rows
// and in the contraction.  Here a workgroup takes a run of up to kL2pRunLeaves consecutive jobs whose target ranges abut
// (at most kL2pRunTargets targets in all, FmmTree::build_l2p_runs) and a lane takes one target of the run, whichever leaf
// it lies in: the run's L rows go to LDS, one slice per leaf, the lane finds its leaf from the run's boundaries and reads
// that leaf's centre, 1 / half-length and slice.  The sums of a target are those of the one-leaf kernel, term by term.
// Slices are S = N | 1 doubles apart: in a 64-lane batch the lanes of a leaf read one address (a broadcast) and the two or
// three leaves that meet in the batch read the same index of neighbouring slices, S and 2 S doubles apart -- with S odd
// these lie in different banks (8-byte reads: bank pair (address / 8) mod 32, and i S mod 32 differs for all i < 32).
template <int P, int D> constexpr bool l2p_runs_fit() { return (D == 1 ? P : D == 2 ? P * P : P * P * P) <= kL2pRunMaxNodes; }

template <int P, int D>
__global__ __launch_bounds__(kL2pRunTargets, 4) void l2p_runs_kernel(const DevCheb *__restrict__ chp, const int32_t *__restrict__ runs,
                                                                 const int32_t *__restrict__ leaf_cells,
                                                                 const int32_t *__restrict__ tgt_begin,
                                                                 const int32_t *__restrict__ tgt_end,
                                                                 const double *__restrict__ centers,
                                                                 const double *__restrict__ lengths, Xyz tgt, int64_t n_tgt, int K,
                                                                 int64_t C, const double *__restrict__ L, double *__restrict__ out,
                                                                 const int32_t *__restrict__ perm, double *__restrict__ user_out,
                                                                 int64_t ldo) {
    constexpr int P1 = D > 1 ? P : 1, P2 = D > 2 ? P : 1, N = P * P1 * P2, S = N | 1;
    __shared__ double s_L[kL2pRunLeaves * S];
    __shared__ double s_geo[kL2pRunLeaves][4]; // centre, 1 / half-length
    __shared__ int32_t s_bnd[kL2pRunLeaves + 1], s_cell[kL2pRunLeaves];
    const int tid = threadIdx.x;
    const double *__restrict__ s_q = chp->q; // through the scalar cache, as in l2p_kernel
    const int first = runs[2 * blockIdx.x], n = min(runs[2 * blockIdx.x + 1], kL2pRunLeaves);
    const int n_pad = chp->n_pad;
    if (n < 1) return; // whole workgroup
    if (tid < n) {
        const int job = first + tid, cell = leaf_cells[job];
        s_cell[tid] = cell;
        s_bnd[tid] = tgt_begin[job];
        if (tid == n - 1) s_bnd[n] = tgt_end[job];
        s_geo[tid][0] = centers[cell * 3 + 0];
        s_geo[tid][1] = centers[cell * 3 + 1];
        s_geo[tid][2] = centers[cell * 3 + 2];
        s_geo[tid][3] = 1.0 / (lengths[cell] * 0.5);
    }
    __syncthreads();
    const int t = s_bnd[0] + tid;
    const bool valid = t < s_bnd[n]; // (a run holds at most kL2pRunTargets targets: one per thread)
    int leaf = 0;
#pragma unroll
    for (int i = 1; i < kL2pRunLeaves; ++i) leaf += (i < n && t >= s_bnd[i]) ? 1 : 0;
    double S0[P], S1[P1], S2[P2];
    {
        const double r = s_geo[leaf][3];
        double dummy[P];
        const double x0 = valid ? (tgt.x[t] - s_geo[leaf][0]) * r : 0.0;
        cheb_S_reg<P, false>(x0, s_q, S0, dummy);
        if (D > 1) {
            const double x1 = valid ? (tgt.y[t] - s_geo[leaf][1]) * r : 0.0;
            double s[P];
            cheb_S_reg<P, false>(x1, s_q, s, dummy);
#pragma unroll
            for (int j = 0; j < P1; ++j) S1[j] = s[j];
        } else {
            S1[0] = 1.0;
        }
        if (D > 2) {
            const double x2 = valid ? (tgt.z[t] - s_geo[leaf][2]) * r : 0.0;
            double s[P];
            cheb_S_reg<P, false>(x2, s_q, s, dummy);
#pragma unroll
            for (int j = 0; j < P2; ++j) S2[j] = s[j];
        } else {
            S2[0] = 1.0;
        }
    }
    const double *Lw = s_L + leaf * S;
    for (int k = 0; k < K; ++k) {
        if (k) __syncthreads(); // the slices of the right-hand side before are read
        for (int idx = tid; idx < n * N; idx += kL2pRunTargets) {
            const int i = idx / N, I = idx - i * N;
            s_L[i * S + I] = L[((int64_t)k * C + s_cell[i]) * n_pad + I];
        }
        __syncthreads();
        double y = 0.0;
#pragma unroll
        for (int a = 0; a < P; ++a) {
            double ua = 0.0;
#pragma unroll
            for (int bb = 0; bb < P1; ++bb) {
                double t0 = 0.0;
#pragma unroll
                for (int c = 0; c < P2; ++c) t0 += S2[c] * Lw[(a * P1 + bb) * P2 + c];
                ua += S1[bb] * t0;
            }
            y += S0[a] * ua;
        }
        if (valid) {
            if (perm) user_out[(int64_t)k * ldo + perm[t]] = out[(int64_t)k * n_tgt + t] + y;
            else out[(int64_t)k * n_tgt + t] += y;
        }
    }
}

bool l2p_runs_supported(int p, int d) {
    if (!l2p_order_supported(p, d)) return false;
    int n = 1;
    for (int a = 0; a < d; ++a) n *= p;
    return n <= kL2pRunMaxNodes;
}

template <int P, int D>
static void l2p_runs_launch_pd(const ChebRef &ch, const L2pRuns &r, const int32_t *leaf_cells, const int32_t *tgt_begin,
                               const int32_t *tgt_end, const double *centers, const double *lengths, Xyz tgt, int64_t n_tgt, int K,
                               int64_t C, const double *L, double *out_sorted, hipStream_t s, const int32_t *perm, double *user_out,
                               int64_t ldo) {
    if constexpr (l2p_runs_fit<P, D>())
        hipLaunchKernelGGL((l2p_runs_kernel<P, D>), dim3(r.n_runs), dim3(kL2pRunTargets), 0, s, ch.dev, r.runs, leaf_cells, tgt_begin,
                           tgt_end, centers, lengths, tgt, n_tgt, K, C, L, out_sorted, perm, user_out, ldo);
}

void launch_l2p(const ChebRef &ch, int n_jobs, const int32_t *leaf_cells, const int32_t *tgt_begin,
                const int32_t *tgt_end, const double *centers, const double *lengths, const double *const *tgt_xyz,
                int64_t n_tgt, int K, int64_t C, const double *L, double *out_sorted, double *grad_sorted,
                hipStream_t s, const int32_t *perm, double *user_out, int64_t ldo, const L2pRuns *runs) {
    if (n_jobs == 0) return;
    if (perm && grad_sorted) return; // (no caller asks for both; the gradient kernels ignore perm)
    const Xyz tgt = make_xyz(tgt_xyz);
    if (runs && runs->n_runs > 0 && !grad_sorted && l2p_runs_supported(ch.p, ch.d)) {
        // the runs (indices into the whole job list), then the jobs outside them, one leaf each
        dispatch_order<2, 16>(ch.p, [&](auto pc) {
            constexpr int P = decltype(pc)::value;
            if (ch.d == 3) l2p_runs_launch_pd<P, 3>(ch, *runs, leaf_cells, tgt_begin, tgt_end, centers, lengths, tgt, n_tgt, K, C, L, out_sorted, s, perm, user_out, ldo);
            else if (ch.d == 2) l2p_runs_launch_pd<P, 2>(ch, *runs, leaf_cells, tgt_begin, tgt_end, centers, lengths, tgt, n_tgt, K, C, L, out_sorted, s, perm, user_out, ldo);
            else l2p_runs_launch_pd<P, 1>(ch, *runs, leaf_cells, tgt_begin, tgt_end, centers, lengths, tgt, n_tgt, K, C, L, out_sorted, s, perm, user_out, ldo);
        });
        n_jobs = runs->n_rest;
        leaf_cells = runs->rest_cell;
        tgt_begin = runs->rest_begin;
        tgt_end = runs->rest_end;
        if (n_jobs == 0) return;
    }
    dispatch_order<2, 16>(ch.p, [&](auto pc) {
        l2p_launch_p<decltype(pc)::value>(ch, n_jobs, leaf_cells, tgt_begin, tgt_end, centers, lengths, tgt, n_tgt, K, C, L,
                                          out_sorted, grad_sorted, s, perm, user_out, ldo);
    });
}

} // namespace bbfmm
