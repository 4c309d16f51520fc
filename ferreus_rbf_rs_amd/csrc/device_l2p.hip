// L2P: the local expansion of a leaf evaluated at its targets, with its launcher.
#include "device_common.hpp"

namespace bbfmm {

// ------------------------------------------------------------------ L2P
// local_to_particle (bbfmm.rs:1358-1440): y[t] += S(x_t) . L_leaf, optionally gradients
// (dS scaled by 2/length, chebyshev.rs:862-869).  One wave per leaf, one lane per target; the
// 1-D factors live in registers (order P is a template parameter), L_leaf is broadcast from LDS.
constexpr int L2P_WAVES = 4;
template <int P, int D> constexpr int l2p_waves() { return D == 3 && P > 12 ? (P > 14 ? 1 : 2) : L2P_WAVES; } // P^3 doubles of LDS per wave

template <int P, int D, bool GRAD>
__global__ __launch_bounds__((64 * l2p_waves<P, D>())) void l2p_kernel(const DevCheb *__restrict__ chp, int n_jobs,
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
    // Values only: the node values T_k(node_j) come through the scalar cache as SGPR operands -- staged in LDS the
    // compiler kept all P^2 of them in vector registers across the three axes (166 -> 102 VGPRs at order 7, L2P 0.98 ->
    // 0.81 ms at 10M points).  With gradients the kernel is out of registers either way and keeps the LDS copy.
    // (A matrix-pipe version like p2m_mfma_kernel -- sixteen points per v_mfma_f64_4x4x4, the coefficients as B operands
    // in registers -- was built and measured: 0.92 ms at order 7, 1.84 ms against 1.42 at order 9, ahead only with eight
    // right-hand sides (4.3 against 5.1 ms).  Not kept.)
    __shared__ double s_polyn_lds[GRAD ? P * P : 1];
    if constexpr (GRAD) {
        for (int i = tid; i < P * P; i += 64 * WAVES) s_polyn_lds[i] = chp->polyn[i];
        __syncthreads();
    }
    const double *__restrict__ s_polyn = GRAD ? s_polyn_lds : chp->polyn;
    const int job = blockIdx.x * WAVES + wave;
    if (job >= n_jobs) return; // whole wave; no block barrier below
    const int n_pad = chp->n_pad;
    const int cell = leaf_cells[job];
    const int b = tgt_begin[job], e = tgt_end[job];
    const double len = lengths[cell];
    const double cc[3] = {centers[cell * 3 + 0], centers[cell * 3 + 1], centers[cell * 3 + 2]};
    double *Lw = s_L[wave];
    for (int base = b; base < e; base += 64) {
        const int t = base + lane;
        const bool valid = t < e;
        double S0[P], S1[P1], S2[P2], D0[P], D1[P1], D2[P2];
        {
            const double x0 = valid ? (tgt.x[t] - cc[0]) / (len * 0.5) : 0.0; // chebyshev.rs:841-845
            cheb_S_reg<P, GRAD>(x0, s_polyn, S0, D0);
            if (D > 1) {
                const double x1 = valid ? (tgt.y[t] - cc[1]) / (len * 0.5) : 0.0;
                double s[P], d[P];
                cheb_S_reg<P, GRAD>(x1, s_polyn, s, d);
#pragma unroll
                for (int j = 0; j < P1; ++j) { S1[j] = s[j]; D1[j] = d[j]; }
            } else {
                S1[0] = 1.0;
                D1[0] = 0.0;
            }
            if (D > 2) {
                const double x2 = valid ? (tgt.z[t] - cc[2]) / (len * 0.5) : 0.0;
                double s[P], d[P];
                cheb_S_reg<P, GRAD>(x2, s_polyn, s, d);
#pragma unroll
                for (int j = 0; j < P2; ++j) { S2[j] = s[j]; D2[j] = d[j]; }
            } else {
                S2[0] = 1.0;
                D2[0] = 0.0;
            }
        }
        const double gs = 2.0 / len;
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

void launch_l2p(const ChebRef &ch, int n_jobs, const int32_t *leaf_cells, const int32_t *tgt_begin,
                const int32_t *tgt_end, const double *centers, const double *lengths, const double *const *tgt_xyz,
                int64_t n_tgt, int K, int64_t C, const double *L, double *out_sorted, double *grad_sorted,
                hipStream_t s, const int32_t *perm, double *user_out, int64_t ldo) {
    if (n_jobs == 0) return;
    if (perm && grad_sorted) return; // (no caller asks for both; the gradient kernels ignore perm)
    const Xyz tgt = make_xyz(tgt_xyz);
    dispatch_order<2, 16>(ch.p, [&](auto pc) {
        l2p_launch_p<decltype(pc)::value>(ch, n_jobs, leaf_cells, tgt_begin, tgt_end, centers, lengths, tgt, n_tgt, K, C, L,
                                          out_sorted, grad_sorted, s, perm, user_out, ldo);
    });
}

} // namespace bbfmm
