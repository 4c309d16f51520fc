// P2M: particles to the multipole coefficients of their leaf, vector- and matrix-pipe kernels with their launcher.
#include "device_common.hpp"

namespace bbfmm {

// ------------------------------------------------------------------ P2M
// particle_to_multipole (bbfmm.rs:691-739): M_c[:, k] += S(x_leaf)^T w_leaf[:, k].
// One wave per leaf.  Points are taken 32 at a time: lanes compute the three 1-D factor rows
// of their point (registers, order P is a template parameter) and park them in a wave-private
// LDS slice; then lane q owns the node pairs (i1, i2) = q and keeps the P sums over i0 in
// registers, so a point costs two private LDS reads plus P broadcast reads per lane.
constexpr int P2M_WAVES = 4;
// 3-D orders above 12 (they work, slowly: bbfmm.rs:77-104 takes any order): two waves per workgroup
template <int P, int D> constexpr int p2m_waves() { return D == 3 && P > 12 ? 2 : P2M_WAVES; }
constexpr int P2M_PTS = 64; // measured at 10M points, K = 1: 1.12 ms against 1.38 ms with 32
                            // (one batch covers a 38-point leaf) and 1.55 ms with two rhs slots

template <int P, int D, int P2M_KB>
__global__ __launch_bounds__((64 * p2m_waves<P, D>())) void p2m_kernel(const DevCheb *__restrict__ chp, int n_leaves, Xyz src,
                                                             const double *__restrict__ ws, int64_t N, int K,
                                                             int64_t C, const int32_t *__restrict__ leaf_cells,
                                                             const int32_t *__restrict__ pt_begin,
                                                             const int32_t *__restrict__ pt_end,
                                                             const double *__restrict__ centers,
                                                             const double *__restrict__ lengths,
                                                             double *__restrict__ M) {
    constexpr int P1 = D > 1 ? P : 1, P2 = D > 2 ? P : 1, NPAIR = P1 * P2;
    constexpr int NPASS = (NPAIR + 63) / 64;
    constexpr int SROW = 3 * P + P2M_KB; // per point: S0[P], S1[P], S2[P], w[KB]
    __shared__ double s_q[P * P];
    constexpr int WAVES = p2m_waves<P, D>();
    __shared__ double s_pts[WAVES][P2M_PTS][SROW];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < P * P; i += 64 * WAVES) s_q[i] = chp->q[i];
    __syncthreads();
    const int job = blockIdx.x * WAVES + wave;
    if (job >= n_leaves) return; // whole wave; no block barrier below
    const int n_pad = chp->n_pad;
    const int cell = leaf_cells[job];
    const int b = pt_begin[cell], e = pt_end[cell];
    const double r = 1.0 / (lengths[cell] * 0.5); // one division per leaf, none per point
    const double cc[3] = {centers[cell * 3 + 0], centers[cell * 3 + 1], centers[cell * 3 + 2]};
    double(*sp)[SROW] = s_pts[wave];
    for (int k0 = 0; k0 < K; k0 += P2M_KB) {
        double acc[NPASS][P2M_KB][P];
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
            for (int kk = 0; kk < P2M_KB; ++kk)
#pragma unroll
                for (int i0 = 0; i0 < P; ++i0) acc[ps][kk][i0] = 0.0;
        for (int base = b; base < e; base += P2M_PTS) {
            const int npts = min(P2M_PTS, e - base);
            if (lane < npts) {
                const int pt = base + lane;
                double S[P], dS[P];
                cheb_S_reg<P, false>((src.x[pt] - cc[0]) * r, s_q, S, dS); // chebyshev.rs:841-845
#pragma unroll
                for (int jx = 0; jx < P; ++jx) sp[lane][jx] = S[jx];
                if (D > 1) {
                    cheb_S_reg<P, false>((src.y[pt] - cc[1]) * r, s_q, S, dS);
#pragma unroll
                    for (int jx = 0; jx < P; ++jx) sp[lane][P + jx] = S[jx];
                } else {
                    sp[lane][P] = 1.0;
                }
                if (D > 2) {
                    cheb_S_reg<P, false>((src.z[pt] - cc[2]) * r, s_q, S, dS);
#pragma unroll
                    for (int jx = 0; jx < P; ++jx) sp[lane][2 * P + jx] = S[jx];
                } else {
                    sp[lane][2 * P] = 1.0;
                }
#pragma unroll
                for (int kk = 0; kk < P2M_KB; ++kk)
                    sp[lane][3 * P + kk] = (k0 + kk < K) ? ws[(int64_t)(k0 + kk) * N + pt] : 0.0;
            }
            __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0): wave-private slice, in-order LDS
#pragma unroll
            for (int ps = 0; ps < NPASS; ++ps) {
                const int q = lane + 64 * ps;
                if (q < NPAIR) {
                    const int i1 = q / P2, i2 = q - i1 * P2;
                    for (int pt = 0; pt < npts; ++pt) {
                        const double *row = sp[pt];
                        const double s12 = row[P + i1] * row[2 * P + i2];
#pragma unroll
                        for (int kk = 0; kk < P2M_KB; ++kk) {
                            const double v = s12 * row[3 * P + kk];
#pragma unroll
                            for (int i0 = 0; i0 < P; ++i0) acc[ps][kk][i0] += v * row[i0];
                        }
                    }
                }
            }
            __builtin_amdgcn_s_waitcnt(0xc07f); // reads done before the slice is rewritten
        }
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int q = lane + 64 * ps;
            if (q < NPAIR) {
#pragma unroll
                for (int kk = 0; kk < P2M_KB; ++kk) {
                    if (k0 + kk < K) {
                        double *Mc = M + ((int64_t)(k0 + kk) * C + cell) * n_pad + q;
#pragma unroll
                        for (int i0 = 0; i0 < P; ++i0) Mc[i0 * NPAIR] = acc[ps][kk][i0]; // a leaf is written once
                    }
                }
            }
        }
    }
}

// P2M as a small matrix product on the FP64 matrix pipe (round 4; 3-D, orders up to 10).  Per leaf
//   M[i0][q] = sum_p (S0[p][i0] w_p) * (S1[p][i1(q)] S2[p][i2(q)]),   q = i1 * P + i2
// is (P x npts) x (npts x P^2).  The kernel above evaluates it with lane = q and one point at a time: two private and
// four broadcast LDS reads for nine multiply-adds per point and lane, which keeps the CU's one LDS pipe busy for four
// waves' worth of arithmetic (VALUBusy 46 %).  Here four points form the contraction of a v_mfma_f64_4x4x4 (four
// independent 4 x 4 x 4 products per instruction, lanes A: 16 k + 4 b + i, B: 16 k + 4 b + j, D: 16 i + 4 b + j):
// row block rb holds i0 = 4 rb + i, column group g holds q = 16 g + 4 b + j; per step of four points a lane reads one
// S0 value per row block and an S1 / S2 pair per column group (private LDS reads, no broadcasts) and issues RB x G
// matrix instructions.  Points beyond the leaf are zero rows.  Same sums as the kernel above in another order.
template <int P>
__global__ __launch_bounds__(64 * P2M_WAVES) void p2m_mfma_kernel(const DevCheb *__restrict__ chp, int n_leaves, Xyz src,
                                                                 const double *__restrict__ ws, int64_t N, int K, int64_t C,
                                                                 const int32_t *__restrict__ leaf_cells,
                                                                 const int32_t *__restrict__ pt_begin,
                                                                 const int32_t *__restrict__ pt_end,
                                                                 const double *__restrict__ centers,
                                                                 const double *__restrict__ lengths, double *__restrict__ M) {
    constexpr int NPAIR = P * P, RB = (P + 3) / 4, G = (NPAIR + 15) / 16;
    constexpr int SROW = 3 * P + 2; // per point: S0[P], S1[P], S2[P], w, one spare (rows start 16-byte aligned for even P)
    __shared__ double s_pts[P2M_WAVES][64][SROW];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // (the table entries q[j][k] (2 T_k(node_j) / p) come through the scalar cache as SGPR operands: the same 8 P^2 bytes for every wave;
    // staged in LDS the compiler kept all P^2 of them in vector registers across the three axes)
    const double *__restrict__ s_q = chp->q;
    const int job = blockIdx.x * P2M_WAVES + wave;
    if (job >= n_leaves) return; // whole wave; no block barrier below
    const int n_pad = chp->n_pad;
    const int cell = leaf_cells[job];
    const int b = pt_begin[cell], e = pt_end[cell];
    const double r = 1.0 / (lengths[cell] * 0.5); // one division per leaf, none per point
    const double cc[3] = {centers[cell * 3 + 0], centers[cell * 3 + 1], centers[cell * 3 + 2]};
    double(*sp)[SROW] = s_pts[wave];
    const int hi = lane >> 4, blk = (lane >> 2) & 3, lo = lane & 3;
    // this lane's column of every group (clamped: columns past P^2 read valid memory and are never stored)
    int o1[G], o2[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int q = min(16 * g + 4 * blk + lo, NPAIR - 1);
        o1[g] = P + q / P;
        o2[g] = 2 * P + q % P;
    }
    for (int k = 0; k < K; ++k) {
        double acc[RB][G];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int g = 0; g < G; ++g) acc[rb][g] = 0.0;
        for (int base = b; base < e; base += 64) {
            const int npts = min(64, e - base);
            if (k == 0 || e - b > 64) { // the factor rows of the batch (kept across right-hand sides when the leaf is one batch)
                double S[P], dS[P];
                const int pt = base + min(lane, npts - 1);
                const bool live = lane < npts;
                cheb_S_reg<P, false>((src.x[pt] - cc[0]) * r, s_q, S, dS); // chebyshev.rs:841-845
#pragma unroll
                for (int jx = 0; jx < P; ++jx) sp[lane][jx] = live ? S[jx] : 0.0;
                cheb_S_reg<P, false>((src.y[pt] - cc[1]) * r, s_q, S, dS);
#pragma unroll
                for (int jx = 0; jx < P; ++jx) sp[lane][P + jx] = live ? S[jx] : 0.0;
                cheb_S_reg<P, false>((src.z[pt] - cc[2]) * r, s_q, S, dS);
#pragma unroll
                for (int jx = 0; jx < P; ++jx) sp[lane][2 * P + jx] = live ? S[jx] : 0.0;
            }
            sp[lane][3 * P] = lane < npts ? ws[(int64_t)k * N + base + lane] : 0.0;
            __builtin_amdgcn_s_waitcnt(0xc07f); // lgkmcnt(0): wave-private slice, in-order LDS
            const int nsteps = (npts + 3) >> 2;
            for (int st = 0; st < nsteps; ++st) {
                const double *row = sp[4 * st + hi];
                const double wv = row[3 * P];
                double av[RB], bv[G];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) av[rb] = 4 * rb + lo < P ? row[4 * rb + lo] * wv : 0.0;
#pragma unroll
                for (int g = 0; g < G; ++g) bv[g] = row[o1[g]] * row[o2[g]];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int g = 0; g < G; ++g) acc[rb][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(av[rb], bv[g], acc[rb][g], 0, 0, 0);
            }
            __builtin_amdgcn_s_waitcnt(0xc07f); // reads done before the slice is rewritten
        }
        double *Mc = M + ((int64_t)k * C + cell) * n_pad;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const int i0 = 4 * rb + hi; // D: lane = 16 i + 4 b + j
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int q = 16 * g + 4 * blk + lo;
                if (i0 < P && q < NPAIR) Mc[i0 * NPAIR + q] = acc[rb][g]; // a leaf is written once
            }
        }
    }
}

template <int P, int D>
static void p2m_launch_pd(const ChebRef &ch, Xyz src, const double *w_sorted, int64_t N, int K, int64_t C,
                          const int32_t *leaf_cells, int n_leaves, const int32_t *pt_begin, const int32_t *pt_end,
                          const double *centers, const double *lengths, double *M, hipStream_t s) {
    constexpr int WAVES = p2m_waves<P, D>();
    const int blocks = (n_leaves + WAVES - 1) / WAVES;
    if constexpr (D == 3 && P >= 4 && P <= 10) { // the matrix-pipe version
        hipLaunchKernelGGL((p2m_mfma_kernel<P>), dim3((n_leaves + P2M_WAVES - 1) / P2M_WAVES), dim3(64 * P2M_WAVES), 0, s, ch.dev,
                           n_leaves, src, w_sorted, N, K, C, leaf_cells, pt_begin, pt_end, centers, lengths, M);
        return;
    }
    if (K == 1 || (D == 3 && P > 12)) // (two rhs slots at orders above 12 would spill: one rhs per pass there)
        hipLaunchKernelGGL((p2m_kernel<P, D, 1>), dim3(blocks), dim3(64 * WAVES), 0, s, ch.dev, n_leaves, src,
                           w_sorted, N, K, C, leaf_cells, pt_begin, pt_end, centers, lengths, M);
    else
        hipLaunchKernelGGL((p2m_kernel<P, D, 2>), dim3(blocks), dim3(64 * WAVES), 0, s, ch.dev, n_leaves, src,
                           w_sorted, N, K, C, leaf_cells, pt_begin, pt_end, centers, lengths, M);
}

void launch_p2m(const ChebRef &ch, const double *const *src_xyz, const double *w_sorted, int64_t N, int K, int64_t C,
                const int32_t *leaf_cells, int n_leaves, const int32_t *pt_begin, const int32_t *pt_end,
                const double *centers, const double *lengths, double *M, hipStream_t s) {
    if (n_leaves == 0) return;
    const Xyz src = make_xyz(src_xyz);
    dispatch_order<2, 16>(ch.p, [&](auto pc) {
        constexpr int P = decltype(pc)::value;
        if (ch.d == 3) p2m_launch_pd<P, 3>(ch, src, w_sorted, N, K, C, leaf_cells, n_leaves, pt_begin, pt_end, centers, lengths, M, s);
        else if (ch.d == 2) p2m_launch_pd<P, 2>(ch, src, w_sorted, N, K, C, leaf_cells, n_leaves, pt_begin, pt_end, centers, lengths, M, s);
        else p2m_launch_pd<P, 1>(ch, src, w_sorted, N, K, C, leaf_cells, n_leaves, pt_begin, pt_end, centers, lengths, M, s);
    });
}

} // namespace bbfmm
