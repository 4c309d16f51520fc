// M2M / L2L: the transfers between a cell and its children, general and 3-D register kernels with their launchers.
#include "device_common.hpp"
#include "m2l_basis_rows.hpp"

namespace bbfmm {

// ------------------------------------------------------------------ M2M / L2L
// One pass of a sum-factorised transfer along `axis`.  in/out are n-vectors in LDS with
// index (i0*P1 + i1)*P2 + i2.  FORWARD (M2M): out[.., i, ..] = sum_a xf[a][i] in[.., a, ..];
// transposed (L2L): out[.., a, ..] = sum_i xf[a][i] in[.., i, ..].  xf = xfer[side] (p x p).
template <bool FORWARD>
__device__ inline void transfer_pass(const double *in, double *out, const double *xf, int axis, int p, int P0, int P1,
                                     int P2, int n, int tid, int nthreads) {
    const int stride = axis == 0 ? P1 * P2 : (axis == 1 ? P2 : 1);
    for (int I = tid; I < n; I += nthreads) {
        const int ia = (I / stride) % p;
        const int base = I - ia * stride;
        double s = 0.0;
        for (int a = 0; a < p; ++a) {
            const double f = FORWARD ? xf[a * p + ia] : xf[ia * p + a];
            s += f * in[base + a * stride];
        }
        out[I] = s;
    }
}

// multipole_to_multipole (bbfmm.rs:742-772): one workgroup per parent.
__global__ __launch_bounds__(256) void m2m_kernel(const DevCheb *__restrict__ chp, int K, int64_t C,
                                                  const int32_t *__restrict__ parents,
                                                  const int64_t *__restrict__ child_ptr,
                                                  const int32_t *__restrict__ child_idx,
                                                  const int32_t *__restrict__ octant, double *__restrict__ M) {
    extern __shared__ double lds[];
    const int p = chp->p, d = chp->d, n = chp->n, n_pad = chp->n_pad;
    int P0, P1, P2;
    axis_sizes(p, d, P0, P1, P2);
    double *bufA = lds, *bufB = lds + n, *acc = lds + 2 * n, *xf = lds + 3 * n;
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * p * p; i += 256) xf[i] = chp->xfer[i];
    const int P = parents[blockIdx.x];
    const int64_t c0 = child_ptr[P], c1 = child_ptr[P + 1];
    for (int k = 0; k < K; ++k) {
        for (int I = tid; I < n; I += 256) acc[I] = 0.0;
        for (int64_t q = c0; q < c1; ++q) {
            const int ch = child_idx[q];
            const int oct = octant[ch];
            const double *Mc = M + ((int64_t)k * C + ch) * n_pad;
            __syncthreads();
            for (int I = tid; I < n; I += 256) bufA[I] = Mc[I];
            __syncthreads();
            double *in = bufA, *out = bufB;
            for (int axis = d - 1; axis >= 0; --axis) {
                const double *x1 = xf + ((oct >> axis) & 1) * p * p; // chebyshev.rs:183-192: bit a <-> axis a
                transfer_pass<true>(in, out, x1, axis, p, P0, P1, P2, n, tid, 256);
                __syncthreads();
                double *t = in;
                in = out;
                out = t;
            }
            for (int I = tid; I < n; I += 256) acc[I] += in[I];
        }
        __syncthreads();
        double *Mp = M + ((int64_t)k * C + P) * n_pad;
        for (int I = tid; I < n; I += 256) Mp[I] = acc[I]; // a parent is written once
        __syncthreads();
    }
}

// local_to_local (bbfmm.rs:1051-1086): one workgroup per child cell.
__global__ __launch_bounds__(256) void l2l_kernel(const DevCheb *__restrict__ chp, int K, int64_t C,
                                                  const int32_t *__restrict__ cells,
                                                  const int32_t *__restrict__ parent,
                                                  const int32_t *__restrict__ octant,
                                                  const uint8_t *__restrict__ active, double *__restrict__ L) {
    extern __shared__ double lds[];
    const int p = chp->p, d = chp->d, n = chp->n, n_pad = chp->n_pad;
    int P0, P1, P2;
    axis_sizes(p, d, P0, P1, P2);
    double *bufA = lds, *bufB = lds + n, *xf = lds + 2 * n;
    const int tid = threadIdx.x;
    const int c = cells[blockIdx.x];
    if (active && !active[c]) return;
    const int P = parent[c];
    if (P < 0) return;
    for (int i = tid; i < 2 * p * p; i += 256) xf[i] = chp->xfer[i];
    const int oct = octant[c];
    for (int k = 0; k < K; ++k) {
        const double *Lp = L + ((int64_t)k * C + P) * n_pad;
        __syncthreads();
        for (int I = tid; I < n; I += 256) bufA[I] = Lp[I];
        __syncthreads();
        double *in = bufA, *out = bufB;
        for (int axis = 0; axis < d; ++axis) {
            const double *x1 = xf + ((oct >> axis) & 1) * p * p;
            transfer_pass<false>(in, out, x1, axis, p, P0, P1, P2, n, tid, 256);
            __syncthreads();
            double *t = in;
            in = out;
            out = t;
        }
        double *Lc = L + ((int64_t)k * C + c) * n_pad;
        for (int I = tid; I < n; I += 256) Lc[I] += in[I];
    }
}

// ------------------------------------------------------------------ M2M / L2L, 3-D fast path
// One wave per cell, order P a template parameter.  A lane owns "pencils" of P entries along one
// axis in registers, so a 1-D transfer is P*P register FMAs against a wave-uniform P x P block
// (scalar loads); between the axes the vector is transposed through a wave-private LDS slice (no
// workgroup barrier).  Layout of a vector: index (i0*P + i1)*P + i2.
template <int P, bool FORWARD>
__device__ inline void pencil_apply(double (&v)[P], const double *__restrict__ xf) {
    double o[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) s += (FORWARD ? xf[k * P + j] : xf[j * P + k]) * v[k];
        o[j] = s;
    }
#pragma unroll
    for (int j = 0; j < P; ++j) v[j] = o[j];
}

// in: global vector of the source cell; buf: wave-private LDS (P^3 doubles); on return buf holds
// the transferred vector.  oct: octant of the child (bit a <-> axis a, chebyshev.rs:183-192).
// (always inline: each kernel instance has its own copy with the P x P blocks in scalar registers -- with two kernel
// instances per order calling it the compiler otherwise leaves it out of line from order 8 up, at twice the time)
template <int P, bool FORWARD>
__device__ __forceinline__ void transfer3_wave(const double *__restrict__ in, double *buf, const double *__restrict__ xfer,
                                      int oct, int lane) {
    constexpr int PP = P * P, NPEN = (PP + 63) / 64;
    const double *x0 = xfer + ((oct >> 0) & 1) * PP, *x1 = xfer + ((oct >> 1) & 1) * PP,
                 *x2 = xfer + ((oct >> 2) & 1) * PP;
    // axis 0: pencil q = (i1, i2), entries at i0 * PP + q (coalesced global reads)
#pragma unroll
    for (int ps = 0; ps < NPEN; ++ps) {
        const int q = lane + 64 * ps;
        if (q < PP) {
            double v[P];
#pragma unroll
            for (int i = 0; i < P; ++i) v[i] = in[i * PP + q];
            pencil_apply<P, FORWARD>(v, x0);
#pragma unroll
            for (int i = 0; i < P; ++i) buf[i * PP + q] = v[i];
        }
    }
    __builtin_amdgcn_wave_barrier();
    // axis 1: pencil r = (i0, i2), entries at i0 * PP + i1 * P + i2
#pragma unroll
    for (int ps = 0; ps < NPEN; ++ps) {
        const int r = lane + 64 * ps;
        if (r < PP) {
            const int i0 = r / P, i2 = r - i0 * P;
            double v[P];
#pragma unroll
            for (int i = 0; i < P; ++i) v[i] = buf[i0 * PP + i * P + i2];
            pencil_apply<P, FORWARD>(v, x1);
#pragma unroll
            for (int i = 0; i < P; ++i) buf[i0 * PP + i * P + i2] = v[i];
        }
    }
    __builtin_amdgcn_wave_barrier();
    // axis 2: pencil s = (i0, i1), entries at s * P + i2
#pragma unroll
    for (int ps = 0; ps < NPEN; ++ps) {
        const int sidx = lane + 64 * ps;
        if (sidx < PP) {
            double v[P];
#pragma unroll
            for (int i = 0; i < P; ++i) v[i] = buf[sidx * P + i];
            pencil_apply<P, FORWARD>(v, x2);
#pragma unroll
            for (int i = 0; i < P; ++i) buf[sidx * P + i] = v[i];
        }
    }
    __builtin_amdgcn_wave_barrier();
}

constexpr int XFER_WAVES = 4;

// local_to_local, one wave per child cell: L_child += T_child^T L_parent (bbfmm.rs:1051-1086)
// UNP = 1 or 2 (the reflection axes of stage 2's basis; 0: the plain kernel): the M2L part of the child comes from Lp, stage 2's output in the parity basis, through the row function of the
// standalone pass back to the node order: L_child = (unparity(Lp_child) + (has_x ? L_child : 0)) + T_child^T L_parent, the
// association of that pass, P2L and the plain kernel one after the other.  Cells in no stage-2 tile (has_m2l = 0) take 0 and
// do not read Lp; only cells with an X list hold anything in L before (P2L, onto rows zeroed by launch_zero_rows).
template <int P, int UNP>
__global__ __launch_bounds__(64 * XFER_WAVES) void l2l3_kernel(const DevCheb *__restrict__ chp, int K, int64_t C,
                                                               const int32_t *__restrict__ cells, int n_cells,
                                                               const int32_t *__restrict__ parent,
                                                               const int32_t *__restrict__ octant,
                                                               const uint8_t *__restrict__ active,
                                                               double *__restrict__ L, M2lUnparityRowArgs unp,
                                                               const double *__restrict__ Lp,
                                                               const uint8_t *__restrict__ has_m2l,
                                                               const uint8_t *__restrict__ has_x) {
    constexpr int N = P * P * P;
    __shared__ double s_buf[XFER_WAVES][N];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int job = blockIdx.x * XFER_WAVES + wave;
    if (job >= n_cells) return;
    const int c = __builtin_amdgcn_readfirstlane(cells[job]);
    if (active && !active[c]) return;
    const int Pc = __builtin_amdgcn_readfirstlane(parent[c]);
    if (Pc < 0) return;
    const int oct = __builtin_amdgcn_readfirstlane(octant[c]);
    const int n_pad = chp->n_pad;
    bool hm = false, hx = false;
    if constexpr (UNP != 0) {
        hm = __builtin_amdgcn_readfirstlane((int)has_m2l[c]) != 0;
        hx = __builtin_amdgcn_readfirstlane((int)has_x[c]) != 0;
    }
    for (int k = 0; k < K; ++k) {
        transfer3_wave<P, false>(L + ((int64_t)k * C + Pc) * n_pad, s_buf[wave], chp->xfer, oct, lane);
        double *Lc = L + ((int64_t)k * C + c) * n_pad;
        if constexpr (UNP != 0) {
            const double *tr = s_buf[wave];
            // (The row of Lp is read here, behind the transfer, one representative after the other.  Loading all of it before the
            // transfer, to hide its latency, was measured slower at order 7: 101 registers halve the waves per SIMD, L2L 0.65
            // against 0.61 ms at 10M points.  The order and p1 = p2 = P as constants: no integer division by a kernel argument.)
            const double *src = Lp + ((int64_t)k * C + c) * unp.n_par;
            const auto add = [&](int m, double v) { Lc[m] = (v + (hx ? Lc[m] : 0.0)) + tr[m]; };
            if (hm && UNP == 2) m2l_unparity2_row(src, unp.plan, P, P, lane, add);
            else if (hm) m2l_unparity_row(src, unp.ne16, unp.n_e, unp.n_o, P, P * P, lane, add);
            else
                for (int I = lane; I < N; I += 64) Lc[I] = (0.0 + (hx ? Lc[I] : 0.0)) + tr[I];
        } else {
            for (int I = lane; I < N; I += 64) Lc[I] += s_buf[wave][I];
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Rows of L that P2L is about to add to: one wave per (right-hand side, listed cell), all n_pad values.
__global__ __launch_bounds__(256) void zero_rows_kernel(const int32_t *__restrict__ cells, int n_cells, int n_pad, int K, int64_t C,
                                                        double *__restrict__ L) {
    const int64_t job = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (job >= static_cast<int64_t>(K) * n_cells) return;
    double *row = L + ((job / n_cells) * C + cells[job % n_cells]) * n_pad;
    for (int j = threadIdx.x & 63; j < n_pad; j += 64) row[j] = 0.0;
}

void launch_zero_rows(const int32_t *cells, int n_cells, int n_pad, int K, int64_t C, double *L, hipStream_t s) {
    if (n_cells <= 0 || K <= 0) return;
    hipLaunchKernelGGL(zero_rows_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(K) * n_cells + 3) / 4)), dim3(256), 0, s, cells,
                       n_cells, n_pad, K, C, L);
}

// multipole_to_multipole, one workgroup per parent, one wave per child:
// M_parent += sum_children T_child M_child (bbfmm.rs:742-772)
// PAR: the wave also writes its child's row of Mp, the multipoles in stage 1's parity basis, through the row function of
// the standalone change of basis.  It reads the child's M from global memory as the transfer does: the two sets of loads
// are in flight together and meet in the cache, where a copy through the wave's LDS slice would put the change of basis
// between the loads and the transfer.  The children of all parents are the cells of level >= 2, the ones stage 1 reads.
template <int P, bool PAR>
__global__ __launch_bounds__(512) void m2m3_kernel(const DevCheb *__restrict__ chp, int K, int64_t C,
                                                   const int32_t *__restrict__ parents,
                                                   const int64_t *__restrict__ child_ptr,
                                                   const int32_t *__restrict__ child_idx,
                                                   const int32_t *__restrict__ octant, double *__restrict__ M,
                                                   M2lParityRowArgs par, double *__restrict__ Mpar) {
    constexpr int N = P * P * P;
    __shared__ double s_buf[8][N];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int Pc = parents[blockIdx.x];
    const int64_t c0 = child_ptr[Pc];
    const int n_ch = (int)(child_ptr[Pc + 1] - c0); // <= 8 in 3-D
    const int n_pad = chp->n_pad;
    for (int k = 0; k < K; ++k) {
        if (wave < n_ch) {
            const int ch = __builtin_amdgcn_readfirstlane(child_idx[c0 + wave]);
            const int oct = __builtin_amdgcn_readfirstlane(octant[ch]);
            const double *Mc = M + ((int64_t)k * C + ch) * n_pad;
            if constexpr (PAR) { // (the order and p1 = p2 = P as constants: no integer division by a kernel argument)
                double *dst = Mpar + ((int64_t)k * C + ch) * par.n_par;
                if (par.axes == 2) m2l_parity2_row(Mc, dst, par.off, P, P, lane);
                else m2l_parity_row(Mc, dst, par.ne16, par.n_e, par.n_o, P, P * P, lane);
            }
            transfer3_wave<P, true>(Mc, s_buf[wave], chp->xfer, oct, lane);
        }
        __syncthreads();
        double *Mp = M + ((int64_t)k * C + Pc) * n_pad;
        for (int I = threadIdx.x; I < N; I += 512) {
            double s = 0.0;
            for (int w = 0; w < n_ch; ++w) s += s_buf[w][I];
            Mp[I] = s; // a parent is written once
        }
        __syncthreads();
    }
}

bool m2m_writes_parity(const ChebRef &ch) { return ch.d == 3 && ch.p >= 2 && ch.p <= 10; }
bool l2l_reads_parity(const ChebRef &ch) { return ch.d == 3 && ch.p >= 2 && ch.p <= 12; }

int launch_m2m(const ChebRef &ch, int K, int64_t C, const int32_t *parents, int n_parents, const int64_t *child_ptr,
               const int32_t *child_idx, const int32_t *octant, double *M, hipStream_t s, const M2lParityRowArgs *par, double *Mp) {
    if (n_parents == 0) return 0;
    if (par && (!Mp || !m2m_writes_parity(ch))) return static_cast<int>(hipErrorInvalidValue); // (no kernel writes Mp here)
    // wave-per-child register kernels (8 x P^3 doubles of LDS)
    if (ch.d == 3 && dispatch_order<2, 10>(ch.p, [&](auto pc) {
            if (par)
                hipLaunchKernelGGL((m2m3_kernel<decltype(pc)::value, true>), dim3(n_parents), dim3(512), 0, s, ch.dev, K, C, parents,
                                   child_ptr, child_idx, octant, M, *par, Mp);
            else
                hipLaunchKernelGGL((m2m3_kernel<decltype(pc)::value, false>), dim3(n_parents), dim3(512), 0, s, ch.dev, K, C, parents,
                                   child_ptr, child_idx, octant, M, M2lParityRowArgs{}, nullptr);
        }))
        return 0;
    const size_t lds = sizeof(double) * (3 * (size_t)ch.n + 2 * ch.p * ch.p);
    static std::atomic<uint64_t> attr_set[4] = {{0}, {0}, {0}, {0}};
    if (const hipError_t e = allow_large_dynamic_lds(reinterpret_cast<const void *>(&m2m_kernel), lds, attr_set)) return static_cast<int>(e);
    hipLaunchKernelGGL(m2m_kernel, dim3(n_parents), dim3(256), lds, s, ch.dev, K, C, parents, child_ptr, child_idx,
                       octant, M);
    return 0;
}

int launch_l2l(const ChebRef &ch, int K, int64_t C, const int32_t *cells, int n_cells, const int32_t *parent,
               const int32_t *octant, const uint8_t *active, double *L, hipStream_t s, const M2lUnparityRowArgs *unp, const double *Lp,
               const uint8_t *has_m2l, const uint8_t *has_x) {
    if (n_cells == 0) return 0;
    if (unp && (!Lp || !has_m2l || !has_x || !l2l_reads_parity(ch))) return static_cast<int>(hipErrorInvalidValue); // (no kernel reads Lp here)
    if (ch.d == 3 && dispatch_order<2, 12>(ch.p, [&](auto pc) {
            const dim3 grid((n_cells + XFER_WAVES - 1) / XFER_WAVES), block(64 * XFER_WAVES);
            if (unp && unp->axes == 2)
                hipLaunchKernelGGL((l2l3_kernel<decltype(pc)::value, 2>), grid, block, 0, s, ch.dev, K, C, cells, n_cells, parent, octant,
                                   active, L, *unp, Lp, has_m2l, has_x);
            else if (unp)
                hipLaunchKernelGGL((l2l3_kernel<decltype(pc)::value, 1>), grid, block, 0, s, ch.dev, K, C, cells, n_cells, parent, octant,
                                   active, L, *unp, Lp, has_m2l, has_x);
            else
                hipLaunchKernelGGL((l2l3_kernel<decltype(pc)::value, 0>), grid, block, 0, s, ch.dev, K, C, cells, n_cells, parent, octant,
                                   active, L, M2lUnparityRowArgs{}, nullptr, nullptr, nullptr);
        }))
        return 0;
    const size_t lds = sizeof(double) * (2 * (size_t)ch.n + 2 * ch.p * ch.p);
    static std::atomic<uint64_t> attr_set[4] = {{0}, {0}, {0}, {0}};
    if (const hipError_t e = allow_large_dynamic_lds(reinterpret_cast<const void *>(&l2l_kernel), lds, attr_set)) return static_cast<int>(e);
    hipLaunchKernelGGL(l2l_kernel, dim3(n_cells), dim3(256), lds, s, ch.dev, K, C, cells, parent, octant, active, L);
    return 0;
}

} // namespace bbfmm
