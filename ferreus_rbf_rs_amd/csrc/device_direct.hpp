// What the pair kernels of device_p2p.hip (points against points) and device_wx.hip (points against the Chebyshev
// nodes of cells) share.  Internal to those two files.
#pragma once
#include "device_common.hpp"

namespace bbfmm {

// ------------------------------------------------------------------ direct interactions
// Shared inner loop of P2P / M2P / P2L: every thread owns two targets and one "slice" of the
// staged source tile (stride S); sources are read from LDS as {x, y}, z, w and serve both targets
// (half the LDS traffic per kernel evaluation of a one-target loop, which ran at ~70 % of the LDS
// bandwidth).  acc[t][kk] += K(t, s) * w_kk(s); gradient accumulators optional.
constexpr int DIRECT_TILE = 512;
constexpr int DIRECT_KB = 4;
constexpr int DIRECT_KB_WIDE = 8; // P2P values without gradients: eight rhs per kernel evaluation (config 4)

template <int KB> struct SrcTile { // LDS per workgroup: 12 KB + 4 KB per right-hand side of the pass
    double2 xy[DIRECT_TILE];
    double zs[DIRECT_TILE];
    double w[KB][DIRECT_TILE];
};

template <int KID, bool GRAD, int KB>
__device__ inline void direct_tile(const KernelSpec &ks, const SrcTile<KB> &tile, int count, int first, int stride,
                                   const double (&t)[2][3], double (&acc)[2][KB], double (&gacc)[2][KB][3]) {
    for (int j = first; j < count; j += stride) {
        const double2 xy = tile.xy[j];
        const double z = tile.zs[j];
        double wk[KB];
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) wk[kk] = tile.w[kk][j];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double dx = t[h][0] - xy.x, dy = t[h][1] - xy.y, dz = t[h][2] - z;
            const double r2 = dx * dx + dy * dy + dz * dz; // distance_sq, utils.rs:230-237
            if (GRAD) {
                double f;
                const double v = kernel_value_grad_r2<KID>(ks, r2, &f);
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) {
                    acc[h][kk] += v * wk[kk];
                    gacc[h][kk][0] += (f * dx) * wk[kk];
                    gacc[h][kk][1] += (f * dy) * wk[kk];
                    gacc[h][kk][2] += (f * dz) * wk[kk];
                }
            } else {
                const double v = kernel_value_r2<KID>(ks, r2);
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) acc[h][kk] += v * wk[kk];
            }
        }
    }
}

// Split nt targets into m passes of n_c targets; a pass runs ceil(n_c / 2) target pairs in
// S = 256 / pairs source slices, so the source tiles are walked m / S times in total.
struct TargetPlan {
    int n_c, pairs, S;
};
// fixed: passes of 64 targets in 8 source slices whatever nt is, so that the order in which a target's sum is formed does
// not depend on how many other targets of the call share its leaf (FmmTree::evaluate_leaves_device, batch_independent).
__device__ inline TargetPlan plan_targets(int nt, int fixed = 0) {
    if (fixed) return TargetPlan{64, 32, 8};
    const int m0 = (nt + 511) / 512;
    TargetPlan best{nt, 256, 1};
    float best_cost = 1e30f;
    for (int m = m0; m < m0 + 4; ++m) {
        const int nc = (nt + m - 1) / m, pairs = (nc + 1) / 2, S = 256 / pairs;
        const float cost = (float)m / (float)S + 0.02f * (float)m; // + restaging the tiles per pass
        if (cost < best_cost) {
            best_cost = cost;
            best = TargetPlan{nc, pairs, S};
        }
    }
    return best;
}

// Cross-slice reduction through LDS; returns the total in the slice-0 thread.
__device__ inline double slice_reduce(double v, double *red, int ti, int sl, int S, int nt, bool participates) {
    __syncthreads();
    if (participates) red[sl * nt + ti] = v;
    __syncthreads();
    double s = 0.0;
    if (participates && sl == 0)
        for (int q = 0; q < S; ++q) s += red[q * nt + ti];
    return s;
}

// ------------------------------------------------------------------ unordered pairs (p2p_sym*_kernel, wx_sym*_kernel)
// Tile, rows per wave and waves per workgroup of the workgroup-per-job kernels; see p2p_sym_kernel.
constexpr int SYM_TILE = 768;
constexpr int SYM_TR = 6;
constexpr int SYM_WAVES = 8;
constexpr int SYM_SEG = 64; // runs packed into one tile at most
template <int KB> constexpr int sym_tile() { return KB <= 2 ? SYM_TILE : SYM_TILE / 2; }
template <int KB> constexpr int sym_rows_pass() { return KB == 1 ? SYM_TR : 3; }

template <int KB> struct SymTile {
    static constexpr int T = sym_tile<KB>();
    double x[T], y[T], z[T], w[KB][T], col[KB][T];
    int32_t cidx[T]; // target position of a two-sided column, -1 for a one-sided one
    int32_t seg_src[SYM_SEG], seg_off[SYM_SEG], seg_two[SYM_SEG]; // runs packed into the tile
    int32_t fill, nseg, next_pos;
    int64_t next_q;
};

// The value is loaded whatever the flag says (a load inside `flag ? load : 0` sits behind a branch of its own, and a
// chunk's dozen scalar loads then wait for one another instead of going out together).
__device__ inline double keep_if(bool keep, double loaded) { return keep ? loaded : 0.0; }

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One pass: NR rows (sorted sources g0 .. g0 + NR, wave-uniform) against the tile.  ALLCOLS: every column takes its column
// sum (the nodes of W cells); otherwise only the two-sided ones (cidx >= 0) are flushed by the caller.  The rows' sums over this tile are reduced
// across the wave and added to out[row0 + r] at once (rows outside [win_lo, win_hi) are dropped: a partition's window) --
// the accumulators do not outlive the pass, so the kernel holds NR of them whatever the size of the leaf.
template <int KID, int NR, bool ALLCOLS>
__device__ inline void sym3_pass(const KernelSpec &ks, SymTile<1> &tile, int fill, int lane, int g0, int row0, const Xyz &src,
                                 const double *__restrict__ ws, double *__restrict__ out, int win_lo, int win_hi) {
    double tx[NR], ty[NR], tz[NR], tw[NR], racc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) { // wave-uniform: scalar loads, SGPR operands
        tx[r] = src.x[g0 + r], ty[r] = src.y[g0 + r], tz[r] = src.z[g0 + r];
        tw[r] = ws[g0 + r];
        racc[r] = 0.0;
    }
    for (int j = lane; j < fill; j += 64) {
        const double xs = tile.x[j], ys = tile.y[j], zs = tile.z[j], wj = tile.w[0][j];
        double csum = 0.0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const double dx = tx[r] - xs, dy = ty[r] - ys, dz = tz[r] - zs;
            const double v = kernel_value_r2<KID>(ks, dx * dx + dy * dy + dz * dz);
            racc[r] += v * wj;
            csum += v * tw[r];
        }
        // (one-sided columns -- cidx < 0: the leaf itself, another part's points -- collect their sums too and are skipped
        // when the tile is flushed: cheaper than reading cidx and masking the add in every iteration)
        unsafeAtomicAdd(&tile.col[0][j], csum);
    }
    if constexpr (NR >= 4) {
        // eight (padded) row sums across the wave by halving: lanes l and l ^ 32 split the rows between them and exchange
        // the halves they give up (four exchanges), then l ^ 16 (two), then l ^ 8 (one) -- every lane is left with ONE row,
        // (l >> 3) & 7, summed over eight lanes -- and three plain steps finish it: 10 exchanges where NR separate
        // reductions took 6 NR (a pass of eight rows: 48), 8 % of a LinearRbf pass.
        const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
        double u[4], t2[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double a = racc[i], b = i + 4 < NR ? racc[i + 4 < NR ? i + 4 : 0] : 0.0;
            u[i] = (b5 ? b : a) + __shfl_xor(b5 ? a : b, 32, 64);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) t2[i] = (b4 ? u[i + 2] : u[i]) + __shfl_xor(b4 ? u[i] : u[i + 2], 16, 64);
        double tot = (b3 ? t2[1] : t2[0]) + __shfl_xor(b3 ? t2[0] : t2[1], 8, 64);
        tot += __shfl_xor(tot, 4, 64);
        tot += __shfl_xor(tot, 2, 64);
        tot += __shfl_xor(tot, 1, 64);
        const int r = (lane >> 3) & 7, o = row0 + r;
        if ((lane & 7) == 0 && r < NR && o >= win_lo && o < win_hi) unsafeAtomicAdd(&out[o], tot);
    } else {
        double mine = 0.0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const double sres = wave_sum(racc[r]);
            if (lane == r) mine = sres;
        }
        const int o = row0 + lane;
        if (lane < NR && o >= win_lo && o < win_hi) unsafeAtomicAdd(&out[o], mine);
    }
}

// A wave's nr rows in passes of at most MAXR rows, all of sz or sz + 1 rows (equal passes: a pass of one or two rows costs
// a third of a full one -- the tile's LDS reads and the column bookkeeping do not shrink with it: 153-row leaves as single
// jobs with passes 6 + 6 + 6 + 1 ran 15.2 ms against 10.9 for two half leaves)
template <int KID, int MAXR, bool ALLCOLS>
__device__ inline void sym3_rows(const KernelSpec &ks, SymTile<1> &tile, int fill, int lane, int g_lo, int row_lo, int nr,
                                 const Xyz &src, const double *__restrict__ ws, double *__restrict__ out, int win_lo, int win_hi) {
    const int npass = (nr + MAXR - 1) / MAXR;
    const int sz = npass > 0 ? nr / npass : 0, big = nr - sz * npass;
    int row = 0;
    for (int p = 0; p < npass; ++p) {
        const int cnt = sz + (p < big ? 1 : 0);
        const int g0 = g_lo + row, row0 = row_lo + row;
        switch (cnt) { // wave-uniform
        case 1: sym3_pass<KID, 1, ALLCOLS>(ks, tile, fill, lane, g0, row0, src, ws, out, win_lo, win_hi); break;
        case 2: sym3_pass<KID, 2, ALLCOLS>(ks, tile, fill, lane, g0, row0, src, ws, out, win_lo, win_hi); break;
        case 3: sym3_pass<KID, 3, ALLCOLS>(ks, tile, fill, lane, g0, row0, src, ws, out, win_lo, win_hi); break;
        case 4: sym3_pass<KID, 4, ALLCOLS>(ks, tile, fill, lane, g0, row0, src, ws, out, win_lo, win_hi); break;
        case 5: sym3_pass<KID, 5, ALLCOLS>(ks, tile, fill, lane, g0, row0, src, ws, out, win_lo, win_hi); break;
        case 6: sym3_pass<KID, 6, ALLCOLS>(ks, tile, fill, lane, g0, row0, src, ws, out, win_lo, win_hi); break;
        case 7: if constexpr (MAXR >= 7) sym3_pass<KID, 7, ALLCOLS>(ks, tile, fill, lane, g0, row0, src, ws, out, win_lo, win_hi); break;
        case 8: if constexpr (MAXR >= 8) sym3_pass<KID, 8, ALLCOLS>(ks, tile, fill, lane, g0, row0, src, ws, out, win_lo, win_hi); break;
        default: break;
        }
        row += cnt;
    }
}

// rows per whole-leaf job from the environment: 0 (no such jobs) or at least a chunk job's worth
inline int sym3_rows_knob(const char *name, int dflt) {
    const int x = env_int(name, dflt);
    return x <= 0 ? 0 : std::max(x, SYM_WAVES * SYM_TR);
}
inline int p2p_sym3_max_rows_per_pass() { // of the whole-leaf kernels of both files
    static const int v = env_int("BBFMM_P2P_SYM_LEAF_PASS", 8) == 6 ? 6 : 8; // rows per pass: 8 (default) or 6
    return v;
}

} // namespace bbfmm
