// The near field: the ordered-pair P2P kernel and the three unordered-pair kernels of the matvec, their launchers
// and the knobs that size their jobs.
#include "device_direct.hpp"

namespace bbfmm {

// particle_to_particle (bbfmm.rs:1162-1251).  One workgroup per target leaf.
template <int KID, bool GRAD, int KB>
__global__ __launch_bounds__(256) void p2p_kernel(KernelSpec ks, int d, DirectJobs jobs, Xyz tgt, int64_t n_tgt,
                                                  Xyz src, const double *__restrict__ ws, int64_t N, int k0, int kb,
                                                  double *__restrict__ out, double *__restrict__ grad, int fixed_plan) {
    __shared__ SrcTile<KB> tile;
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int job = blockIdx.x;
    const int t0 = jobs.tgt_begin[job], t1 = jobs.tgt_end[job];
    const int jcell = jobs.job_cell[job];
    const int64_t r0 = jobs.run_ptr[jcell], r1 = jobs.run_ptr[jcell + 1];
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
            const int sb = jobs.runs[2 * r], se = jobs.runs[2 * r + 1];
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
                if (wr) out[(int64_t)(k0 + kk) * n_tgt + it] += v;
                if (GRAD) {
                    for (int a = 0; a < d; ++a) {
                        const double g = slice_reduce(gacc[h][kk][a], red, ti, sl, tp.S, tp.pairs, part);
                        if (wr) grad[((int64_t)(k0 + kk) * d + a) * n_tgt + it] += g;
                    }
                }
            }
        }
    }
}

// particle_to_particle with targets = sources (the matvec): every unordered pair of points once.
// The reference evaluates phi(x_i, x_j) for both (i, j) and (j, i) (bbfmm.rs:1162-1251 runs once per target
// leaf over its whole U list); U lists are symmetric and so is every kernel of the closed set, so a leaf A
// here takes only the part of its U list that lies AFTER it in the sorted order ("two-sided" runs): each
// value phi(a_i, b_j) is added to the row sum of a_i (times w_b[j]) and to the column sum of b_j (times
// w_a[i]).  "One-sided" runs (the leaf itself; for a partition the U points other ranks own) only feed the
// rows.  A job = up to SYM_WAVES * SYM_TR consecutive targets of one leaf, one workgroup (8 waves) each: a wave
// owns up to SYM_TR targets whose coordinates are wave-uniform (scalar loads), its lanes walk the staged source
// tile -- the leaf's runs packed back to back, lane-linear LDS reads; row sums stay in registers over all
// tiles and are reduced across the wave once, column sums go to an LDS accumulator by ds_add_f64 (distinct
// addresses inside a wave) and from there to HBM with one f64 atomic per source and tile.  One right-hand
// side per launch (more rhs take the ordered-pair kernel above).
// KB right-hand sides in one pass (round 4): one kernel evaluation feeds KB row and KB column sums; the rows of a wave
// go by in passes of sym_rows_pass<KB>() (their weights are SGPR operands), the tile shrinks with KB so that its
// weights and column accumulators stay under 64 KB of LDS.  rhs k reads ws + k * ldw and adds to out + k * ldo.
struct SymJobs {
    int n_jobs;
    const int32_t *tgt_begin, *tgt_end; // targets of job i: positions in the target set (sorted order)
    const int64_t *run_range;           // 2 per job: first and one-past-last run of the job's leaf
    const int32_t *runs;                // 3 ints per run: begin, end (sorted source indices), 1 = two-sided
    int32_t tgt_off;                    // sorted source index of target position 0
};

template <int KID, int KB>
__global__ __launch_bounds__(64 * SYM_WAVES) void p2p_sym_kernel(KernelSpec ks, SymJobs jobs, Xyz src,
                                                                const double *__restrict__ ws, int64_t ldw, int kb,
                                                                double *__restrict__ out, int64_t ldo) {
    constexpr int T = sym_tile<KB>();
    constexpr int TRP = sym_rows_pass<KB>();
    __shared__ SymTile<KB> tile;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int job = blockIdx.x;
    const int t0 = jobs.tgt_begin[job], t1 = jobs.tgt_end[job];
    const int rpw = (t1 - t0 + SYM_WAVES - 1) / SYM_WAVES; // rows per wave, <= SYM_TR
    const int r_lo = min(t0 + wave * rpw, t1);
    const int nr = min(rpw, t1 - r_lo);
    double racc[SYM_TR][KB];
#pragma unroll
    for (int r = 0; r < SYM_TR; ++r)
#pragma unroll
        for (int k = 0; k < KB; ++k) racc[r][k] = 0.0;
    int64_t q = jobs.run_range[2 * job];
    const int64_t q1 = jobs.run_range[2 * job + 1];
    int pos = 0; // points of run q already staged
    while (q < q1) {
        __syncthreads(); // the previous tile has been read and its columns flushed
        // The tile's segment table: up to SYM_SEG runs packed back to back until T columns are full.  One
        // wave reads the run triples in one go and scans their lengths; then every thread finds the run of its
        // column by bisection in LDS, so that all source loads of the tile leave in one batch (one memory round
        // trip for the table, one for the columns, whatever the number of runs).
        if (wave == 0) {
            const int64_t r = q + lane;
            const bool valid = r < q1;
            int b = valid ? jobs.runs[3 * r] : 0;
            const int e = valid ? jobs.runs[3 * r + 1] : 0;
            const int two = valid ? jobs.runs[3 * r + 2] : 0;
            if (lane == 0) b += pos;
            const int len = e - b;
            int incl = len;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            const int excl = incl - len;
            const int take = min(len, max(T - excl, 0));
            tile.seg_src[lane] = b;
            tile.seg_off[lane] = excl;
            tile.seg_two[lane] = two;
            const unsigned long long used = __ballot(take > 0);
            const int nseg = __popcll(used);
            if (lane == nseg - 1) {
                const bool full = take == len;
                tile.fill = excl + take;
                tile.nseg = nseg;
                tile.next_q = q + lane + (full ? 1 : 0);
                tile.next_pos = full ? 0 : ((lane == 0 ? pos : 0) + take);
            }
        }
        __syncthreads();
        const int fill = tile.fill, nseg = tile.nseg;
        q = tile.next_q;
        pos = tile.next_pos;
        for (int j = tid; j < fill; j += 64 * SYM_WAVES) {
            int lo = 0, hi = nseg;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (tile.seg_off[mid] <= j) lo = mid;
                else hi = mid;
            }
            const int g = tile.seg_src[lo] + (j - tile.seg_off[lo]);
            tile.x[j] = src.x[g];
            tile.y[j] = src.y[g];
            tile.z[j] = src.z[g];
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                tile.w[k][j] = ws[min(k, kb - 1) * ldw + g]; // (idle slots repeat the last rhs; their sums are never stored)
                tile.col[k][j] = 0.0;
            }
            tile.cidx[j] = tile.seg_two[lo] ? g - jobs.tgt_off : -1;
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < SYM_TR; p += TRP) {
            if (p < nr) { // wave-uniform
                double tx[TRP], ty[TRP], tz[TRP], tw[TRP][KB];
#pragma unroll
                for (int r = 0; r < TRP; ++r) { // sorted source index of the target (wave-uniform: scalar loads)
                    const int g = jobs.tgt_off + min(r_lo + min(p + r, nr - 1), t1 - 1);
                    tx[r] = src.x[g], ty[r] = src.y[g], tz[r] = src.z[g];
#pragma unroll
                    for (int k = 0; k < KB; ++k) tw[r][k] = keep_if(p + r < nr, ws[min(k, kb - 1) * ldw + g]);
                }
                for (int j = lane; j < fill; j += 64) {
                    const double xs = tile.x[j], ys = tile.y[j], zs = tile.z[j];
                    double wj[KB], csum[KB];
#pragma unroll
                    for (int k = 0; k < KB; ++k) wj[k] = tile.w[k][j], csum[k] = 0.0;
#pragma unroll
                    for (int r = 0; r < TRP; ++r) {
                        if (p + r < SYM_TR) { // (rows past nr are clamped copies with weight 0; their row sums are dropped)
                            const double dx = tx[r] - xs, dy = ty[r] - ys, dz = tz[r] - zs;
                            const double v = kernel_value_r2<KID>(ks, dx * dx + dy * dy + dz * dz);
#pragma unroll
                            for (int k = 0; k < KB; ++k) {
                                racc[p + r < SYM_TR ? p + r : 0][k] += v * wj[k];
                                csum[k] += v * tw[r][k];
                            }
                        }
                    }
                    if (tile.cidx[j] >= 0) {
#pragma unroll
                        for (int k = 0; k < KB; ++k)
                            if (k < kb) unsafeAtomicAdd(&tile.col[k][j], csum[k]);
                    }
                }
            }
        }
        __syncthreads();
        for (int j = tid; j < fill; j += 64 * SYM_WAVES) {
            const int c = tile.cidx[j];
            if (c >= 0) {
#pragma unroll
                for (int k = 0; k < KB; ++k)
                    if (k < kb) unsafeAtomicAdd(&out[k * ldo + c], tile.col[k][j]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < SYM_TR; ++r) {
        if (r < nr) {
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                if (k < kb) {
                    const double s = wave_sum(racc[r][k]);
                    if (lane == 0) unsafeAtomicAdd(&out[k * ldo + r_lo + r], s);
                }
            }
        }
    }
}

// ---- the workgroup kernel for WHOLE big leaves, one right-hand side (round 6).  The kernel above takes a leaf of 153
// rows (40M points) as four jobs of 38-39: every job stages the same tiles and flushes the same column sums again, and its
// eight waves get five rows each, computed as six (rows per wave are padded to the pass) -- 0.80 of the pair arithmetic
// it executes is real, and the potentials are written 54 times over (profiles/r05_final_config5_size_*_counters.txt).
// Here a job is a leaf (bigger ones than p2p_sym3_rows_per_job() in equal parts): its rows are dealt to the waves
// evenly (counts differ by one at most), a wave runs them against a tile as full passes of SYM_TR rows plus ONE pass of
// exactly the remaining rows (six instances of the pass, selected by a wave-uniform switch): no padded row is ever
// evaluated.  A pass reduces its row sums across the wave and adds them to the potentials at once -- accumulators that
// lived over all tiles cost the kernel its occupancy (111 VGPRs for three passes' worth, 164 for five: 11.1 and 19.9 ms
// at 5M Spheroidal3 points against 12.4 for the chunk kernel); column sums collect in the tile's LDS accumulator over
// all of the leaf's rows and leave with one atomic per source and (leaf, tile).
template <int KID, int MAXR>
__global__ __launch_bounds__(64 * SYM_WAVES) void p2p_sym3_kernel(KernelSpec ks, SymJobs jobs, Xyz src,
                                                                 const double *__restrict__ ws, double *__restrict__ out) {
    constexpr int T = sym_tile<1>();
    __shared__ SymTile<1> tile;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int job = blockIdx.x;
    const int t0 = jobs.tgt_begin[job], t1 = jobs.tgt_end[job];
    const int rows = t1 - t0, base = rows / SYM_WAVES, extra = rows - base * SYM_WAVES;
    const int nr = base + (wave < extra ? 1 : 0);
    const int r_lo = t0 + wave * base + min(wave, extra);
    const int g_lo = jobs.tgt_off + r_lo;                       // sorted source index of the wave's first row
    int64_t q = jobs.run_range[2 * job];
    const int64_t q1 = jobs.run_range[2 * job + 1];
    int pos = 0;
    while (q < q1) {
        __syncthreads(); // the previous tile has been read and its columns flushed
        if (wave == 0) { // the tile's segment table, as in p2p_sym_kernel
            const int64_t r = q + lane;
            const bool valid = r < q1;
            int bq = valid ? jobs.runs[3 * r] : 0;
            const int e = valid ? jobs.runs[3 * r + 1] : 0;
            const int two = valid ? jobs.runs[3 * r + 2] : 0;
            if (lane == 0) bq += pos;
            const int len = e - bq;
            int incl = len;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            const int excl = incl - len;
            const int take = min(len, max(T - excl, 0));
            tile.seg_src[lane] = bq;
            tile.seg_off[lane] = excl;
            tile.seg_two[lane] = two;
            const unsigned long long used = __ballot(take > 0);
            const int nseg = __popcll(used);
            if (lane == nseg - 1) {
                const bool full = take == len;
                tile.fill = excl + take;
                tile.nseg = nseg;
                tile.next_q = q + lane + (full ? 1 : 0);
                tile.next_pos = full ? 0 : ((lane == 0 ? pos : 0) + take);
            }
        }
        __syncthreads();
        const int fill = tile.fill, nseg = tile.nseg;
        q = tile.next_q;
        pos = tile.next_pos;
        for (int j = tid; j < fill; j += 64 * SYM_WAVES) {
            int lo = 0, hi = nseg;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (tile.seg_off[mid] <= j) lo = mid;
                else hi = mid;
            }
            const int g = tile.seg_src[lo] + (j - tile.seg_off[lo]);
            tile.x[j] = src.x[g];
            tile.y[j] = src.y[g];
            tile.z[j] = src.z[g];
            tile.w[0][j] = ws[g];
            tile.col[0][j] = 0.0;
            tile.cidx[j] = tile.seg_two[lo] ? g - jobs.tgt_off : -1;
        }
        __syncthreads();
        sym3_rows<KID, MAXR, false>(ks, tile, fill, lane, g_lo, r_lo, nr, src, ws, out, 0, 0x7fffffff);
        __syncthreads();
        for (int j = tid; j < fill; j += 64 * SYM_WAVES) {
            const int c = tile.cidx[j];
            if (c >= 0) unsafeAtomicAdd(&out[c], tile.col[0][j]);
        }
    }
}

// ---- the same unordered-pair sums, one WAVE per job (round 3).  The workgroup version above spends a third of its
// busy cycles around the pair arithmetic (three workgroup barriers per tile, one wave building the segment table while
// seven wait, column sums through LDS atomics, six-row reductions per wave) and leaves the vector ALU idle a quarter of
// the time.  Here a wave owns a whole leaf (up to SYM2_MAX_ROWS rows):
//   * the columns of a tile (SYM2_CG x 64 sources: coordinates, weight, output index) live in REGISTERS -- lane l
//     owns columns l, l + 64, ... -- loaded once per tile through the wave's own segment table (wave-private LDS
//     slice, in-order LDS: no barrier anywhere in the kernel);
//   * the rows go by in chunks of SYM2_R whose coordinates and weights are wave-uniform (scalar loads, SGPR
//     operands); the SYM2_R pair chains of a column are independent and branch-free (rows past the leaf are clamped
//     copies with weight 0), so the compiler interleaves them;
//   * column sums stay in registers over all rows of the leaf and leave with one atomic per source and tile; row sums
//     are reduced per (tile, chunk) through a 4 KB wave-private transpose (8 ds_write_b64, 4 ds_read_b128, 3 DPP
//     steps) and one atomic per row.
//
// KB <= 4 right-hand sides in one pass (round 4; config 4's near field): one kernel evaluation feeds the KB row sums and
// the KB column sums (15 + 2 KB FP64 instructions per unordered pair for LinearRbf against 2 x (15 + KB) of the
// ordered-pair kernel) -- the reference evaluates the kernel once per rhs (bbfmm.rs:1162-1251: loop order rhs, target,
// source); the values are the same, the sums differ in order only.  A column's KB weights and KB sums live in registers
// like its coordinates; the rows' weights are wave-uniform (SGPR operands), which bounds rows-per-chunk x KB: 8 rows for
// one rhs, 4 for 2-4.  rhs k reads ws + k * ldw and adds to out + k * ldo; kb <= KB of them are live.
constexpr int SYM2_CG = 4; // column groups of a tile (5 and 6 measured at one rhs: 4.23 against 4.16 ms, one wave less per SIMD)
constexpr int SYM2_WAVES = 4;
constexpr int SYM2_MAX_ROWS = 256;
template <int KB> constexpr int sym2_rows() { return KB == 1 ? 8 : 4; }

// The transpose of the row sums: NV rows of 64 partial sums, every NV-column segment followed by two pad columns so that
// the 16-byte reads of the reduction (lane l reads segment l % LPV of row l / LPV) fall on sixteen different bank groups
// per pass (round 5: unpadded, 65 % of the kernel's LDS cycles at four rhs and 36 % at one were bank conflicts --
// SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE, profiles/r05_nearfield_counters_before.json; time unchanged, the kernel
// does not wait for its LDS: DESIGN.md section 10).
template <int NV> struct Sym2Wave { // wave-private
    static constexpr int kSeg = NV + 2, kRow = (64 / NV) * kSeg;
    double red[NV][kRow];
    int32_t seg_src[64], seg_off[64], seg_two[64];
};

template <int KID, int KB>
__global__ __launch_bounds__(64 * SYM2_WAVES) void p2p_sym2_kernel(KernelSpec ks, SymJobs jobs, Xyz src,
                                                                  const double *__restrict__ ws, int64_t ldw, int kb,
                                                                  double *__restrict__ out, int64_t ldo) {
    constexpr int R = sym2_rows<KB>();
    constexpr int NV = R * KB;        // row sums per (tile, chunk): 8 or 16
    constexpr int LPV = 64 / NV;      // lanes that share the final sum of one of them
    __shared__ Sym2Wave<NV> lds[SYM2_WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int job = blockIdx.x * SYM2_WAVES + wave;
    if (job >= jobs.n_jobs) return; // whole wave; no workgroup barrier below
    Sym2Wave<NV> &W = lds[wave];
    const int t0 = jobs.tgt_begin[job], t1 = jobs.tgt_end[job];
    int64_t q = jobs.run_range[2 * job];
    const int64_t q1 = jobs.run_range[2 * job + 1];
    int pos = 0; // points of run q already taken
    constexpr int TILE = 64 * SYM2_CG;
    while (q < q1) {
        // segment table of the tile: up to 64 runs packed back to back until TILE columns are full
        int fill, nseg;
        {
            const int64_t r = q + lane;
            const bool valid = r < q1;
            int b = valid ? jobs.runs[3 * r] : 0;
            const int e = valid ? jobs.runs[3 * r + 1] : 0;
            const int two = valid ? jobs.runs[3 * r + 2] : 0;
            if (lane == 0) b += pos;
            const int len = e - b;
            int incl = len;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            const int excl = incl - len;
            const int take = min(len, max(TILE - excl, 0));
            W.seg_src[lane] = b;
            W.seg_off[lane] = excl;
            W.seg_two[lane] = two;
            nseg = __popcll(__ballot(take > 0));
            const int last = max(nseg - 1, 0);
            fill = __builtin_amdgcn_readlane(excl + take, last);
            const int take_l = __builtin_amdgcn_readlane(take, last), len_l = __builtin_amdgcn_readlane(len, last);
            const bool full = take_l == len_l;
            const int pos_now = pos;
            q = q + last + (full ? 1 : 0);
            pos = full ? 0 : ((last == 0 ? pos_now : 0) + take_l);
            if (nseg == 0) break; // (empty runs only: cannot happen with the host's lists; never spin)
        }
        // the tile's columns into registers
        double cx[SYM2_CG], cy[SYM2_CG], cz[SYM2_CG], cw[SYM2_CG][KB], csum[SYM2_CG][KB];
        int cidx[SYM2_CG];
#pragma unroll
        for (int cg = 0; cg < SYM2_CG; ++cg) {
            const int j = cg * 64 + lane;
            cx[cg] = cy[cg] = cz[cg] = 0.0; // a padding column: weight 0, its sums are dropped
            cidx[cg] = -1;
#pragma unroll
            for (int k = 0; k < KB; ++k) cw[cg][k] = csum[cg][k] = 0.0;
            if (j < fill) {
                int lo = 0, hi = nseg;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (W.seg_off[mid] <= j) lo = mid;
                    else hi = mid;
                }
                const int g = W.seg_src[lo] + (j - W.seg_off[lo]);
                cx[cg] = src.x[g];
                cy[cg] = src.y[g];
                cz[cg] = src.z[g];
#pragma unroll
                for (int k = 0; k < KB; ++k) // (idle slots repeat the last rhs; their sums are never stored)
                    cw[cg][k] = ws[min(k, kb - 1) * ldw + g];
                cidx[cg] = W.seg_two[lo] ? g - jobs.tgt_off : -1;
            }
        }
        const int ncg = (fill + 63) >> 6; // wave-uniform
        for (int rb = t0; rb < t1; rb += R) {
            // the rows of a chunk: coordinates and weights are wave-uniform (scalar loads, SGPR operands)
            double tx[R], ty[R], tz[R], tw[R][KB], racc[R][KB];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int g = jobs.tgt_off + min(rb + r, t1 - 1);
                tx[r] = src.x[g], ty[r] = src.y[g], tz[r] = src.z[g];
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    tw[r][k] = keep_if(rb + r < t1, ws[min(k, kb - 1) * ldw + g]);
                    racc[r][k] = 0.0;
                }
            }
#pragma unroll
            for (int cg = 0; cg < SYM2_CG; ++cg) {
                if (cg < ncg) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const double dx = tx[r] - cx[cg], dy = ty[r] - cy[cg], dz = tz[r] - cz[cg];
                        const double v = kernel_value_r2<KID>(ks, dx * dx + dy * dy + dz * dz);
#pragma unroll
                        for (int k = 0; k < KB; ++k) {
                            racc[r][k] += v * cw[cg][k];
                            csum[cg][k] += v * tw[r][k];
                        }
                    }
                }
            }
            // row sums: transpose through the wave's slice; LPV lanes share one of the NV sums, each adds NV of its 64
            // partial sums (NV / 2 16-byte reads)
            const int wcol = lane + 2 * (lane / NV); // (pad columns behind every NV-column segment)
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int k = 0; k < KB; ++k) W.red[r * KB + k][wcol] = racc[r][k];
            const double2 *pr = reinterpret_cast<const double2 *>(&W.red[lane / LPV][(lane % LPV) * Sym2Wave<NV>::kSeg]);
            double sum = 0.0;
#pragma unroll
            for (int i = 0; i < NV / 2; i += 2) {
                const double2 a0 = pr[i], a1 = pr[i + 1];
                sum += (a0.x + a0.y) + (a1.x + a1.y);
            }
#pragma unroll
            for (int off = 1; off < LPV; off <<= 1) sum += __shfl_xor(sum, off, 64);
            const int vi = lane / LPV, row = rb + vi / KB, k = vi % KB;
            if (lane % LPV == 0 && row < t1 && k < kb) unsafeAtomicAdd(&out[k * ldo + row], sum);
        }
#pragma unroll
        for (int cg = 0; cg < SYM2_CG; ++cg)
            if (cg < ncg && cidx[cg] >= 0) {
#pragma unroll
                for (int k = 0; k < KB; ++k)
                    if (k < kb) unsafeAtomicAdd(&out[k * ldo + cidx[cg]], csum[cg][k]);
            }
    }
}

// ------------------------------------------------------------------ launchers and job-size knobs
void launch_p2p(const KernelSpec &ks, int d, const DirectJobs &jobs, const double *const *tgt_xyz, int64_t n_tgt,
                const double *const *src_xyz, const double *w_sorted, int64_t N, int K, double *out_sorted,
                double *grad_sorted, hipStream_t s, bool fixed_plan) {
    if (jobs.n_jobs == 0) return;
    dispatch_kernel_id(ks.id, [&](auto idc) {
        constexpr int ID = decltype(idc)::value;
        for (int k0 = 0; k0 < K;) {
            const bool wide = !grad_sorted && K - k0 > DIRECT_KB; // more than four rhs left: eight per pass
            const int kb = std::min(wide ? DIRECT_KB_WIDE : DIRECT_KB, K - k0);
            auto go = [&](auto grad, auto kbv) {
                hipLaunchKernelGGL((p2p_kernel<ID, decltype(grad)::value, decltype(kbv)::value>), dim3(jobs.n_jobs), dim3(256), 0, s, ks,
                                   d, jobs, make_xyz(tgt_xyz), n_tgt, make_xyz(src_xyz), w_sorted, N, k0, kb, out_sorted, grad_sorted,
                                   fixed_plan ? 1 : 0);
            };
            if (grad_sorted && kb == 1) go(std::true_type{}, int_c<1>{}); // single right-hand side: a quarter of the accumulators
            else if (grad_sorted) go(std::true_type{}, int_c<DIRECT_KB>{});
            else if (kb == 1) go(std::false_type{}, int_c<1>{});
            else if (wide) go(std::false_type{}, int_c<DIRECT_KB_WIDE>{});
            else go(std::false_type{}, int_c<DIRECT_KB>{});
            k0 += kb;
        }
    });
}

// K right-hand sides in passes of at most kSymMaxRhs = 4: kernel instances for 1, 2 and 4 rhs (three run the 4-slot
// instance).  Measured at 10M points, LinearRbf (scripts/p2p_rhs_sweep.py): 4.4 / 5.1 / 7.3 ms for 1 / 2 / 4 rhs; an
// 8-slot instance (two rows per chunk, 222 VGPRs, two waves per SIMD; also with point-major weights and software-pipelined
// row loads) took 16.6 ms per pass against 2 x 7.3: not kept.
void launch_p2p_sym(const KernelSpec &ks, int n_jobs, const int32_t *tgt_begin, const int32_t *tgt_end,
                    const int64_t *run_range, int n_leaf_jobs, const int32_t *l_tgt_begin, const int32_t *l_tgt_end,
                    const int64_t *l_run_range, int n_wave_jobs, const int32_t *w_tgt_begin, const int32_t *w_tgt_end,
                    const int64_t *w_run_range, const int32_t *runs3, int32_t tgt_off, const double *const *src_xyz,
                    const double *w_sorted, int64_t ldw, int K, double *out_sorted, int64_t ldo, hipStream_t s) {
    dispatch_kernel_id(ks.id, [&](auto idc) {
        constexpr int ID = decltype(idc)::value;
        const SymJobs wj{n_wave_jobs, w_tgt_begin, w_tgt_end, w_run_range, runs3, tgt_off};
        const SymJobs gj{n_jobs, tgt_begin, tgt_end, run_range, runs3, tgt_off};
        const SymJobs lj{n_leaf_jobs, l_tgt_begin, l_tgt_end, l_run_range, runs3, tgt_off};
        const Xyz src = make_xyz(src_xyz);
        for (int k0 = 0; k0 < K; k0 += kSymMaxRhs) {
            const int kb = std::min(kSymMaxRhs, K - k0);
            const double *w = w_sorted + static_cast<int64_t>(k0) * ldw;
            double *o = out_sorted + static_cast<int64_t>(k0) * ldo;
#define SYM_GO(KBV)                                                                                                   \
    do {                                                                                                              \
        if (n_wave_jobs > 0)                                                                                          \
            hipLaunchKernelGGL((p2p_sym2_kernel<ID, KBV>), dim3((n_wave_jobs + SYM2_WAVES - 1) / SYM2_WAVES),          \
                               dim3(64 * SYM2_WAVES), 0, s, ks, wj, src, w, ldw, kb, o, ldo);                         \
        if (KBV == 1 && n_leaf_jobs > 0) { /* one rhs: whole big leaves (the same rows as the chunk jobs below) */     \
            if (p2p_sym3_max_rows_per_pass() == 8)                                                                    \
                hipLaunchKernelGGL((p2p_sym3_kernel<ID, 8>), dim3(n_leaf_jobs), dim3(64 * SYM_WAVES), 0, s, ks, lj, src, w, o); \
            else                                                                                                      \
                hipLaunchKernelGGL((p2p_sym3_kernel<ID, 6>), dim3(n_leaf_jobs), dim3(64 * SYM_WAVES), 0, s, ks, lj, src, w, o); \
        } else if (n_jobs > 0)                                                                                        \
            hipLaunchKernelGGL((p2p_sym_kernel<ID, KBV>), dim3(n_jobs), dim3(64 * SYM_WAVES), 0, s, ks, gj, src, w,    \
                               ldw, kb, o, ldo);                                                                      \
    } while (0)
            if (kb == 1) SYM_GO(1);
            else if (kb == 2) SYM_GO(2);
            else SYM_GO(4);
#undef SYM_GO
        }
    });
}

// Leaves of at most this many rows are one job of the wave-per-job kernel (BBFMM_P2P_SYM_WAVE=<rows>, 0: none).
// Measured on MI355X: 38-point leaves (10M uniform points) 5.55 -> 4.46 ms with the wave kernel; 153- and 238-point
// leaves (40M, 1M points) are faster in the workgroup kernel (89.7 against 103 ms, 2.5 against 4.7 ms).
int p2p_sym_wave_rows() {
    static const int rows = std::clamp(env_int("BBFMM_P2P_SYM_WAVE", 64), 0, SYM2_MAX_ROWS);
    return rows;
}

// A launch of the wave kernel with fewer jobs than this leaves the chip to a handful of waves per SIMD, each walking its
// whole leaf alone: such trees give every leaf to a workgroup instead (eight waves share its rows).  Measured on MI355X,
// uniform points, near field per matvec, wave kernel -> workgroup kernels: 512 leaves (20k / 36k points) 0.055 -> 0.018 /
// 0.130 -> 0.035 ms, 4,096 leaves (150k / 200k / 300k) 0.134 -> 0.083 / 0.131 -> 0.112 / 0.288 -> 0.203 ms; 32,768 leaves
// (1.6M / 2M) 0.71 -> 0.89 / 1.11 -> 1.23 ms the other way.  Default 48 jobs per CU; BBFMM_P2P_SYM_WAVE_MIN=<jobs> overrides.
int64_t p2p_sym_wave_min_jobs() {
    const char *e = std::getenv("BBFMM_P2P_SYM_WAVE_MIN"); // read per plan (a handle's job lists are built once): the tests
    if (e && *e) return std::max<int64_t>(0, std::atoll(e)); // run small trees through either kind of job in one process
    return int64_t(48) * device_cu_count();
}

int p2p_sym_rows_per_job() { return SYM_WAVES * SYM_TR; }
// Whole-leaf jobs of the one-rhs workgroup kernel: rows per job (BBFMM_P2P_SYM_LEAF=<rows>; 0: no such jobs, the chunk
// jobs serve one rhs too).  A job of R rows gives each of the eight waves R / 8 of them.
int p2p_sym3_passes() {
    // (305-point leaves -- max_points_per_cell 512 at 10M points -- as ONE job: 24.3 -> 23.0 ms with 8 rows per pass)
    static const int v = sym3_rows_knob("BBFMM_P2P_SYM_LEAF", 512);
    return v;
}
int p2p_sym3_rows_per_job() { return p2p_sym3_passes(); }

} // namespace bbfmm
