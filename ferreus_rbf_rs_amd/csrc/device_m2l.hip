// M2L: the streamed-operator GEMM kernel of both stages, its chunk and split plans, and the operators' assembly in HBM.
#include "device_common.hpp"
#include "m2l_basis_rows.hpp"

#include <cmath>

namespace bbfmm {

// ------------------------------------------------------------------ M2L (MFMA FP64)
// multipole_to_local (bbfmm.rs:864-986) regrouped for the matrix cores.  The reference
// permutes each V cell's multipoles onto one of 16 reference operators, multiplies by
// Vt then U, and permutes back.  Here the permutations are folded into per-transfer-
// vector operators stacked per octant class (host side, fmm_m2l_tables.cpp), which turns the
// whole level into two dense streamed-operator GEMMs with no data permutation:
//   stage 1:  Cbuf[target(V,t)][(t,kk)] = sum_m VtAll[(t,kk)][m] * M_V[m]   (X-stationary)
//   stage 2:  L_B[i]                    = sum_k UAll[i][k] * Cbuf[B][k]     (accumulator-stationary)
// ------------------------------------------------------------------ M2L on v_mfma_f64_4x4x4_4b
// Measured on MI355X (scripts/fp64_microbench.hip): v_mfma_f64_16x16x4 sustains ~46 TFLOP/s
// chip-wide (~100-144 cycles per instruction), v_mfma_f64_4x4x4 (4 blocks) ~70 TFLOP/s (17
// cycles per 512-flop instruction).  The kernels below are the same two streamed-operator
// GEMMs as above on the faster instruction.  Lane layout (probed, scripts/mfma4_probe.hip):
//   A[b][i][k]: lane = 16k + 4b + i    B[b][k][j]: lane = 16k + 4b + j    D[b][i][j]: lane = 16i + 4b + j
// with D_b = A_b * B_b for the four independent blocks b.
//
// Stage 1 uses the blocks as four slices of the contraction index (t = lane>>2 = 4k + b selects
// the m values a lane owns), so one operator fragment feeds four cell groups and each D register
// holds four partial sums that are added across lanes (xor 4, xor 8) once per tile.
// Operator tiles are staged with the asynchronous global->LDS DMA (global_load_lds_dwordx4,
// no VGPR round trip) into two LDS buffers: the tile for step i+1 streams in while step i is
// multiplied.  The LDS image is in MFMA-fragment order, so every fragment read is a lane-linear,
// conflict-free ds_read, and the per-lane DMA source address performs the permutation from the
// operator's row-major HBM layout.  The DMA is issued from inline asm: through the builtin the
// compiler must assume the in-flight LDS write may alias every later ds_read and drains it
// (s_waitcnt vmcnt(0)) before each fragment read, which serialises the whole pipeline.
typedef __attribute__((address_space(3))) void *lptr_t;

__device__ inline unsigned lds_offset(const double *p) {
    return static_cast<unsigned>(reinterpret_cast<uintptr_t>((lptr_t)p));
}
// Wave-uniform values the compiler cannot prove uniform (derived from threadIdx.x >> 6).
__device__ inline unsigned uniform_u32(unsigned v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline const double *uniform_ptr(const double *p) {
    const uintptr_t v = reinterpret_cast<uintptr_t>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v));
    const unsigned hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v >> 32));
    return reinterpret_cast<const double *>((static_cast<uintptr_t>(hi) << 32) | lo);
}
// 64 lanes x 16 B land at LDS byte offset m0 + lane * 16 (destination = wave-uniform base + lane*16).
__device__ inline void dma16(const double *g, unsigned lds_wave_byte_offset) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g),
                 "s"(uniform_u32(lds_wave_byte_offset))
                 : "memory");
}
// 64 lanes x 4 B (a gather of table entries) land at LDS byte offset m0 + lane * 4.
__device__ inline void dma4(const int32_t *g, unsigned lds_wave_byte_offset) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(g),
                 "s"(uniform_u32(lds_wave_byte_offset))
                 : "memory");
}
__device__ inline void wait_dma_and_barrier() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}
// Same, but lets the N most recent vector-memory operations of the wave stay in flight.  gfx9
// retires loads and stores in issue order on one counter, so when N stores were issued after the
// DMA the DMA has landed once at most N operations are outstanding (the field holds 0..63).
template <int N> __device__ inline void wait_dma_keep_stores_and_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N < 63 ? N : 63) : "memory");
    __syncthreads();
}
// v + (v rotated right by N lanes inside each row of 16 lanes), via DPP row_ror
template <int N> __device__ inline double add_row_ror(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int rlo = __builtin_amdgcn_update_dpp(0, lo, 0x120 + N, 0xf, 0xf, false);
    const int rhi = __builtin_amdgcn_update_dpp(0, hi, 0x120 + N, 0xf, 0xf, false);
    return v + __hiloint2double(rhi, rlo);
}

// Same with a uniform (SGPR) base and a 32-bit per-lane byte offset: saves address VGPRs.
__device__ inline void dma16s(const double *sbase, unsigned voff_bytes, unsigned lds_wave_byte_offset) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff_bytes),
                 "s"(uniform_ptr(sbase)), "s"(uniform_u32(lds_wave_byte_offset))
                 : "memory");
}

// One kernel serves both stages: OUT[cell][col] = sum_k IN[cell][k] * OP[k][col] for the 128
// cells of a workgroup and a block of 16*NG16 output columns.
//   stage 1: IN = multipoles M (k = Chebyshev node m, n_pad of them), OP = VtAll (n_pad x r_pad),
//            col = stacked operator row (t, kk); the result is scattered into the target slots.
//   stage 2: IN = slot contents (k over the slot, k_pad), OP = UAll (k_pad x n_pad), col = node;
//            the result is the local expansion L.
//   stage 3: a plain product per cell, IN = rows of in_len values per cell (like M), OP = cls.u_all
//            (in_len x n_pad), OUT = rows of n_pad values per cell (like L): the change of basis of the
//            shared-basis extension (multipoles -> coordinates in the level's basis, and back for the locals).
// The four MFMA blocks are four groups of four output columns: A_b = operator fragment
// OP[k][col 4b + i] (one lane-linear ds_read_b64 per 16 columns, feeding four MFMAs), B_b = the
// IN values of four cells (the same for every block), D_b[i][j] = OUT[cell j][col 4b + i].  A wave
// owns 16 cells (four groups tg) and keeps 4 x NG16 accumulators; the operator tile and the
// cells' IN values of step q+1 stream into LDS by DMA while step q is multiplied.
// PAIRS (stage 1 in the parity basis of the x reflection): IN = Mp = [M_e | pad | M_o | pad] (n_pad = n_par values per
// cell), OP = [Vt_e | pad | Vt_o | pad]; the first in_len / 16 steps of a column block are the even part a, the rest
// the odd part b.  At the boundary the accumulators move to a second set, and the epilogue stores a + b through
// row_dst and, for the blocks that hold pairs, a - b through row_dst2: one product serves t and Rt.
// Two axes (in_len also carries s_ee and s_eo): IN = [M_ee | M_eo | M_oe | M_oo], each part padded to 16.  A block below
// cls.yb0 walks the parts in storage order (a over the x-even parts ee, eo: its pairs are (t, R_x t)); a block from yb0 on
// walks ee, oe, eo, oo (a over the y-even parts: its pairs are (t, R_y t)).  eo and oe are equally long, so the boundary
// between a and b is the same step in both orders; a single's a + b does not depend on the order.
template <int NG16, int STAGE, int MINW, bool PAIRS = false>
__global__ __launch_bounds__(512, MINW) void m2l_gemm_k4(const M2lClass *__restrict__ classes,
                                                  const M2lTileDesc *__restrict__ tiles, int n_pad, int g16_0,
                                                  int64_t C, const double *__restrict__ in, int64_t in_len,
                                                  double *__restrict__ out, int64_t out_len,
                                                  const uint16_t *__restrict__ qlist, int slot_t,
                                                  const int32_t *__restrict__ tile_idx) {
    // 2 x { operator [e][ng][k*16 + col], IN tile [wave][tg][eh][k][j] x 2 }; stage 1 adds the slot
    // lookups of the current column block, [wave][cell 0..15][slot_t] int32
    extern __shared__ double lds[];
    const M2lTileDesc tile = tiles[blockIdx.x];
    const M2lClass cls = classes[tile.level_class];
    const int kr = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // stage 1: the workgroup walks the column blocks zb0 .. zb1 of kM2lS1Block stacked rows (g16_0
    // selects a chunk inside a block); stage 2: one block, g16_0 selects the nodes
    constexpr int BLK = PAIRS ? kM2lS1BlockPairs : kM2lS1Block; // stacked rows per column block
    const int n_zb = STAGE == 1 ? cls.r_pad16 / BLK : 1;
    // (a tile of a sparse plan, pad == 2, names its own column blocks: q_first, q_count)
    const bool own_blocks = STAGE == 1 && tile.pad == 2;
    const int zb0 = STAGE == 1 ? (own_blocks ? tile.q_first : (int)((int64_t)n_zb * blockIdx.z / gridDim.z)) : 0;
    const int zb1 = STAGE == 1 ? (own_blocks ? tile.q_first + tile.q_count : (int)((int64_t)n_zb * (blockIdx.z + 1) / gridDim.z)) : 1;
    const int ld = STAGE == 1 ? cls.r_pad16 : n_pad;            // operator leading dimension
    // contraction steps of 16: all of them in stage 1; in stage 2 only those for which some cell
    // of the tile has a V-list entry (tile.q_first/q_count index the compact list qlist)
    // Stage 2 of a launch with few tiles is split over the contraction as well (slot_t = number of parts, the
    // parameter is stage 1's otherwise): a tile's chain of ~290 steps is what a small tree's matvec waits for.
    // blockIdx.z = part * column chunks + column chunk; the parts add their results to the zeroed L with atomics.
    const int ksplit = STAGE == 2 && slot_t > 1 ? slot_t : 1;
    const int zcols = STAGE == 2 ? (int)gridDim.z / ksplit : 1;
    const int zk = STAGE == 2 ? (int)blockIdx.z / zcols : 0, zc = STAGE == 2 ? (int)blockIdx.z - zk * zcols : (int)blockIdx.z;
    const int q_lo = STAGE == 2 ? tile.q_count * zk / ksplit : 0;
    const int nq = STAGE == 1 ? n_pad / 16 : STAGE == 2 ? tile.q_count * (zk + 1) / ksplit - q_lo : (int)(in_len / 16);
    const uint16_t *ql = qlist + tile.q_first + q_lo;
    const int nq_e = PAIRS ? (int)(in_len & 0xffffffff) / 16 : 0;
    const int s_ee = PAIRS ? (int)(in_len >> 32) & 0xffff : 0, s_eo = PAIRS ? (int)(in_len >> 48) : 0; // (0, 0: one axis)
    if (zb0 >= zb1) return;
    // stage 2 with gridDim.z > 1: the z workgroups of a tile take adjacent chunks of NG16 column groups
    const int g16 = g16_0 + (STAGE >= 2 ? zc * NG16 : 0);
    const double *opbase = (STAGE == 1 ? cls.vt_all : cls.u_all) + 16 * g16;

    constexpr int OP_CHUNKS = 2 * NG16;
    constexpr int NCH = (OP_CHUNKS + 7) / 8;
    constexpr int OP_DOUBLES = OP_CHUNKS * 128;
    constexpr int BUF = OP_DOUBLES + 2048;

    // Operator image in LDS.  The NG16 column groups are taken as NP pairs (+ one single group when
    // NG16 is odd).  A pair chunk (e, pr) is [k][p = 4b + i][2]: lane 16k + p holds columns
    // 32 pr + 2p and + 1 of row 4k + e, fetched as one 16-byte DMA granule and read back with one
    // ds_read_b128 feeding the MFMAs of groups 2 pr and 2 pr + 1.  An accumulator pair of a lane is
    // thus two ADJACENT output columns, which the epilogues store as 16 bytes (the stage-1 scatter
    // is bound by the number of store instructions).  The single group keeps [e][k][16 columns].
    constexpr int NP = NG16 / 2, NS = NG16 & 1;
    unsigned voff[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = wave + 8 * i;
        if (c < 4 * NP) {
            const int e = c / NP, pr = c - e * NP, k = lane >> 4, p = lane & 15;
            voff[i] = (unsigned)(((4 * k + e) * ld + 32 * pr + 2 * p) * 8);
        } else {
            const int e = 2 * (c - 4 * NP) + (lane >> 5), r = lane & 31, k = r >> 3, pair = r & 7;
            voff[i] = (unsigned)(((4 * k + e) * ld + 32 * NP + 2 * pair) * 8);
        }
    }
    // position of the tile's cell `pos` in its class list (a partition's source tiles are compact
    // lists of class positions, tile.pad != 0)
    auto cell_p = [&](int pos) {
        const int q = pos < tile.count ? pos : 0;
        return tile.pad ? tile_idx[tile.first + q] : tile.first + q;
    };
    // IN tile: chunk h of this wave covers tg = 2h + (lane>>5), eh = (lane>>4)&1, k = (lane>>2)&3, j = lane&3
    const double *cptr[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int tg = 2 * h + (lane >> 5), eh = (lane >> 4) & 1, k = (lane >> 2) & 3, j = lane & 3;
        const int pos = wave * 16 + 4 * tg + j;
        const int p = cell_p(pos);
        const int64_t base = STAGE == 2 ? (int64_t)kr * in_len + cls.cbase[p]
                                        : ((int64_t)kr * C + cls.cells[p]) * (STAGE == 1 ? (int64_t)n_pad : in_len);
        cptr[h] = in + base + 4 * k + 2 * eh;
    }
    const unsigned lds0 = lds_offset(lds);
    const int64_t qstride = (int64_t)16 * ld;
    // step s of the flattened (column block, contraction step) loop
    auto stage = [&](int sidx, int buf) {
        const int zb = zb0 + sidx / nq, qi = sidx - (sidx / nq) * nq;
        int q = STAGE == 2 ? (int)ql[qi] : qi;
        if constexpr (PAIRS) {
            if (zb >= cls.yb0) { // y order: the parts eo and oe change places (wave-uniform, scalar arithmetic)
                if (qi >= s_ee && qi < s_ee + s_eo) q = qi + s_eo;
                else if (qi >= s_ee + s_eo && qi < s_ee + 2 * s_eo) q = qi - s_eo;
            }
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i)
            if (wave + 8 * i < OP_CHUNKS)
                dma16s(opbase + (int64_t)zb * BLK + q * qstride, voff[i],
                       lds0 + (unsigned)(buf * BUF + (wave + 8 * i) * 128) * 8u);
#pragma unroll
        for (int h = 0; h < 2; ++h)
            dma16(cptr[h] + 16 * q, lds0 + (unsigned)(buf * BUF + OP_DOUBLES + (2 * wave + h) * 128) * 8u);
    };

    double acc[4][NG16];
    double acc_e[4][PAIRS ? NG16 : 1]; // PAIRS: the even part a, while acc collects the odd part b
#pragma unroll
    for (int tg = 0; tg < 4; ++tg)
#pragma unroll
        for (int g = 0; g < NG16; ++g) {
            acc[tg][g] = 0.0;
            if constexpr (PAIRS) acc_e[tg][g] = 0.0;
        }

    const int bk = lane >> 4, bj = lane & 3; // B layout (k, j); the block index is broadcast
    const bool wave_live = wave * 16 < tile.count;
    const int n_steps = (zb1 - zb0) * nq;
    // epilogue coordinates: D[b][i][j] at lane 16 i + 4 b + j = OUT[cell 4 tg + j][col0 + 16 g + 4 b + i]
    const int di = lane >> 4, db = (lane >> 2) & 3, dj = lane & 3;
    // Stage-1 scatter tables.  gfx9 retires vector-memory operations in issue order on one counter,
    // and the compiler cannot see the DMA in its wait counting: a wait for any ordinary load in this
    // loop would be vmcnt(0) and drain the DMA in flight and the scatter stores with it.  The loop
    // therefore issues no ordinary loads at all.  All lookups come in by DMA and are read from LDS:
    //   aux[parity][0 .. 16 NG16)  packed row entries of a column block, aux[parity][16 NG16] its first
    //                              transfer-vector position (requested during the previous block)
    //   slots[wave][cell][slot_t]  slot bases of the wave's 16 cells for the block's transfer vectors
    //                              (requested two steps before the block ends)
    // and the stores of a block leave together and drain under the next block.
    //   PAIRS: aux[parity][192 .. 192 + 16 NG16) the second destinations of the block's columns
    constexpr int AUX = PAIRS ? 384 : 192;
    const int32_t *aux = reinterpret_cast<const int32_t *>(lds + 2 * BUF);
    int32_t *ptab = reinterpret_cast<int32_t *>(lds + 2 * BUF) + 2 * AUX; // class positions of the 128 cells
    const int32_t *slds = aux + 2 * AUX + 128 + wave * 16 * slot_t;
    if (STAGE == 1 && lane < 16) ptab[wave * 16 + lane] = cell_p(wave * 16 + lane); // read by this wave only
    const unsigned aux0 = lds0 + (unsigned)(2 * BUF) * 8u;
    auto stage_cols = [&](int zb_, int par) {
        if (STAGE == 1 && 64 * wave <= 16 * NG16) {
            const int e = 64 * wave + lane;
            const int32_t *src = e < 16 * NG16 ? cls.row_dst + zb_ * BLK + 16 * g16 + e : cls.blk_t0 + zb_;
            dma4(src, aux0 + (unsigned)(par * AUX + 64 * wave) * 4u);
        } else if (PAIRS && 64 * wave < 192 + 16 * NG16) { // (16 NG16 <= 192: waves 3 .. 5)
            const int e = 64 * wave + lane - 192;
            const int32_t *src = e < 16 * NG16 ? cls.row_dst2 + zb_ * BLK + 16 * g16 + e : cls.blk_t0 + zb_;
            dma4(src, aux0 + (unsigned)(par * AUX + 64 * wave) * 4u);
        }
    };
    const int slot_sh = 31 - __builtin_clz(slot_t | 1); // slot_t is a power of two >= 16 in stage 1
    auto stage_slots = [&](int par) {
        const int t0 = __builtin_amdgcn_readfirstlane(aux[par * AUX + 16 * NG16]) & (kM2lBlkTwoDst - 1);
        const unsigned dst0 = aux0 + (unsigned)(2 * AUX + 128 + wave * 16 * slot_t) * 4u;
        for (int i = 0; i < slot_t / 4; ++i) {
            const int e = i * 64 + lane, cl = e >> slot_sh, tl = e & (slot_t - 1);
            const int32_t *src = cls.cslot + (int64_t)ptab[wave * 16 + cl] * cls.n_t + min(t0 + tl, cls.n_t - 1);
            dma4(src, dst0 + (unsigned)i * 256u);
        }
    };
    if (n_steps > 0) {
        stage(0, 0);
        stage_cols(zb0, 0);
    }
    wait_dma_and_barrier();
    int qcnt = 0, zb = zb0;
    for (int sidx = 0; sidx < n_steps; ++sidx) {
        const double *op = lds + (sidx & 1) * BUF + lane;
        const double2 *op2 = reinterpret_cast<const double2 *>(lds + (sidx & 1) * BUF) + lane;
        const double *ct = lds + (sidx & 1) * BUF + OP_DOUBLES + wave * 256 + (bk * 4 + bj) * 2;
        if (sidx + 1 < n_steps) stage(sidx + 1, (sidx + 1) & 1); // streams in under the MFMAs below
        if (STAGE == 1) {
            if (qcnt == 0 && zb + 1 < zb1) stage_cols(zb + 1, (zb + 1 - zb0) & 1);
            if (qcnt == nq - 2) stage_slots((zb - zb0) & 1);
        }
        if (wave_live) { // a wave without cells (short tile) only helps with the DMA and the barriers
            if constexpr (PAIRS) {
                if (qcnt == nq_e) { // the even part is complete: keep it, collect the odd part
#pragma unroll
                    for (int tg = 0; tg < 4; ++tg)
#pragma unroll
                        for (int g = 0; g < NG16; ++g) {
                            acc_e[tg][g] = acc[tg][g];
                            acc[tg][g] = 0.0;
                        }
                }
            }
            // the cells' values of contraction indices 2 eh, 2 eh + 1 (PAIRS holds twice the accumulators: one half
            // of the values at a time, where the other instances keep all sixteen in registers)
            constexpr int EH = PAIRS ? 1 : 2;
#pragma unroll
            for (int eh0 = 0; eh0 < 2; eh0 += EH) {
                double bq[4][2 * EH];
#pragma unroll
                for (int tg = 0; tg < 4; ++tg)
#pragma unroll
                    for (int eh = 0; eh < EH; ++eh) {
                        const double2 v = *reinterpret_cast<const double2 *>(ct + ((tg * 2 + eh0 + eh) * 16) * 2);
                        bq[tg][2 * eh] = v.x;
                        bq[tg][2 * eh + 1] = v.y;
                    }
#pragma unroll
                for (int el = 0; el < 2 * EH; ++el) {
                    const int e = 2 * eh0 + el;
#pragma unroll
                    for (int pr = 0; pr < NP; ++pr) {
                        const double2 a = op2[(e * NP + pr) * 64];
#pragma unroll
                        for (int tg = 0; tg < 4; ++tg) {
                            acc[tg][2 * pr] = __builtin_amdgcn_mfma_f64_4x4x4f64(a.x, bq[tg][el], acc[tg][2 * pr], 0, 0, 0);
                            acc[tg][2 * pr + 1] =
                                __builtin_amdgcn_mfma_f64_4x4x4f64(a.y, bq[tg][el], acc[tg][2 * pr + 1], 0, 0, 0);
                        }
                    }
                    if (NS) {
                        const double a = op[4 * NP * 128 + e * 64];
#pragma unroll
                        for (int tg = 0; tg < 4; ++tg)
                            acc[tg][NG16 - 1] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, bq[tg][el], acc[tg][NG16 - 1], 0, 0, 0);
                    }
                }
            }
        }
        if (++qcnt == nq) { // a column block is complete: write it out, start the next one
            qcnt = 0;
            const int col0 = zb * BLK + 16 * g16;
            ++zb;
            bool two_dst = false; // PAIRS: the block holds pairs (wave-uniform)
            if constexpr (PAIRS) {
              if (wave_live) {
                // As below with two destinations per column: a + b to the slot of V + t, a - b to that of V + Rt.
                double *cb = out + (int64_t)kr * out_len;
                double *dump = cb + (out_len - 128) + 2 * lane;
                const int32_t *auxb = aux + ((zb - 1 - zb0) & 1) * AUX;
                two_dst = (__builtin_amdgcn_readfirstlane(auxb[16 * NG16]) & kM2lBlkTwoDst) != 0;
                int pk[NP + NS], pk2[NP + NS];
#pragma unroll
                for (int pr = 0; pr < NP + NS; ++pr) {
                    pk[pr] = auxb[pr < NP ? 32 * pr + 2 * (4 * db + di) : 32 * NP + 4 * db + di]; // the even column of a pair of columns
                    pk2[pr] = two_dst ? auxb[192 + (pr < NP ? 32 * pr + 2 * (4 * db + di) : 32 * NP + 4 * db + di)] : -1;
                }
#pragma unroll
                for (int tg = 0; tg < 4; ++tg) {
                    const bool spv = wave * 16 + 4 * tg + dj < tile.count;
                    const int32_t *srow = slds + (4 * tg + dj) * slot_t;
#pragma unroll
                    for (int pr = 0; pr < NP + NS; ++pr) {
                        const bool single = NS && pr == NP;
                        const int g0 = single ? NG16 - 1 : 2 * pr, g1 = single ? NG16 - 1 : 2 * pr + 1;
                        const int sl = srow[max(pk[pr] >> 24, 0)];
                        const int okm = (spv ? -1 : 0) & ~(pk[pr] | sl); // sign bit set: valid cell, row, slot
                        double *dst = okm < 0 ? cb + (int64_t)sl * 2 + (pk[pr] & 0xffffff) : dump;
                        if (single) *dst = acc_e[tg][g0] + acc[tg][g0];
                        else *reinterpret_cast<double2 *>(dst) = make_double2(acc_e[tg][g0] + acc[tg][g0], acc_e[tg][g1] + acc[tg][g1]);
                        if (two_dst) {
                            const int sl2 = srow[max(pk2[pr] >> 24, 0)];
                            const int okm2 = (spv ? -1 : 0) & ~(pk2[pr] | sl2);
                            double *dst2 = okm2 < 0 ? cb + (int64_t)sl2 * 2 + (pk2[pr] & 0xffffff) : dump;
                            if (single) *dst2 = acc_e[tg][g0] - acc[tg][g0];
                            else *reinterpret_cast<double2 *>(dst2) = make_double2(acc_e[tg][g0] - acc[tg][g0], acc_e[tg][g1] - acc[tg][g1]);
                        }
                    }
                    // (both accumulator sets are live here: keep the slot lookups of the next cell group from being
                    // hoisted above this group's stores, which would spill)
                    __builtin_amdgcn_sched_barrier(0);
                }
              }
            } else if (STAGE == 1 && wave_live) {
                // Scatter into the target slots, branch-free: entries without a destination (padding
                // rows, absent targets, cells beyond the tile) go to a dump area behind the slot buffer.
                // Measured: the epilogue is store-issue bound (about 75 cycles per store instruction
                // and CU whatever its width, the address pattern or the wait after it): adjacent
                // column pairs leave as 16-byte stores, half the instructions of 8-byte ones.
                double *cb = out + (int64_t)kr * out_len;
                double *dump = cb + (out_len - 128) + 2 * lane; // 16-byte aligned (out_len is even)
                const int32_t *auxb = aux + ((zb - 1 - zb0) & 1) * AUX;
                int pk[NP + NS];
#pragma unroll
                for (int pr = 0; pr < NP; ++pr) pk[pr] = auxb[32 * pr + 2 * (4 * db + di)]; // the even column
                if (NS) pk[NP] = auxb[32 * NP + 4 * db + di];
#pragma unroll
                for (int tg = 0; tg < 4; ++tg) {
                    const bool spv = wave * 16 + 4 * tg + dj < tile.count;
                    const int32_t *srow = slds + (4 * tg + dj) * slot_t;
#pragma unroll
                    for (int pr = 0; pr < NP; ++pr) {
                        const int sl = srow[max(pk[pr] >> 24, 0)];
                        const int okm = (spv ? -1 : 0) & ~(pk[pr] | sl); // sign bit set: valid cell, row, slot
                        double *dst = okm < 0 ? cb + (int64_t)sl * 2 + (pk[pr] & 0xffffff) : dump;
                        *reinterpret_cast<double2 *>(dst) = make_double2(acc[tg][2 * pr], acc[tg][2 * pr + 1]);
                    }
                    if (NS) {
                        const int sl = srow[max(pk[NP] >> 24, 0)];
                        const int okm = (spv ? -1 : 0) & ~(pk[NP] | sl);
                        double *dst = okm < 0 ? cb + (int64_t)sl * 2 + (pk[NP] & 0xffffff) : dump;
                        *dst = acc[tg][NG16 - 1];
                    }
                }
            } else if (STAGE >= 2) {
#pragma unroll
                for (int tg = 0; tg < 4; ++tg) {
                    const int tp = wave * 16 + 4 * tg + dj;
                    if (tp < tile.count) {
                        const int cell = cls.cells[cell_p(tp)];
                        double *Lc = out + ((int64_t)kr * C + cell) * n_pad + col0;
                        if (ksplit > 1) { // one of several parts of the contraction
#pragma unroll
                            for (int pr = 0; pr < NP; ++pr) {
                                unsafeAtomicAdd(Lc + 32 * pr + 2 * (4 * db + di), acc[tg][2 * pr]);
                                unsafeAtomicAdd(Lc + 32 * pr + 2 * (4 * db + di) + 1, acc[tg][2 * pr + 1]);
                            }
                            if (NS) unsafeAtomicAdd(Lc + 32 * NP + 4 * db + di, acc[tg][NG16 - 1]);
                        } else {
#pragma unroll
                            for (int pr = 0; pr < NP; ++pr)
                                *reinterpret_cast<double2 *>(Lc + 32 * pr + 2 * (4 * db + di)) =
                                    make_double2(acc[tg][2 * pr], acc[tg][2 * pr + 1]);
                            if (NS) Lc[32 * NP + 4 * db + di] = acc[tg][NG16 - 1];
                        }
                    }
                }
            }
#pragma unroll
            for (int tg = 0; tg < 4; ++tg)
#pragma unroll
                for (int g = 0; g < NG16; ++g) acc[tg][g] = 0.0;
            // the 4 * (NP + NS) scatter stores issued after this step's DMA drain under the next block
            // (a wave without cells stored nothing: it waits for its DMA as usual)
            if (STAGE == 1) {
                if (wave_live && two_dst) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 * (NP + NS) < 63 ? 8 * (NP + NS) : 63) : "memory");
                else if (wave_live) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (NP + NS) < 63 ? 4 * (NP + NS) : 63) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                continue;
            }
        }
        wait_dma_and_barrier();
    }
}

template <int NG16, int STAGE, int MINW, bool PAIRS = false>
static void m2l_gemm_launch(const M2lClass *classes, const M2lTileDesc *tiles, int n_tiles, int n_pad, int g16_0,
                            int n_colblocks, int K, int64_t C, const double *in, int64_t in_len, double *out,
                            int64_t out_len, const uint16_t *qlist, int slot_t, const int32_t *tile_idx, hipStream_t s) {
    const size_t lds = 2 * sizeof(double) * (size_t)(2 * NG16 * 128 + 2048) + (STAGE == 1 ? (size_t)(2 * (PAIRS ? 384 : 192) + 128 + 8 * 16 * (slot_t & 0xffff)) * 4 : 0); // + aux, cell and slot tables
    // one flag word per template instance; a refused attribute shows up as the failed launch
    static std::atomic<uint64_t> attr_set[4] = {{0}, {0}, {0}, {0}};
    (void)allow_large_dynamic_lds(reinterpret_cast<const void *>(&m2l_gemm_k4<NG16, STAGE, MINW, PAIRS>), lds, attr_set);
    const int zdim = STAGE == 2 && slot_t > 1 ? n_colblocks * slot_t : n_colblocks; // stage 2: slot_t = parts of the contraction
    hipLaunchKernelGGL((m2l_gemm_k4<NG16, STAGE, MINW, PAIRS>), dim3(n_tiles, K, zdim), dim3(512), lds, s, classes,
                       tiles, n_pad, g16_0, C, in, in_len, out, out_len, qlist, slot_t, tile_idx);
}

// Column-chunk plan: 16-column groups per workgroup.  Stage 1 walks column blocks of kM2lS1Block =
// 11 groups (44 accumulators per lane; 22 spills in the persistent walk).  Stage 2 covers the n_pad
// output nodes with 22-group chunks (88 accumulators, one workgroup per CU), measured faster there
// than 11 or 8.

template <int STAGE> constexpr int m2l_chunk_pref() { return STAGE == 1 ? kM2lS1Block / 16 : 22; }
constexpr int kM2lS2KsplitFill = 4; // workgroups per CU up to which stage 2 keeps splitting the contraction

template <int STAGE>
static void m2l_dispatch_chunks(int total_groups, const M2lClass *classes, const M2lTileDesc *tiles, int n_tiles,
                                int n_pad, int n_colblocks, int K, int64_t C, const double *in, int64_t in_len,
                                double *out, int64_t out_len, const uint16_t *qlist, int slot_t,
                                const int32_t *tile_idx, hipStream_t s) {
    int done = 0;
    const int pref = m2l_chunk_pref<STAGE>();
    while (done < total_groups) {
        const int left = total_groups - done;
        int take;
#define M2L_GO(NG, MW)                                                                                              \
    {                                                                                                               \
        take = NG;                                                                                                  \
        m2l_gemm_launch<NG, STAGE, MW>(classes, tiles, n_tiles, n_pad, done,                                        \
                                       STAGE >= 2 ? 1 : n_colblocks, K, C, in, in_len,                            \
                                       out, out_len, qlist, slot_t, tile_idx, s);                                   \
    }
        if (STAGE >= 2 && !(n_colblocks == 1 && left >= 16)) { // (one workgroup per tile and a wide chunk: the plan below)
            // stage 2 / 3 with several workgroups per tile (gridDim.z = zc): the largest NG x zc <= left from the
            // kernels without spills, at most 2 x 11 or 3 x (8, 7, 6, 4, 2) -- 22 = 2 x 11, 46 = 3 x 8 + 2 x 11,
            // 18 = 3 x 6, 16 = 2 x 8, 7 = 1 x 7
            int best_ng = 2, best_z = 1;
            for (int ng : {11, 8, 7, 6, 4, 2})
                for (int zc = 1; zc <= (n_colblocks == 1 ? 1 : ng == 11 ? 2 : 3); ++zc)
                    if (ng * zc <= left && ((left - ng * zc) % 2 == 0 || left - ng * zc == 7) && // what remains must be coverable
                        (ng * zc > best_ng * best_z || (ng * zc == best_ng * best_z && ng > best_ng))) {
                        best_ng = ng;
                        best_z = zc;
                    }
            take = best_ng * best_z;
#define M2L_ZGO(NG, MW)                                                                                             \
    m2l_gemm_launch<NG, STAGE, MW>(classes, tiles, n_tiles, n_pad, done, best_z, K, C, in, in_len, out, out_len,    \
                                   qlist, slot_t, tile_idx, s);
            if constexpr (STAGE >= 2) {
                switch (best_ng) {
                case 11: M2L_ZGO(11, 1) break;
                case 8: M2L_ZGO(8, 4) break;
                case 7: M2L_ZGO(7, 2) break;
                case 6: M2L_ZGO(6, 4) break;
                case 4: M2L_ZGO(4, 4) break;
                default: M2L_ZGO(2, 4) break;
                }
            }
#undef M2L_ZGO
        } else if (pref == 22 && left >= 22) M2L_GO(22, 1)
        else if (pref == 22 && left >= 16) M2L_GO(16, 1)
        else if (pref == 11 && left >= 11) M2L_GO(11, 1)
        else if (left >= 8) M2L_GO(8, 4)
        else if (left >= 6) M2L_GO(6, 4)
        else if (left >= 4) M2L_GO(4, 4)
        else M2L_GO(2, 4)
#undef M2L_GO
        done += take;
    }
}

// Stage 1: every class's stacked operator is padded to a whole number of kM2lS1Block columns;
// blockIdx.z walks the column blocks, the chunk plan splits a block.
void launch_m2l_stage1(const M2lClass *classes, const M2lTileDesc *tiles, const int32_t *tile_idx, int n_tiles,
                       int n_pad, int max_slot_t, int K, int64_t C, const double *M, double *cbuf, int64_t cbuf_len,
                       hipStream_t s, bool own_blocks, int max_blocks, int ne16, int s_ee, int s_eo) {
    if (n_tiles == 0) return;
    int slot_t = 16; // LDS slot-table width: power of two covering the transfer vectors of any block
    while (slot_t < max_slot_t) slot_t *= 2;
    // every workgroup walks its share of the column blocks; splitting the walk over gridDim.z
    // workgroups shortens the last, partially filled round of the launch
    const int n_cu = device_cu_count();
    // One workgroup per CU at a time: n_tiles * z workgroups take ceil(n_tiles * z / CUs) rounds of 1/z of the
    // column-block walk each; z is chosen so that the last, partially filled round is short (a per-workgroup
    // overhead of about half a percent of a walk keeps z small).  Measured at 10M points (2,336 tiles): z = 2 18.2 ms,
    // 3 18.0, 4 17.75, 7 18.0, 13 18.3.
    // A launch that does not fill the chip even at z = 8 (a small tree: 16 tiles at 36k points, where a workgroup's walk of
    // four column blocks WAS the stage: 0.155 ms of a 0.46 ms matvec) may split the walk down to one block per workgroup.
    const int zmax = n_tiles * 8 < n_cu ? std::max(8, std::min(max_blocks, 32)) : 8;
    int zsplit = 1;
    double best = 1e300;
    for (int z = 1; z <= zmax; ++z) {
        const double rounds = std::ceil(static_cast<double>(n_tiles) * z / n_cu);
        const double cost = rounds / z * (1.0 + 0.005 * z);
        if (cost < best - 1e-12) {
            best = cost;
            zsplit = z;
        }
    }
    const int n_colblocks = own_blocks ? 1 : zsplit; // tiles that name their own blocks are not split further
    if (ne16 > 0) { // parity basis: one instance, a whole column block per walk step (in_len carries the even part's length
        // and, for two axes, the steps of the parts ee and eo)
        const int64_t packed = static_cast<int64_t>(ne16) | (static_cast<int64_t>(s_ee & 0xffff) << 32) | (static_cast<int64_t>(s_eo & 0x7fff) << 48);
        m2l_gemm_launch<kM2lS1BlockPairs / 16, 1, 1, true>(classes, tiles, n_tiles, n_pad, 0, n_colblocks, K, C, M, packed, cbuf, cbuf_len,
                                                      nullptr, slot_t, tile_idx, s);
        return;
    }
    m2l_dispatch_chunks<1>(kM2lS1Block / 16, classes, tiles, n_tiles, n_pad, n_colblocks, K, C, M, 0, cbuf, cbuf_len, nullptr,
                           slot_t, tile_idx, s);
}

// Parts of stage 2's contraction for a launch of `wgs` workgroups (the rule of launch_m2l_stage2's comment, shared by the
// node-basis and the parity-basis launch): 1 when the launch fills the chip or the handle is deterministic (the parts add
// atomically), else the cheapest of 1..16 by ceil(workgroups * parts / CUs) * (0.05 + 1 / parts).  BBFMM_M2L_S2_KSPLIT overrides.
static int m2l_s2_ksplit(int64_t wgs, bool allow_ksplit) {
    static const int ks_env = [] {
        const int v = env_int("BBFMM_M2L_S2_KSPLIT", 0);
        return v >= 1 && v <= 32 ? v : 0;
    }();
    if (!allow_ksplit) return 1;
    if (ks_env > 0) return ks_env;
    const int n_cu = device_cu_count();
    int ksplit = 1;
    if (wgs * 2 <= static_cast<int64_t>(kM2lS2KsplitFill) * n_cu) { // (launches of at most two workgroups per CU)
        double best = 1e300;
        for (int ks = 1; ks <= 16; ++ks) {
            const double cost = std::ceil(static_cast<double>(wgs * ks) / n_cu) * (0.05 + 1.0 / ks);
            if (cost < best - 1e-12) {
                best = cost;
                ksplit = ks;
            }
        }
    }
    return ksplit;
}

// Stage 2: the output nodes (n_pad, in groups of 16; n_pad is a multiple of 32) in column chunks.
void launch_m2l_stage2(const M2lClass *classes, const M2lTileDesc *tiles, const int32_t *tile_idx, int n_tiles,
                       int n_pad, int K, int64_t C, const double *cbuf, int64_t cbuf_len, const uint16_t *qlist,
                       double *L, hipStream_t s, bool allow_ksplit) {
    if (n_tiles == 0) return;
    // Two workgroups per tile, each with half of a 22-group chunk of the output nodes (gridDim.z = 2, 11 groups,
    // 78 KB of LDS: two fit a CU).  The halves of a tile read the same slot contents at about the same time (L2
    // hits) and twice as many, shorter workgroups balance tiles of unequal length (per-tile active steps) and fill
    // the CUs of launches with few tiles.  Measured, stage 2 per matvec: 10M points 16.2 -> 15.8 ms, p = 9 55.1 ->
    // 53.6 (52.5 with the remainder as 3 x 8 instead of 22 + 2), 1M points (about 200 tiles) 2.10 -> 1.54 and 1.12 -> 0.71,
    // one rank of an 8-way partition 2.81 -> 2.28.  (Two separate launches of 11 groups were slower than one of 22.)
    // BBFMM_M2L_S2_ZSPLIT=1 turns it off.
    static const int z = env_int("BBFMM_M2L_S2_ZSPLIT", 2) == 1 ? 1 : 2;
    // Few tiles (a small tree, a thin slice of a partition): also split the contraction, so that no workgroup walks a
    // tile's chain of ~290 dependent steps alone.  The parts add to L (zeroed by the caller before every downward pass) with
    // f64 atomics; launches that fill the chip keep plain stores.
    // Stage 2 per matvec: 50k points 0.50 -> 0.11 ms (the whole matvec 0.79 -> 0.39 ms), 200k 0.52 -> 0.43, 1M 0.95 -> 0.78;
    // from 3M points on the launch fills the chip and nothing changes.  BBFMM_M2L_S2_KSPLIT=<n> overrides (1: off).
    // Round 6: the number of parts from what was measured instead of a power of two -- a CU works its workgroups off one after
    // the other (two resident ones share its matrix pipe), a part costs a fixed 4-5 % of a whole chain plus its share of it,
    // so the launch takes ceil(workgroups * parts / CUs) * (0.05 + 1 / parts) chains: 585 cells (32 workgroups) 16 -> 8 parts,
    // 0.105 -> 0.085 ms; 4,681 cells (158 workgroups) 4 -> 3 parts, 0.419 -> 0.368 ms (5 parts: 0.462, 8: 0.411, 2: 0.511).
    const int ksplit = m2l_s2_ksplit(static_cast<int64_t>(n_tiles) * z * K, allow_ksplit);
    m2l_dispatch_chunks<2>(n_pad / 16, classes, tiles, n_tiles, n_pad, z, K, C, cbuf, cbuf_len, L, 0, qlist, ksplit > 1 ? ksplit : 0, tile_idx, s);
}

// ------------------------------------------------------------------ stage 2 in the parity basis of the x reflection
// The slot of a target is [A | B | S] (M2lClass::kp): for a pair (t, Rt) the leader's segment x lies in A and the partner's
// segment y at the same offset in B; the operator is [U_e | pad | U_o | pad] with one set of rows per pair.  A workgroup
// takes a chunk of column groups that lies wholly in the even or wholly in the odd half.  Step q of the operator's rows
// brings the 16 slot values at kp + 16 q by DMA and, for a pair step (16 q < kp), the 16 at 16 q into a second IN tile;
// every lane forms x + y (even half) or x - y (odd half) from LDS before the MFMAs.  A singles step multiplies the one
// tile as m2l_gemm_k4 does.  The operator image, the IN tile layout, the MFMA loop and the epilogue are those of
// m2l_gemm_k4's stage 2 (its comments apply); OUT is Lp with n_par values per cell.
// Two axes (Y < NG16): the chunk is [Y groups that are even along y | NG16 - Y groups that are odd along y] and the pair
// steps from kpy / 16 on hold y pairs (t, R_y t): every lane forms x + y AND x - y and feeds the first Y groups from the
// one set, the others from the other set, in either x half.  The boundary Y is fixed per instance, the kind of a step is
// wave-uniform; x-pair steps and singles steps use one set for all groups as before.
template <int NG16, int Y = NG16>
__device__ __forceinline__ void m2l_s2_pairs_body(const M2lClass &cls, const M2lTileDesc &tile, int n_par, int g16, bool odd,
                                                  int zk, int ksplit, int64_t C, const double *__restrict__ in, int64_t in_len,
                                                  double *__restrict__ out, const uint16_t *__restrict__ qlist,
                                                  const int32_t *__restrict__ tile_idx, double *lds) {
    const int kr = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ld = n_par;
    const int q_lo = tile.q_count * zk / ksplit;
    const int nq = tile.q_count * (zk + 1) / ksplit - q_lo;
    const uint16_t *ql = qlist + tile.q_first + q_lo;
    const int kp = cls.kp, kp16 = kp >> 4;
    const int kpy16 = Y < NG16 ? cls.kpy >> 4 : kp16; // first step of the y pairs
    const double *opbase = cls.u_all + 16 * g16;

    constexpr int OP_CHUNKS = 2 * NG16;
    constexpr int NCH = (OP_CHUNKS + 7) / 8;
    constexpr int OP_DOUBLES = OP_CHUNKS * 128;
    constexpr int BUF = OP_DOUBLES + 4096; // the operator tile, the x tile (pair steps), the y / singles tile
    constexpr int NP = NG16 / 2, NS = NG16 & 1;
    unsigned voff[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = wave + 8 * i;
        if (c < 4 * NP) {
            const int e = c / (NP > 0 ? NP : 1), pr = c - e * NP, k = lane >> 4, p = lane & 15;
            voff[i] = (unsigned)(((4 * k + e) * ld + 32 * pr + 2 * p) * 8);
        } else {
            const int e = 2 * (c - 4 * NP) + (lane >> 5), r = lane & 31, k = r >> 3, pair = r & 7;
            voff[i] = (unsigned)(((4 * k + e) * ld + 32 * NP + 2 * pair) * 8);
        }
    }
    auto cell_p = [&](int pos) {
        const int q = pos < tile.count ? pos : 0;
        return tile.pad ? tile_idx[tile.first + q] : tile.first + q;
    };
    const double *cptr[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int tg = 2 * h + (lane >> 5), eh = (lane >> 4) & 1, k = (lane >> 2) & 3, j = lane & 3;
        const int p = cell_p(wave * 16 + 4 * tg + j);
        cptr[h] = in + (int64_t)kr * in_len + cls.cbase[p] + 4 * k + 2 * eh;
    }
    const unsigned lds0 = lds_offset(lds);
    const int64_t qstride = (int64_t)16 * ld;
    auto stage = [&](int qi, int buf) { // returns the kind of the step (wave-uniform): 0 singles, 1 x pairs, 2 y pairs
        const int q = (int)uniform_u32(ql[qi]);
#pragma unroll
        for (int i = 0; i < NCH; ++i)
            if (wave + 8 * i < OP_CHUNKS)
                dma16s(opbase + q * qstride, voff[i], lds0 + (unsigned)(buf * BUF + (wave + 8 * i) * 128) * 8u);
#pragma unroll
        for (int h = 0; h < 2; ++h)
            dma16(cptr[h] + kp + 16 * q, lds0 + (unsigned)(buf * BUF + OP_DOUBLES + 2048 + (2 * wave + h) * 128) * 8u);
        if (q < kp16) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                dma16(cptr[h] + 16 * q, lds0 + (unsigned)(buf * BUF + OP_DOUBLES + (2 * wave + h) * 128) * 8u);
        }
        if constexpr (Y < NG16) return q < kpy16 ? 1 : q < kp16 ? 2 : 0;
        else return q < kp16; // (one axis: whether the step is a pair step)
    };
    using StepKind = std::conditional_t<(Y < NG16), int, bool>;

    double acc[4][NG16];
#pragma unroll
    for (int tg = 0; tg < 4; ++tg)
#pragma unroll
        for (int g = 0; g < NG16; ++g) acc[tg][g] = 0.0;

    const int bk = lane >> 4, bj = lane & 3;
    const bool wave_live = wave * 16 < tile.count;
    const int di = lane >> 4, db = (lane >> 2) & 3, dj = lane & 3;
    const double sgn = odd ? -1.0 : 1.0;
    StepKind pair_cur{};
    if (nq > 0) pair_cur = stage(0, 0);
    wait_dma_and_barrier();
    auto grp = [](auto &bs, auto &bd, int g) -> auto & { return g < Y ? bs : bd; }; // (g is a constant after unrolling)
    for (int sidx = 0; sidx < nq; ++sidx) {
        const double *op = lds + (sidx & 1) * BUF + lane;
        const double2 *op2 = reinterpret_cast<const double2 *>(lds + (sidx & 1) * BUF) + lane;
        const double *cx = lds + (sidx & 1) * BUF + OP_DOUBLES + wave * 256 + (bk * 4 + bj) * 2;
        StepKind pair_next{};
        if (sidx + 1 < nq) pair_next = stage(sidx + 1, (sidx + 1) & 1); // streams in under the MFMAs below
        if (wave_live) {
            double bq[4][4], bd[4][4]; // bd: the set of the y-odd groups (two axes only)
#pragma unroll
            for (int tg = 0; tg < 4; ++tg)
#pragma unroll
                for (int eh = 0; eh < 2; ++eh) {
                    const double2 y = *reinterpret_cast<const double2 *>(cx + 2048 + ((tg * 2 + eh) * 16) * 2);
                    bq[tg][2 * eh] = y.x;
                    bq[tg][2 * eh + 1] = y.y;
                }
            if (pair_cur == StepKind(1)) { // x + y for the even half, x - y for the odd half (sgn * y is exact)
#pragma unroll
                for (int tg = 0; tg < 4; ++tg)
#pragma unroll
                    for (int eh = 0; eh < 2; ++eh) {
                        const double2 x = *reinterpret_cast<const double2 *>(cx + ((tg * 2 + eh) * 16) * 2);
                        bq[tg][2 * eh] = x.x + sgn * bq[tg][2 * eh];
                        bq[tg][2 * eh + 1] = x.y + sgn * bq[tg][2 * eh + 1];
                    }
            }
            if constexpr (Y < NG16) {
                if (pair_cur == 2) { // a y pair: x + y for the y-even groups, x - y for the y-odd groups, in both x halves
#pragma unroll
                    for (int tg = 0; tg < 4; ++tg)
#pragma unroll
                        for (int eh = 0; eh < 2; ++eh) {
                            const double2 x = *reinterpret_cast<const double2 *>(cx + ((tg * 2 + eh) * 16) * 2);
                            const double y0 = bq[tg][2 * eh], y1 = bq[tg][2 * eh + 1];
                            bq[tg][2 * eh] = x.x + y0;
                            bq[tg][2 * eh + 1] = x.y + y1;
                            bd[tg][2 * eh] = x.x - y0;
                            bd[tg][2 * eh + 1] = x.y - y1;
                        }
                } else {
#pragma unroll
                    for (int tg = 0; tg < 4; ++tg)
#pragma unroll
                        for (int e = 0; e < 4; ++e) bd[tg][e] = bq[tg][e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int pr = 0; pr < NP; ++pr) {
                    const double2 a = op2[(e * NP + pr) * 64];
#pragma unroll
                    for (int tg = 0; tg < 4; ++tg) {
                        acc[tg][2 * pr] = __builtin_amdgcn_mfma_f64_4x4x4f64(a.x, grp(bq, bd, 2 * pr)[tg][e], acc[tg][2 * pr], 0, 0, 0);
                        acc[tg][2 * pr + 1] = __builtin_amdgcn_mfma_f64_4x4x4f64(a.y, grp(bq, bd, 2 * pr + 1)[tg][e], acc[tg][2 * pr + 1], 0, 0, 0);
                    }
                }
                if (NS) {
                    const double a = op[4 * NP * 128 + e * 64];
#pragma unroll
                    for (int tg = 0; tg < 4; ++tg)
                        acc[tg][NG16 - 1] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, grp(bq, bd, NG16 - 1)[tg][e], acc[tg][NG16 - 1], 0, 0, 0);
                }
            }
        }
        pair_cur = pair_next;
        wait_dma_and_barrier();
    }
    const int col0 = 16 * g16;
#pragma unroll
    for (int tg = 0; tg < 4; ++tg) {
        const int tp = wave * 16 + 4 * tg + dj;
        if (tp < tile.count) {
            const int cell = cls.cells[cell_p(tp)];
            double *Lc = out + ((int64_t)kr * C + cell) * n_par + col0;
            if (ksplit > 1) { // one of several parts of the contraction
#pragma unroll
                for (int pr = 0; pr < NP; ++pr) {
                    unsafeAtomicAdd(Lc + 32 * pr + 2 * (4 * db + di), acc[tg][2 * pr]);
                    unsafeAtomicAdd(Lc + 32 * pr + 2 * (4 * db + di) + 1, acc[tg][2 * pr + 1]);
                }
                if (NS) unsafeAtomicAdd(Lc + 32 * NP + 4 * db + di, acc[tg][NG16 - 1]);
            } else {
#pragma unroll
                for (int pr = 0; pr < NP; ++pr)
                    *reinterpret_cast<double2 *>(Lc + 32 * pr + 2 * (4 * db + di)) = make_double2(acc[tg][2 * pr], acc[tg][2 * pr + 1]);
                if (NS) Lc[32 * NP + 4 * db + di] = acc[tg][NG16 - 1];
            }
        }
    }
}

// One launch for both halves: blockIdx.z = part of the contraction * (ce + co) + chunk; the first ce chunks are GA groups
// of the even half, the other co chunks GB groups of the odd half (two launches of one width each were measured slower
// than one launch in the node basis: the halves of a tile read the same slot contents at about the same time).
template <int GA, int GB>
__global__ __launch_bounds__(512, 1) void m2l_s2_pairs_kernel(const M2lClass *__restrict__ classes, const M2lTileDesc *__restrict__ tiles,
                                                              int n_par, int ce, int co, int ksplit, int64_t C,
                                                              const double *__restrict__ in, int64_t in_len, double *__restrict__ out,
                                                              const uint16_t *__restrict__ qlist, const int32_t *__restrict__ tile_idx) {
    extern __shared__ double lds[];
    const M2lTileDesc tile = tiles[blockIdx.x];
    const M2lClass cls = classes[tile.level_class];
    const int zcols = ce + co;
    const int zk = (int)blockIdx.z / zcols, zc = (int)blockIdx.z - zk * zcols;
    if (zc < ce) m2l_s2_pairs_body<GA>(cls, tile, n_par, zc * GA, false, zk, ksplit, C, in, in_len, out, qlist, tile_idx, lds);
    else m2l_s2_pairs_body<GB>(cls, tile, n_par, ce * GA + (zc - ce) * GB, true, zk, ksplit, C, in, in_len, out, qlist, tile_idx, lds);
}

// Two axes: a chunk of the x-even half is [YA groups of ee | GA - YA of eo], one of the x-odd half [YB of oe | GB - YB of oo].
template <int GA, int YA, int GB, int YB>
__global__ __launch_bounds__(512, 1) void m2l_s2_pairs2_kernel(const M2lClass *__restrict__ classes, const M2lTileDesc *__restrict__ tiles,
                                                               int n_par, int ce, int co, int ksplit, int64_t C,
                                                               const double *__restrict__ in, int64_t in_len, double *__restrict__ out,
                                                               const uint16_t *__restrict__ qlist, const int32_t *__restrict__ tile_idx) {
    extern __shared__ double lds[];
    const M2lTileDesc tile = tiles[blockIdx.x];
    const M2lClass cls = classes[tile.level_class];
    const int zcols = ce + co;
    const int zk = (int)blockIdx.z / zcols, zc = (int)blockIdx.z - zk * zcols;
    if (zc < ce) m2l_s2_pairs_body<GA, YA>(cls, tile, n_par, zc * GA, false, zk, ksplit, C, in, in_len, out, qlist, tile_idx, lds);
    else m2l_s2_pairs_body<GB, YB>(cls, tile, n_par, ce * GA + (zc - ce) * GB, true, zk, ksplit, C, in, in_len, out, qlist, tile_idx, lds);
}

// The chunk widths the kernel is instantiated for, (even, odd): 3-D order 7 has 13 + 10 groups, order 9 26 + 21, order 5
// 5 + 4; the equal widths serve the other orders.  A half is padded to a whole number of chunks (zero operator columns).
// The planner's table and the launcher's dispatch are both generated from this list.
#define M2L_S2_PAIR_WIDTHS(X) X(13, 10) X(13, 11) X(8, 8) X(7, 7) X(5, 4) X(4, 4) X(2, 2) X(1, 1)
#define M2L_S2_WIDTH_ENTRY(A, B) {A, B},
static constexpr int kM2lS2PairWidths[][2] = {M2L_S2_PAIR_WIDTHS(M2L_S2_WIDTH_ENTRY)};
#undef M2L_S2_WIDTH_ENTRY

// Fewest executed column groups, a chunk counted two groups dearer than its width (its share of the IN tiles and barriers).
M2lS2PairsPlan m2l_s2_pairs_plan(int groups_even, int groups_odd) {
    M2lS2PairsPlan best{1, 1, std::max(groups_even, 1), std::max(groups_odd, 1)};
    int best_cost = 1 << 30;
    for (const auto &w : kM2lS2PairWidths) {
        const int ce = std::max(1, (groups_even + w[0] - 1) / w[0]), co = std::max(1, (groups_odd + w[1] - 1) / w[1]);
        const int cost = ce * (w[0] + 2) + co * (w[1] + 2);
        if (cost < best_cost) {
            best_cost = cost;
            best = M2lS2PairsPlan{w[0], w[1], ce, co};
        }
    }
    return best;
}

// Two axes, (GA, YA, GB, YB): 3-D order 7 has 7 + 6 and 6 + 4 groups, order 9 15 + 12 and 12 + 9 (two chunks of 8 + 6 and of
// 6 + 5), order 5 3 + 2 and 2 + 2; (2, 1, 2, 1) serves any order with one chunk per group of the longer part.  Planner and
// dispatch are generated from this list, as above.
#define M2L_S2_PAIR2_WIDTHS(X) X(13, 7, 10, 6) X(14, 8, 11, 6) X(8, 4, 8, 4) X(5, 3, 4, 2) X(4, 2, 4, 2) X(2, 1, 2, 1)
#define M2L_S2_WIDTH2_ENTRY(A, YA, B, YB) {A, YA, B, YB},
static constexpr int kM2lS2Pair2Widths[][4] = {M2L_S2_PAIR2_WIDTHS(M2L_S2_WIDTH2_ENTRY)};
#undef M2L_S2_WIDTH2_ENTRY

M2lS2PairsPlan m2l_s2_pairs_plan2(const int groups[4]) {
    M2lS2PairsPlan best{2, 2, 1, 1, 1, 1};
    int best_cost = 1 << 30;
    auto chunks = [](int n, int w) { return std::max(1, (n + w - 1) / w); };
    for (const auto &w : kM2lS2Pair2Widths) {
        const int ce = std::max(chunks(groups[0], w[1]), chunks(groups[1], w[0] - w[1]));
        const int co = std::max(chunks(groups[2], w[3]), chunks(groups[3], w[2] - w[3]));
        const int cost = ce * (w[0] + 2) + co * (w[2] + 2);
        if (cost < best_cost) {
            best_cost = cost;
            best = M2lS2PairsPlan{w[0], w[2], ce, co, w[1], w[3]};
        }
    }
    return best;
}

template <int GA, int YA, int GB, int YB>
static void m2l_s2_pairs2_launch(const M2lClass *classes, const M2lTileDesc *tiles, const int32_t *tile_idx, int n_tiles,
                                 const M2lS2PairsPlan &plan, int ksplit, int K, int64_t C, const double *cbuf, int64_t cbuf_len,
                                 const uint16_t *qlist, double *Lp, hipStream_t s) {
    const size_t lds = 2 * sizeof(double) * (size_t)(2 * (GA > GB ? GA : GB) * 128 + 4096);
    static std::atomic<uint64_t> attr_set[4] = {{0}, {0}, {0}, {0}};
    (void)allow_large_dynamic_lds(reinterpret_cast<const void *>(&m2l_s2_pairs2_kernel<GA, YA, GB, YB>), lds, attr_set);
    hipLaunchKernelGGL((m2l_s2_pairs2_kernel<GA, YA, GB, YB>), dim3(n_tiles, K, (plan.ce + plan.co) * ksplit), dim3(512), lds, s, classes,
                       tiles, plan.n_par(), plan.ce, plan.co, ksplit, C, cbuf, cbuf_len, Lp, qlist, tile_idx);
}

template <int GA, int GB>
static void m2l_s2_pairs_launch(const M2lClass *classes, const M2lTileDesc *tiles, const int32_t *tile_idx, int n_tiles,
                                const M2lS2PairsPlan &plan, int ksplit, int K, int64_t C, const double *cbuf, int64_t cbuf_len,
                                const uint16_t *qlist, double *Lp, hipStream_t s) {
    const size_t lds = 2 * sizeof(double) * (size_t)(2 * (GA > GB ? GA : GB) * 128 + 4096);
    static std::atomic<uint64_t> attr_set[4] = {{0}, {0}, {0}, {0}};
    (void)allow_large_dynamic_lds(reinterpret_cast<const void *>(&m2l_s2_pairs_kernel<GA, GB>), lds, attr_set);
    hipLaunchKernelGGL((m2l_s2_pairs_kernel<GA, GB>), dim3(n_tiles, K, (plan.ce + plan.co) * ksplit), dim3(512), lds, s, classes, tiles,
                       plan.n_par(), plan.ce, plan.co, ksplit, C, cbuf, cbuf_len, Lp, qlist, tile_idx);
}

int m2l_s2_pairs_ksplit(int n_tiles, const M2lS2PairsPlan &plan, int K, bool allow_ksplit) {
    return m2l_s2_ksplit(static_cast<int64_t>(n_tiles) * (plan.ce + plan.co) * K, allow_ksplit);
}

bool launch_m2l_stage2_pairs(const M2lClass *classes, const M2lTileDesc *tiles, const int32_t *tile_idx, int n_tiles,
                             const M2lS2PairsPlan &plan, int K, int64_t C, const double *cbuf, int64_t cbuf_len,
                             const uint16_t *qlist, double *Lp, hipStream_t s, bool allow_ksplit, int *ksplit_out) {
    if (n_tiles == 0) return true;
    // the contraction split of launch_m2l_stage2, on this launch's workgroups per tile (the parts add to the zeroed Lp)
    const int ksplit = m2l_s2_pairs_ksplit(n_tiles, plan, K, allow_ksplit);
    if (ksplit_out) *ksplit_out = ksplit;
    if (plan.ya > 0) { // two axes
#define M2L_S2_DISPATCH2(A, YA, B, YB)                                                                                   \
    if (plan.ga == A && plan.ya == YA && plan.gb == B && plan.yb == YB) {                                                \
        m2l_s2_pairs2_launch<A, YA, B, YB>(classes, tiles, tile_idx, n_tiles, plan, ksplit, K, C, cbuf, cbuf_len, qlist, \
                                           Lp, s);                                                                       \
        return true;                                                                                                     \
    }
        M2L_S2_PAIR2_WIDTHS(M2L_S2_DISPATCH2)
#undef M2L_S2_DISPATCH2
        return false;
    }
#define M2L_S2_DISPATCH(A, B)                                                                                           \
    if (plan.ga == A && plan.gb == B) {                                                                                  \
        m2l_s2_pairs_launch<A, B>(classes, tiles, tile_idx, n_tiles, plan, ksplit, K, C, cbuf, cbuf_len, qlist, Lp, s);  \
        return true;                                                                                                     \
    }
    M2L_S2_PAIR_WIDTHS(M2L_S2_DISPATCH)
#undef M2L_S2_DISPATCH
    return false; // a plan that m2l_s2_pairs_plan did not make: no instance, nothing launched
}

// Lp = [L_e | pad | L_o | pad] back to the node order, one wave per row = (right-hand side, cell): L[j] = L_e[j] + L_o[j]
// and L[rho j] = L_e[j] - L_o[j] for the representatives j < n_o, L[j] = L_e[j] on the centre plane; the padding of the
// row is written as zeros, so L needs no clearing before.  Streaming, HBM bound.
__global__ __launch_bounds__(256) void m2l_unparity_kernel(const double *__restrict__ Lp, int n_par, int ne16, double *__restrict__ L,
                                                           int n, int n_pad, int n_e, int n_o, int p, int p1, int64_t rows) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const double *src = Lp + row * n_par;
    double *dst = L + row * n_pad;
    m2l_unparity_row(src, ne16, n_e, n_o, p, p1, threadIdx.x & 63, [&](int m, double v) { dst[m] = v; });
    for (int j = n + (threadIdx.x & 63); j < n_pad; j += 64) dst[j] = 0.0;
}

void launch_m2l_unparity(const double *Lp, int n_par, int ne16, double *L, int n, int n_pad, int n_e, int n_o, int p, int64_t rows,
                         hipStream_t s) {
    if (rows <= 0) return;
    const int p1 = n_e / ((p + 1) / 2);
    hipLaunchKernelGGL(m2l_unparity_kernel, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, s, Lp, n_par, ne16, L, n, n_pad, n_e,
                       n_o, p, p1, rows);
}

// Lp in the basis of two axes back to the node order, the inverse of m2l_parity2_kernel in one pass: a representative (i0, i1
// < ceil(p/2), r < p2) reads ee, eo, oe, oo at the columns plan.col() and writes a = ee + eo, b = ee - eo, c = oe + oo, d =
// oe - oo as L[m] = a + c, L[rho_x m] = a - c, L[rho_y m] = b + d, L[rho_x rho_y m] = b - d; on a centre plane the part that is
// odd along that axis does not exist and the reflected node is the node itself.  The padding of the row is written as zeros.
__global__ __launch_bounds__(256) void m2l_unparity2_kernel(const double *__restrict__ Lp, M2lS2PairsPlan plan, double *__restrict__ L,
                                                            int n, int n_pad, int p, int p2, int64_t rows) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int n_par = plan.n_par();
    const double *src = Lp + row * n_par;
    double *dst = L + row * n_pad;
    m2l_unparity2_row(src, plan, p, p2, threadIdx.x & 63, [&](int m, double v) { dst[m] = v; });
    for (int j = n + (threadIdx.x & 63); j < n_pad; j += 64) dst[j] = 0.0;
}

void launch_m2l_unparity2(const double *Lp, const M2lS2PairsPlan &plan, double *L, int n, int n_pad, int p, int p2, int64_t rows,
                          hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(m2l_unparity2_kernel, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, s, Lp, plan, L, n, n_pad, p, p2,
                       rows);
}

// The multipoles in the parity basis of the x reflection: row = (right-hand side, cell), Mp[row] = [M_e | pad | M_o | pad]
// with M_e[j] = M[j] + M[rho j], M_o[j] = M[j] - M[rho j] for the representatives j < n_o, M_e[j] = M[j] on the centre
// plane n_o <= j < n_e of an odd order.  rho j = j + (p - 1 - 2 (j / p1)) p1, p1 = n_e / ceil(p / 2).  Streaming, HBM bound.
__global__ __launch_bounds__(256) void m2l_parity_kernel(const double *__restrict__ M, int n_pad, double *__restrict__ Mp, int n_par,
                                                         int ne16, int n_e, int n_o, int p, int p1, int64_t rows) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const double *src = M + row * n_pad;
    double *dst = Mp + row * n_par;
    m2l_parity_row(src, dst, ne16, n_e, n_o, p, p1, threadIdx.x & 63);
}

void launch_m2l_parity(const double *M, int n_pad, double *Mp, int n_par, int ne16, int n_e, int n_o, int p, int64_t rows,
                       hipStream_t s) {
    if (rows <= 0) return;
    const int p1 = n_e / ((p + 1) / 2);
    hipLaunchKernelGGL(m2l_parity_kernel, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, s, M, n_pad, Mp, n_par, ne16, n_e,
                       n_o, p, p1, rows);
}

// The multipoles in the parity basis of axes 0 and 1, the two-level butterfly in one pass: a representative (i0, i1 <
// ceil(p/2), r < p2) with node m = (i0 p + i1) p2 + r reads M at m, rho_x m, rho_y m, rho_x rho_y m and writes
// ee = (m + x) + (y + xy), eo = (m + x) - (y + xy), oe = (m - x) + (y - xy), oo = (m - x) - (y - xy); on a centre plane of an
// odd order the reflected node is the node itself and the part that is odd along that axis does not exist (the even
// part keeps the value once, as m2l_parity_kernel does).  Part ab holds its representatives in the order (i0, i1, r).
__global__ __launch_bounds__(256) void m2l_parity2_kernel(const double *__restrict__ M, int n_pad, double *__restrict__ Mp, int n_par,
                                                          M2lParityOffsets off, int p, int p2, int64_t rows) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const double *src = M + row * n_pad;
    double *dst = Mp + row * n_par;
    m2l_parity2_row(src, dst, off, p, p2, threadIdx.x & 63);
}

void launch_m2l_parity2(const double *M, int n_pad, double *Mp, int n_par, M2lParityOffsets off, int p, int p2, int64_t rows,
                        hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(m2l_parity2_kernel, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, s, M, n_pad, Mp, n_par, off, p, p2,
                       rows);
}

// The same change of basis (either layout) for the rows of a list of cells: one wave per (right-hand side, listed cell).
__global__ __launch_bounds__(256) void m2l_parity_cells_kernel(const double *__restrict__ M, int n_pad, double *__restrict__ Mp,
                                                               M2lParityRowArgs par, const int32_t *__restrict__ cells, int n_cells,
                                                               int K, int64_t C) {
    const int64_t job = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (job >= static_cast<int64_t>(K) * n_cells) return;
    const int64_t row = (job / n_cells) * C + cells[job % n_cells];
    m2l_parity_row_any(par, M + row * n_pad, Mp + row * par.n_par, threadIdx.x & 63);
}

void launch_m2l_parity_cells(const double *M, int n_pad, double *Mp, const M2lParityRowArgs &par, const int32_t *cells, int n_cells,
                             int K, int64_t C, hipStream_t s) {
    if (n_cells <= 0 || K <= 0) return;
    hipLaunchKernelGGL(m2l_parity_cells_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(K) * n_cells + 3) / 4)), dim3(256), 0, s, M,
                       n_pad, Mp, par, cells, n_cells, K, C);
}

// Slot segments of absent pairs: 16 lanes per segment, 16 bytes per lane and round.
__global__ __launch_bounds__(256) void m2l_zero_segments_kernel(const int32_t *__restrict__ segs, int64_t n_segs,
                                                                double *__restrict__ cbuf, int64_t cbuf_len) {
    const int64_t sg = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    if (sg >= n_segs) return;
    const int2 e = reinterpret_cast<const int2 *>(segs)[sg];
    double2 *dst = reinterpret_cast<double2 *>(cbuf + static_cast<int64_t>(blockIdx.y) * cbuf_len) + e.x;
    for (int i = l; i < e.y; i += 16) dst[i] = make_double2(0.0, 0.0);
}

void launch_m2l_zero_segments(const int32_t *segs, int64_t n_segs, int K, double *cbuf, int64_t cbuf_len, hipStream_t s) {
    if (n_segs <= 0) return;
    hipLaunchKernelGGL(m2l_zero_segments_kernel, dim3(static_cast<unsigned>((n_segs * 16 + 255) / 256), K), dim3(256), 0, s, segs,
                       n_segs, cbuf, cbuf_len);
}

// Shared-basis extension: change of basis of every cell of a level (stage 3 of the GEMM kernel), OUT[cell][0..out_ld) =
// sum_k IN[cell][k] * OP_level[k][0..out_ld).  classes[].cells / u_all: the level's cells and its in_ld x out_ld operator.
void launch_m2l_basis(const M2lClass *classes, const M2lTileDesc *tiles, int n_tiles, int in_ld, int out_ld, int K,
                      int64_t C, const double *in, double *out, hipStream_t s) {
    if (n_tiles == 0) return;
    m2l_dispatch_chunks<3>(out_ld / 16, classes, tiles, n_tiles, out_ld, 2, K, C, in, in_ld, out, 0, nullptr, 0, nullptr, s);
}

// Setup-time product for the projected operators: C[i][j] = sum_k A(i, k) * B[k][j], A(i, k) = A[k * lda + i] (TA) or
// A[i * lda + k]; 64 x 64 tiles, 4 x 4 per thread, 16 contraction indices per LDS round.
template <bool TA>
__global__ __launch_bounds__(256) void small_gemm_kernel(int M, int N, int Kd, const double *__restrict__ A, int64_t lda,
                                                         const double *__restrict__ B, int64_t ldb, double *__restrict__ Cm,
                                                         int64_t ldc) {
    __shared__ double sa[16][64 + 1], sb[16][64 + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    double acc[4][4] = {};
    for (int k0 = 0; k0 < Kd; k0 += 16) {
        for (int e = threadIdx.x; e < 16 * 64; e += 256) {
            const int kk = TA ? e >> 6 : e & 15, ii = TA ? e & 63 : e >> 4;
            const int k = k0 + kk, i = i0 + ii;
            sa[kk][ii] = (k < Kd && i < M) ? (TA ? A[(int64_t)k * lda + i] : A[(int64_t)i * lda + k]) : 0.0;
        }
        for (int e = threadIdx.x; e < 16 * 64; e += 256) {
            const int kk = e >> 6, jj = e & 63;
            const int k = k0 + kk, j = j0 + jj;
            sb[kk][jj] = (k < Kd && j < N) ? B[(int64_t)k * ldb + j] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = sa[kk][ty + 16 * r];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = sb[kk][tx + 16 * c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] += a[r] * b[c];
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
            if (i < M && j < N) Cm[(int64_t)i * ldc + j] = acc[r][c];
        }
}

void launch_small_gemm(bool trans_a, int M, int N, int Kd, const double *A, int64_t lda, const double *B, int64_t ldb,
                       double *Cm, int64_t ldc, hipStream_t s) {
    if (M <= 0 || N <= 0) return;
    const dim3 grid((N + 63) / 64, (M + 63) / 64);
    if (trans_a) hipLaunchKernelGGL(small_gemm_kernel<true>, grid, dim3(256), 0, s, M, N, Kd, A, lda, B, ldb, Cm, ldc);
    else hipLaunchKernelGGL(small_gemm_kernel<false>, grid, dim3(256), 0, s, M, N, Kd, A, lda, B, ldb, Cm, ldc);
}

// ------------------------------------------------------------------ stacked M2L operators, assembled in HBM
// fmm_m2l_tables.cpp fill_m2l_operator_arrays on the device: the reference operators of a level (16 in 3-D) and the
// symmetry tables go up once (MBs), the stacked per-class operators (GBs) are gathered from them here instead
// of being filled on the host and sent over PCIe.  VtAll[m][first_row(t) + kk] = Vt_ref(t)[kk][invperm_t[m]]
// (identity rows when uncompressed); UAll[tgt_off(t) + kk][i] = U_ref(t)[invperm_t[i]][kk].
__global__ __launch_bounds__(256) void assemble_vt_kernel(M2lAssembleClass c, int n, int n_pad, int compressed,
                                                          const double *__restrict__ ops, const int32_t *__restrict__ invperm,
                                                          double *__restrict__ vt_all) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= static_cast<int64_t>(c.n_src) * n) return;
    const int pos = static_cast<int>(t / n), m = static_cast<int>(t % n);
    const M2lAssembleTv tv = c.src[pos];
    const int im = invperm[static_cast<int64_t>(tv.perm) * n + m];
    double *dst = vt_all + static_cast<int64_t>(m) * c.r_pad16 + tv.row;
    if (compressed) {
        const double *src = ops + tv.vt_off + static_cast<int64_t>(im) * tv.rank;
        for (int kk = 0; kk < tv.rank; ++kk) dst[kk] = src[kk];
    } else {
        dst[im] = 1.0;
    }
}

// The same in the parity basis: one thread per (row-owning transfer vector, representative j < n_e) writes the entries
// of Vt_e row j and, off the centre plane, of Vt_o row ne16 + j; the factor 1/2 is exact.
__global__ __launch_bounds__(256) void assemble_vt_parity_kernel(M2lAssembleClass c, int n, const double *__restrict__ ops,
                                                                 const int32_t *__restrict__ invperm, double *__restrict__ vt_all) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= static_cast<int64_t>(c.n_src) * c.n_e) return;
    const int pos = static_cast<int>(t / c.n_e), j = static_cast<int>(t % c.n_e);
    const M2lAssembleTv tv = c.src[pos];
    const int p1 = n / c.p;
    const int rj = j + (c.p - 1 - 2 * (j / p1)) * p1;
    const int32_t *inv = invperm + static_cast<int64_t>(tv.perm) * n;
    const double *s0 = ops + tv.vt_off + static_cast<int64_t>(inv[j]) * tv.rank;
    const double *s1 = ops + tv.vt_off + static_cast<int64_t>(inv[rj]) * tv.rank;
    double *de = vt_all + static_cast<int64_t>(j) * c.r_pad16 + tv.row;
    double *dod = vt_all + static_cast<int64_t>(c.ne16 + j) * c.r_pad16 + tv.row;
    if (j >= c.n_o) {
        for (int kk = 0; kk < tv.rank; ++kk) de[kk] = s0[kk];
    } else {
        for (int kk = 0; kk < tv.rank; ++kk) {
            de[kk] = 0.5 * (s0[kk] + s1[kk]);
            dod[kk] = 0.5 * (s0[kk] - s1[kk]);
        }
    }
}

// The same in the parity basis of axes 0 and 1 (m2l_parity2_kernel's enumeration): one thread per (row-owning transfer
// vector, representative of ee); the factors 1/2 and 1/4 are exact.
__global__ __launch_bounds__(256) void assemble_vt_parity2_kernel(M2lAssembleClass c, int n, const double *__restrict__ ops,
                                                                  const int32_t *__restrict__ invperm, double *__restrict__ vt_all) {
    const int p = c.p, p2 = n / (p * p), h = (p + 1) / 2, f = p / 2, n_ee = h * h * p2;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= static_cast<int64_t>(c.n_src) * n_ee) return;
    const int pos = static_cast<int>(t / n_ee), e = static_cast<int>(t % n_ee);
    const M2lAssembleTv tv = c.src[pos];
    const int i0 = e / (h * p2), i1 = (e - i0 * h * p2) / p2, r = e - (i0 * h + i1) * p2;
    const int m = (i0 * p + i1) * p2 + r;
    const int dx = (p - 1 - 2 * i0) * p * p2, dy = (p - 1 - 2 * i1) * p2;
    const bool cx = i0 >= f, cy = i1 >= f;
    const int32_t *inv = invperm + static_cast<int64_t>(tv.perm) * n;
    const double *s0 = ops + tv.vt_off + static_cast<int64_t>(inv[m]) * tv.rank;
    const double *sx = ops + tv.vt_off + static_cast<int64_t>(inv[m + dx]) * tv.rank;
    const double *sy = ops + tv.vt_off + static_cast<int64_t>(inv[m + dy]) * tv.rank;
    const double *sxy = ops + tv.vt_off + static_cast<int64_t>(inv[m + dx + dy]) * tv.rank;
    const int je = (i0 * h + i1) * p2 + r, jo = (i0 * f + i1) * p2 + r;
    double *dee = vt_all + static_cast<int64_t>(c.s1_off.v[0] + je) * c.r_pad16 + tv.row;
    double *deo = vt_all + static_cast<int64_t>(c.s1_off.v[1] + jo) * c.r_pad16 + tv.row;
    double *doe = vt_all + static_cast<int64_t>(c.s1_off.v[2] + je) * c.r_pad16 + tv.row;
    double *doo = vt_all + static_cast<int64_t>(c.s1_off.v[3] + jo) * c.r_pad16 + tv.row;
    const double wx = cx ? 1.0 : 0.5, wy = cy ? 1.0 : 0.5;
    for (int kk = 0; kk < tv.rank; ++kk) {
        const double v = s0[kk], vx = sx[kk], vy = sy[kk], vxy = sxy[kk];
        const double e0 = cx ? v : v + vx, e1 = cx ? vy : vy + vxy, o0 = v - vx, o1 = vy - vxy;
        dee[kk] = wx * wy * (cy ? e0 : e0 + e1);
        if (!cy) deo[kk] = wx * wy * (e0 - e1);
        if (!cx) doe[kk] = wx * wy * (cy ? o0 : o0 + o1);
        if (!cx && !cy) doo[kk] = wx * wy * (o0 - o1);
    }
}

__global__ __launch_bounds__(256) void assemble_u_kernel(M2lAssembleClass c, int n, int n_pad, const double *__restrict__ ops,
                                                         const int32_t *__restrict__ invperm, double *__restrict__ u_all) {
    const int pos = blockIdx.y;
    const M2lAssembleTv tv = c.tgt[pos];
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= static_cast<int64_t>(tv.rank) * n) return;
    const int kk = static_cast<int>(t / n), i = static_cast<int>(t % n);
    u_all[static_cast<int64_t>(tv.row + kk) * n_pad + i] = ops[tv.u_off + static_cast<int64_t>(kk) * n + invperm[static_cast<int64_t>(tv.perm) * n + i]];
}

// The same in the parity basis of stage 2: one thread per (rank index kk, representative i < u_ne) of a transfer vector
// that owns operator rows writes U_e[row + kk][i] and, off the centre plane, U_o[row + kk][i]; the factor 1/2 is exact.
__global__ __launch_bounds__(256) void assemble_u_parity_kernel(M2lAssembleClass c, int n, const double *__restrict__ ops,
                                                                const int32_t *__restrict__ invperm, double *__restrict__ u_all) {
    const M2lAssembleTv tv = c.tgt[blockIdx.y];
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= static_cast<int64_t>(tv.rank) * c.u_ne) return;
    const int kk = static_cast<int>(t / c.u_ne), i = static_cast<int>(t % c.u_ne);
    const int p1 = n / c.p;
    const int ri = i + (c.p - 1 - 2 * (i / p1)) * p1;
    const int32_t *inv = invperm + static_cast<int64_t>(tv.perm) * n;
    const double *ucol = ops + tv.u_off + static_cast<int64_t>(kk) * n;
    double *dst = u_all + static_cast<int64_t>(tv.row + kk) * c.u_npar;
    const double a = ucol[inv[i]];
    if (i >= c.u_no) {
        dst[i] = a;
    } else {
        const double b = ucol[inv[ri]];
        dst[i] = 0.5 * (a + b);
        dst[c.u_ne16 + i] = 0.5 * (a - b);
    }
}

// The same in the parity basis of axes 0 and 1 (assemble_vt_parity2_kernel's enumeration and factors): one thread per (rank
// index kk, representative of ee) writes the entries of U_ee, U_eo, U_oe, U_oo of row + kk at the columns u_plan.col().
__global__ __launch_bounds__(256) void assemble_u_parity2_kernel(M2lAssembleClass c, int n, const double *__restrict__ ops,
                                                                 const int32_t *__restrict__ invperm, double *__restrict__ u_all) {
    const int p = c.p, p2 = n / (p * p), h = (p + 1) / 2, f = p / 2, n_ee = h * h * p2;
    const M2lAssembleTv tv = c.tgt[blockIdx.y];
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= static_cast<int64_t>(tv.rank) * n_ee) return;
    const int kk = static_cast<int>(t / n_ee), e = static_cast<int>(t % n_ee);
    const int i0 = e / (h * p2), i1 = (e - i0 * h * p2) / p2, r = e - (i0 * h + i1) * p2;
    const int m = (i0 * p + i1) * p2 + r;
    const int dx = (p - 1 - 2 * i0) * p * p2, dy = (p - 1 - 2 * i1) * p2;
    const bool cx = i0 >= f, cy = i1 >= f;
    const int32_t *inv = invperm + static_cast<int64_t>(tv.perm) * n;
    const double *ucol = ops + tv.u_off + static_cast<int64_t>(kk) * n;
    double *dst = u_all + static_cast<int64_t>(tv.row + kk) * c.u_npar;
    const int je = (i0 * h + i1) * p2 + r, jo = (i0 * f + i1) * p2 + r;
    const double v = ucol[inv[m]], vx = ucol[inv[m + dx]], vy = ucol[inv[m + dy]], vxy = ucol[inv[m + dx + dy]];
    const double w = (cx ? 1.0 : 0.5) * (cy ? 1.0 : 0.5);
    const double e0 = cx ? v : v + vx, e1 = cx ? vy : vy + vxy, o0 = v - vx, o1 = vy - vxy;
    dst[c.u_plan.col(0, je)] = w * (cy ? e0 : e0 + e1);
    if (!cy) dst[c.u_plan.col(1, jo)] = w * (e0 - e1);
    if (!cx) dst[c.u_plan.col(2, je)] = w * (cy ? o0 : o0 + o1);
    if (!cx && !cy) dst[c.u_plan.col(3, jo)] = w * (o0 - o1);
}

void launch_m2l_assemble(const M2lAssembleClass &c, int n, int n_pad, bool compressed, const double *ops,
                         const int32_t *invperm, double *vt_all, double *u_all, hipStream_t s) {
    (void)hipMemsetAsync(vt_all, 0, static_cast<size_t>(c.n_e > 0 ? c.n_par : n_pad) * c.r_pad16 * sizeof(double), s);
    (void)hipMemsetAsync(u_all, 0, (c.u_npar > 0 ? static_cast<size_t>(c.u_rows) * c.u_npar : static_cast<size_t>(c.k_pad) * n_pad) * sizeof(double), s);
    if (c.n_src > 0 && c.n_e > 0 && c.s1_axes == 2) {
        const int h = (c.p + 1) / 2, n_ee = h * h * (n / (c.p * c.p));
        hipLaunchKernelGGL(assemble_vt_parity2_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(c.n_src) * n_ee + 255) / 256)), dim3(256),
                           0, s, c, n, ops, invperm, vt_all);
    } else if (c.n_src > 0 && c.n_e > 0)
        hipLaunchKernelGGL(assemble_vt_parity_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(c.n_src) * c.n_e + 255) / 256)), dim3(256),
                           0, s, c, n, ops, invperm, vt_all);
    else if (c.n_src > 0)
        // (one thread per entry, no grid-stride loop: the exact block count, not grid_for's capped one)
        hipLaunchKernelGGL(assemble_vt_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(c.n_src) * n + 255) / 256)), dim3(256), 0, s, c, n, n_pad,
                           compressed ? 1 : 0, ops, invperm, vt_all);
    if (c.n_tgt > 0 && c.max_rank > 0 && c.u_npar > 0 && c.u_plan.ya > 0) {
        const int h = (c.p + 1) / 2, n_ee = h * h * (n / (c.p * c.p));
        hipLaunchKernelGGL(assemble_u_parity2_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(c.max_rank) * n_ee + 255) / 256), c.n_tgt),
                           dim3(256), 0, s, c, n, ops, invperm, u_all);
    } else if (c.n_tgt > 0 && c.max_rank > 0 && c.u_npar > 0)
        hipLaunchKernelGGL(assemble_u_parity_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(c.max_rank) * c.u_ne + 255) / 256), c.n_tgt),
                           dim3(256), 0, s, c, n, ops, invperm, u_all);
    else if (c.n_tgt > 0 && c.max_rank > 0)
        hipLaunchKernelGGL(assemble_u_kernel, dim3(static_cast<unsigned>((static_cast<int64_t>(c.max_rank) * n + 255) / 256), c.n_tgt), dim3(256), 0, s, c,
                           n, n_pad, ops, invperm, u_all);
}

} // namespace bbfmm
