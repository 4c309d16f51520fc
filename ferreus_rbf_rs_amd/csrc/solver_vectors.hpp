// Vector kernels of the device-resident solvers (solver_device.cpp; iterative_solvers.rs:38-281): what
// bbfmm_fgmres / bbfmm_schwarz_ddm_solver do to their host vectors, as kernels on one stream whose scalars live in
// device memory.  All HBM-streaming, f64.
//
// Layout: block c of a launch owns the elements [c * kSolverChunk, (c + 1) * kSolverChunk) -- the host solver's
// kChunk -- whatever the vector length, and thread t of it the pairs (it * 1024 + t) * 2 + {0, 1}, it = 0 .. 31.  A
// reduction adds a thread's elements in that order, the 64 lanes of a wave by shuffles (offsets 32, 16, .. 1), the 16
// waves in wave order through LDS, and writes ONE partial per chunk; reduce_finish adds the partials in index order
// like reduce_chunks on the host.  No atomics: the same bits every run, and nothing depends on a grid size.
// Elementwise results use separate multiply and add roundings (no fused multiply-add), like the host loops.
// Pointers that are all 16-byte aligned are read and written as double2; any other alignment takes 8-byte accesses
// with the same element-to-thread map, so the results do not depend on the alignment either.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct bbfmm_handle;
struct bbfmm_schwarz;

namespace bbfmm {

constexpr int64_t kSolverChunk = 1 << 16;
inline int64_t solver_chunks(int64_t n) { return n < 1 ? 1 : (n + kSolverChunk - 1) / kSolverChunk; }

// How a kernel reads its factor alpha.
enum SolverAlpha : int32_t {
    kAlphaSlot = 0,    // *slot
    kAlphaNegSlot = 1, // -*slot
    kAlphaInvSlot = 2, // 1 / *slot, and 0 when *slot == 0 (a zero norm yields a zero vector)
    kAlphaImmediate = 3 // the argument `imm`
};
// What a pass adds to its elementwise work.
enum SolverReduce : int32_t { kReduceNone = 0, kReduceDot = 1, kReduceMax = 2 };

// y = a - b; part_sum[c] = sum y^2, part_max[c] = max |y| over chunk c (either may be nullptr)
void launch_solver_sub(const double *a, const double *b, double *y, int64_t n, double *part_sum, double *part_max, hipStream_t s);
// y = alpha x
void launch_solver_scale(const double *x, const double *slot, int32_t mode, double imm, double *y, int64_t n, hipStream_t s);
// y += alpha x (x == nullptr: y is left as it is), then per chunk: kReduceDot -> sum d[i] y[i] (d == nullptr: y[i]^2),
// kReduceMax -> max |y[i]|.  The modified Gram-Schmidt step "w -= h_i v_i; h_{i+1} = <v_{i+1}, w>" in one pass over w.
void launch_solver_axpy_reduce(const double *x, const double *slot, int32_t mode, double imm, double *y, const double *d,
                               int64_t n, int32_t reduce, double *part, hipStream_t s);
// *out = the partials 0 .. n_chunks-1 combined in index order (sum, or max starting from 0), then sqrt when asked
void launch_solver_reduce_finish(const double *part, int64_t n_chunks, bool take_max, bool take_sqrt, double *out, hipStream_t s);
// x[i] = (..((x[i] + y[0] z[i]) + y[1] z[ldz + i]) ..) + y[count-1] z[(count-1) ldz + i]     (get_solution)
void launch_solver_update(const double *z, int64_t ldz, const double *y, int32_t count, double *x, int64_t n, hipStream_t s);
// y[i] = (y[i] + x[i] nugget) + sum_q P[q ldp + i] x[N + q] for i < N (the sum first, then added); y[N .. N + basis) = 0
void launch_rbf_system_tail(const double *x, const double *P, int64_t ldp, int32_t basis, double nugget, int64_t N, double *y,
                            hipStream_t s);
// out[i] = v[i], i < count <= 16 (the polynomial tail of a Schwarz correction, passed by value)
struct SolverTail {
    double v[16];
};
void launch_solver_set_tail(SolverTail t, int32_t count, double *out, hipStream_t s);

// schwarz.cpp: the tree a Schwarz preconditioner was built on
bbfmm_handle *schwarz_tree(const bbfmm_schwarz *h);
// solver_device.cpp: the tree a native device operator belongs to (nullptr: not a native operator)
bbfmm_handle *rbf_system_device_tree(const void *user);

} // namespace bbfmm
