// Target -> leaf assignment and grouping on the device (the per-evaluate part:
// points_to_keys / points_to_leaves, ferreus_bbfmm/src/linear_tree.rs:487-534, bbfmm.rs:455-465).
// Same arithmetic as the host path (tree.cpp points_to_leaves): f64 floor((x - disp) / side) anchors,
// Morton key at the tree depth, walk up the parents until a leaf of the tree is found; rows are then
// grouped by leaf in ascending cell index with ascending rows inside a leaf (stable radix sort), so
// the target set is identical to the one the host builds.
#pragma once
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace bbfmm {

struct DevLeafLookup {
    const uint64_t *keys = nullptr; // open-addressing table of the tree's cells (KeyTable)
    const int32_t *vals = nullptr;
    uint64_t mask = 0;
    const uint8_t *is_leaf = nullptr;
    int d = 3, depth = 0;
    double disp[3] = {0, 0, 0};
    double side = 1.0;
};

// cell[i] = leaf of row i or -1; *bad_row = min(*bad_row, first row outside the tree)
void launch_points_to_leaves(const DevLeafLookup &lk, const double *x0, const double *x1, const double *x2, int64_t m,
                             int32_t *cell, unsigned long long *bad_row, hipStream_t s);

// scratch bytes group_targets needs for m rows (keys of end_bit bits)
size_t group_targets_temp_bytes(int64_t m, int end_bit);

// cell (m) -> cell_sorted, perm (sorted position -> row); heads (m bytes) scratch;
// runs: job_cell / tgt_begin / tgt_end (capacity >= min(m, cells)), *n_runs on the device.
int group_targets(const int32_t *cell, int64_t m, int end_bit, int32_t *cell_sorted, int32_t *perm, uint8_t *heads,
                  int32_t *job_cell, int32_t *tgt_begin, int32_t *tgt_end, int32_t *n_runs, void *temp, size_t temp_bytes,
                  hipStream_t s);

// Jobs of bounded size: a run of n targets starting at b is cut into q = ceil(n / cap) jobs, job j covering
// [b + floor(j n / q), b + floor((j + 1) n / q)) -- the jobs tile the run, none is empty, their sizes differ by at most
// one.  One definition for the host restatement and the kernels.
#if defined(__HIPCC__)
#define BBFMM_TARGETS_HD __host__ __device__
#else
#define BBFMM_TARGETS_HD
#endif
BBFMM_TARGETS_HD inline int64_t split_job_count(int64_t n, int64_t cap) { return n <= 0 ? 0 : (n + cap - 1) / cap; }
BBFMM_TARGETS_HD inline int64_t split_job_edge(int64_t b, int64_t n, int64_t q, int64_t j) { return b + j * n / q; }

// scratch bytes split_runs needs for n_runs runs
size_t split_runs_temp_bytes(int64_t n_runs);
// The runs (job_cell / tgt_begin / tgt_end, n_runs of them, the count known to the host) cut into jobs of at most cap >= 1
// targets, in run order: a count per run (cnt), an exclusive scan (offs), then a fill by one thread per job -- nothing is
// placed by an atomic.  out_*: `capacity` entries, >= split_jobs_capacity() (nothing is written past it); *n_jobs (device)
// the number of jobs.
inline int64_t split_jobs_capacity(int64_t n_runs, int64_t m, int64_t cap) { return n_runs + m / cap; }
int split_runs(const int32_t *job_cell, const int32_t *tgt_begin, const int32_t *tgt_end, int64_t n_runs, int32_t cap, int32_t *cnt,
               int32_t *offs, int32_t *out_cell, int32_t *out_begin, int32_t *out_end, int64_t capacity, int32_t *n_jobs, void *temp,
               size_t temp_bytes, hipStream_t s);
// the same rule on host arrays; returns the number of jobs (out_* may be null: the count alone)
int64_t split_runs_host(const int32_t *job_cell, const int32_t *tgt_begin, const int32_t *tgt_end, int64_t n_runs, int32_t cap,
                        int32_t *out_cell, int32_t *out_begin, int32_t *out_end);

// out[a][i] = in[a][perm[i]] for the axes with non-null pointers
void launch_gather_targets(const double *in0, const double *in1, const double *in2, const int32_t *perm, int64_t m,
                           double *out0, double *out1, double *out2, hipStream_t s);

} // namespace bbfmm
