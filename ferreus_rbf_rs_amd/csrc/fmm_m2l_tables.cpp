// FmmTree: the stacked, permutation-folded M2L tables, their bounded batches, and the host fill of the
// stacked operators.  See fmm_tree.hpp.  (The shared-basis extension: fmm_m2l_shared_basis.cpp; the test hooks: fmm_m2l_debug.cpp.)
#include "fmm_tree_impl.hpp"

namespace bbfmm {

// Stacked operators of one (level, class): VtAll (n_pad x r_pad16) and UAll (k_pad x n_pad; in the parity basis of stage 2
// (k_pad - kp) x n_par).
void FmmTree::fill_m2l_operator_arrays(const HostM2lClass &hc, std::vector<double> *vt_all,
                                       std::vector<double> *u_all) const {
    const int n_pad = round_up(ops_.n, 32);
    vt_all->resize(static_cast<size_t>(m2l_pairs_ ? m2l_npar_ : n_pad) * hc.r_pad16);
    u_all->resize(m2l_pairs2_ ? static_cast<size_t>(hc.k_pad - hc.kp) * m2l_s2_plan_.n_par() : static_cast<size_t>(hc.k_pad) * n_pad);
    fill_m2l_operator_arrays(hc, vt_all->data(), u_all->data());
}

// vt_all: n_pad x r_pad16 (m2l_npar_ x r_pad16 in the parity basis), u_all: k_pad x n_pad (both overwritten, padding zeroed)
void FmmTree::fill_m2l_operator_arrays(const HostM2lClass &hc, double *vt_all, double *u_all) const {
    const int n = ops_.n, n_pad = round_up(n, 32);
    const bool compressed = ops_.compression != kCompressionNone;
    const auto &lops = ops_.m2l[hc.level];
    auto zero = [](double *p, size_t len) {
        parallel_for_chunks(static_cast<int64_t>(len), int64_t(1) << 18, [&](int64_t b, int64_t e) {
            std::memset(p + b, 0, static_cast<size_t>(e - b) * sizeof(double));
        });
    };
    zero(vt_all, static_cast<size_t>(m2l_pairs_ ? m2l_npar_ : n_pad) * hc.r_pad16);
    zero(u_all, m2l_pairs2_ ? static_cast<size_t>(hc.k_pad - hc.kp) * m2l_s2_plan_.n_par() : static_cast<size_t>(hc.k_pad) * n_pad);
    struct RowSrc {
        const M2lOperator *op;
        const int32_t *inv;
        int first_row;
    };
    std::vector<RowSrc> row_src;
    for (size_t pos = 0; pos < hc.src_tv.size(); ++pos) {
        if (m2l_pairs_ && hc.src_pair[pos] == -2) continue; // the second of a pair shares the rows of the first
        const int tv = hc.src_tv[pos];
        const M2lOperator &op = lops[ops_.ref_lookup[tv]];
        row_src.push_back(RowSrc{&op, &ops_.invperm[static_cast<size_t>(ops_.perm_lookup[tv]) * n], hc.src_row0[pos]});
    }
    // Parity basis: rows [0, ne16) hold Vt_e[kk][j] = (Vt_t[kk][j] + Vt_t[kk][rho j]) / 2 (the centre plane of an odd
    // order: Vt_t[kk][j]), rows [ne16, n_par) hold Vt_o[kk][j] = (Vt_t[kk][j] - Vt_t[kk][rho j]) / 2
    // Two axes: row k of the part ab holds (1 / orbit) sum over the orbit of +- Vt_t[kk][.] (m2l_par_node_ / m2l_par_sign_;
    // the orbit has 1, 2 or 4 nodes, so the factor is exact)
    if (m2l_pairs_ && m2l_axes_ == 2) {
        parallel_for(m2l_npar_, 8, [&](int64_t k) {
            const int32_t *nd = &m2l_par_node_[static_cast<size_t>(4 * k)];
            const int8_t *sg = &m2l_par_sign_[static_cast<size_t>(4 * k)];
            int cnt = 0;
            for (int g = 0; g < 4; ++g) cnt += nd[g] >= 0;
            if (cnt == 0) return; // padding
            const double w = 1.0 / cnt;
            double *dst = vt_all + static_cast<size_t>(k) * hc.r_pad16;
            for (const RowSrc &rs : row_src) {
                const int r = rs.op->rank;
                for (int kk = 0; kk < r; ++kk) {
                    double v = 0.0;
                    for (int g = 0; g < 4; ++g)
                        if (nd[g] >= 0) v += sg[g] * rs.op->vt[static_cast<size_t>(rs.inv[nd[g]]) * r + kk];
                    dst[rs.first_row + kk] = w * v;
                }
            }
        });
    } else if (m2l_pairs_) {
        parallel_for(m2l_ne_, 8, [&](int64_t j) {
            const bool centre = j >= m2l_no_;
            const int rj = m2l_rho(static_cast<int>(j));
            double *de = vt_all + static_cast<size_t>(j) * hc.r_pad16;
            double *dod = vt_all + static_cast<size_t>(m2l_ne16_ + j) * hc.r_pad16;
            for (const RowSrc &rs : row_src) {
                const int r = rs.op->rank;
                const double *s0 = &rs.op->vt[static_cast<size_t>(rs.inv[j]) * r], *s1 = &rs.op->vt[static_cast<size_t>(rs.inv[rj]) * r];
                for (int kk = 0; kk < r; ++kk) {
                    if (centre) {
                        de[rs.first_row + kk] = s0[kk];
                    } else {
                        de[rs.first_row + kk] = 0.5 * (s0[kk] + s1[kk]);
                        dod[rs.first_row + kk] = 0.5 * (s0[kk] - s1[kk]);
                    }
                }
            }
        });
    } else {
        // c[kk] = sum_m Vt[kk][invperm[m]] * M_V[m]   (bbfmm.rs:924-930 folded)
        parallel_for(n, 8, [&](int64_t m) {
            double *dst = vt_all + static_cast<size_t>(m) * hc.r_pad16;
            for (const RowSrc &rs : row_src) {
                const int r = rs.op->rank;
                const int im = rs.inv[m];
                if (compressed) {
                    const double *src = &rs.op->vt[static_cast<size_t>(im) * r];
                    for (int kk = 0; kk < r; ++kk) dst[rs.first_row + kk] = src[kk];
                } else {
                    dst[rs.first_row + im] = 1.0;
                }
            }
        });
    }
    // Parity basis of stage 2: operator row (leader: its slot offset; single: its slot offset - kp) holds U_e[kk][i] =
    // (U_t[kk][i] + U_t[kk][rho i]) / 2 in columns [0, ne16) and U_o[kk][i] = (U_t[kk][i] - U_t[kk][rho i]) / 2 behind them
    if (m2l_pairs2_) {
        const int n_par = m2l_s2_plan_.n_par(), ne16 = m2l_s2_plan_.ne16();
        parallel_for(static_cast<int64_t>(hc.tgt_tv.size()), 1, [&](int64_t pos) {
            if (hc.tgt_pair[pos] == -2) return; // the partner shares the rows of the leader
            const int tv = hc.tgt_tv[pos];
            const M2lOperator &op = lops[ops_.ref_lookup[tv]];
            const int32_t *inv = &ops_.invperm[static_cast<size_t>(ops_.perm_lookup[tv]) * n];
            const int row0 = hc.tgt_off[pos] - (hc.tgt_pair[pos] >= 0 ? 0 : hc.kp);
            for (int kk = 0; kk < op.rank; ++kk) {
                double *dst = u_all + static_cast<size_t>(row0 + kk) * n_par;
                const double *ucol = &op.u[static_cast<size_t>(kk) * n];
                // two axes: column k holds (1 / orbit) sum over the orbit of +- U_t[kk][.] (m2l_s2_node_ / m2l_s2_sign_)
                for (int k = 0; m2l_s2_axes_ == 2 && k < n_par; ++k) {
                    const int32_t *nd = &m2l_s2_node_[static_cast<size_t>(4 * k)];
                    const int8_t *sg = &m2l_s2_sign_[static_cast<size_t>(4 * k)];
                    if (nd[0] < 0) continue; // padding
                    int cnt = 0;
                    double half[2] = {0.0, 0.0}; // (m, rho_x m) and (rho_y m, rho_x rho_y m), summed as the device's butterfly does
                    for (int g = 0; g < 4; ++g)
                        if (nd[g] >= 0) {
                            half[g >> 1] += sg[g] * ucol[inv[nd[g]]];
                            ++cnt;
                        }
                    dst[k] = (half[0] + half[1]) / cnt;
                }
                if (m2l_s2_axes_ == 2) continue;
                for (int i = 0; i < m2l_ne_; ++i) {
                    const double a = ucol[inv[i]], b = ucol[inv[m2l_rho(i)]];
                    if (i >= m2l_no_) {
                        dst[i] = a;
                    } else {
                        dst[i] = 0.5 * (a + b);
                        dst[ne16 + i] = 0.5 * (a - b);
                    }
                }
            }
        });
        return;
    }
    // L_B[i] += sum_kk U[invperm[i]][kk] * c[kk]   (bbfmm.rs:975-981 folded)
    parallel_for(static_cast<int64_t>(hc.tgt_tv.size()), 1, [&](int64_t pos) {
        const int tv = hc.tgt_tv[pos];
        const M2lOperator &op = lops[ops_.ref_lookup[tv]];
        const int32_t *inv = &ops_.invperm[static_cast<size_t>(ops_.perm_lookup[tv]) * n];
        for (int kk = 0; kk < op.rank; ++kk) {
            double *dst = u_all + static_cast<size_t>(hc.tgt_off[pos] + kk) * n_pad;
            const double *ucol = &op.u[static_cast<size_t>(kk) * n];
            for (int i = 0; i < n; ++i) dst[i] = ucol[inv[i]];
        }
    });
}

// ---------------------------------------------------------------- the table builder
// build_m2l_tables() at the end of the file is the table of contents: one function per stage, in the order of the calls.
// What flows between the stages lives in the structs below; what a stage writes of the handle's members is in its comment.

// The switches, read once per handle at the top of build_m2l_tables() (tests vary them inside one process: no statics).
struct FmmTree::M2lSwitches {
    double cbuf_mb = 0.0;                  // BBFMM_M2L_CBUF_MB > 0: the budget of the intermediate (fractions allowed)
    bool s1_pairs = true, s2_pairs = true; // BBFMM_M2L_S1_PAIRS / _S2_PAIRS = 0: no pairs in that stage
    int s1_axes = 0, s2_axes = 0;          // BBFMM_M2L_S1_AXES / _S2_AXES: 1, 2; 0 (unset): by executed work
    int variant_min_tiles = 4;             // BBFMM_M2L_VARIANTS: 0 none, n > 0 runs of at least n full tiles
    bool verbose = false;                  // BBFMM_VERBOSE
    static M2lSwitches read() {
        M2lSwitches sw;
        auto number = [](const char *name, int unset) {
            const char *e = std::getenv(name);
            return e ? std::atoi(e) : unset;
        };
        if (const char *e = std::getenv("BBFMM_M2L_CBUF_MB")) sw.cbuf_mb = std::atof(e);
        sw.s1_pairs = number("BBFMM_M2L_S1_PAIRS", 1) != 0;
        sw.s2_pairs = number("BBFMM_M2L_S2_PAIRS", 1) != 0;
        sw.s1_axes = number("BBFMM_M2L_S1_AXES", 0);
        sw.s2_axes = number("BBFMM_M2L_S2_AXES", 0);
        sw.variant_min_tiles = number("BBFMM_M2L_VARIANTS", 4);
        sw.verbose = std::getenv("BBFMM_VERBOSE") != nullptr;
        return sw;
    }
};

struct FmmTree::M2lLists {
    // per octant class: the admissible transfer vectors of a source / a target (B = V + t) in the order of stage 1 / stage 2
    std::vector<std::vector<int>> src, tgt;
    // per class: transfer vector -> its position in the list, -1: not admissible.  Valid once both axes decisions are
    // taken (index()); every stage after them reads the lists through these.
    std::vector<std::vector<int>> tpos_src, tpos_tgt;
    std::vector<std::vector<int32_t>> tgt_pair; // per target position: the partner's position (leader of a pair), -1 (single), -2 (partner)
    std::vector<std::vector<int8_t>> tgt_kind;  // 0 single, 1 member of an x pair, 2 member of a y pair
    std::vector<int> level_groups;              // per level: groups of target classes it is cut into (plan_m2l_batches)
    std::vector<std::vector<int>> batch_of;     // per level and class: its batch
    void index(int nvec) {
        for (auto *p : {&tpos_src, &tpos_tgt}) {
            const std::vector<std::vector<int>> &lists = p == &tpos_src ? src : tgt;
            p->assign(lists.size(), std::vector<int>(static_cast<size_t>(nvec), -1));
            for (size_t o = 0; o < lists.size(); ++o)
                for (size_t i = 0; i < lists[o].size(); ++i) (*p)[o][static_cast<size_t>(lists[o][i])] = static_cast<int>(i);
        }
    }
};

// Slot layout of the targets of one level, per class: one segment per admissible transfer vector.
// With the pairs of stage 2 the slot is [A | B | S]: the leaders' segments, padded to kp (a multiple of 16); their
// partners' at the same offsets behind them; the singles.  Step q of the pair region contracts the 16 values at 16 q
// and the 16 at kp + 16 q; a vector's rows stay contiguous, so stage 1 stores as before.
// Two axes: the list is [x pairs | y pairs | singles]; the first y leader starts at kpy = the x leaders' length rounded up
// to 16, so that a contraction step holds pairs of one kind (kpy = kp when there are no y pairs).
struct FmmTree::M2lSlotLayout {
    std::vector<std::vector<int>> off_tgt; // per class and target position: offset of the segment in the slot
    std::vector<int> k_pad, kp, kpy, pad;  // per class: slot length, length of A, the y boundary in A, entries left empty before it
};

struct FmmTree::M2lPairSplit {
    std::vector<size_t> x, y, singles; // list positions; a pair is two consecutive entries, leader first
};

struct FmmTree::M2lStage1Marks {
    std::vector<int32_t> pair; // per position: partner's position (first of a pair), -1 (single), -2 (second of a pair)
    std::vector<int8_t> kind;  // 0 single, 1 x pair, 2 y pair
    std::vector<int32_t> row0; // first stacked row of every position that owns rows
    int rows = 0;              // stacked rows
    int y_blk = -1;            // first column block of a y pair, -1: none
    int pad_rows = 0;          // rows left empty so that the y pairs start a block of their own
};

struct FmmTree::M2lTargetOrder {
    std::vector<std::vector<int>> tgt;
    std::vector<std::vector<int32_t>> pair;
    std::vector<std::vector<int8_t>> kind;
    std::vector<M2lSlotLayout> layout; // per level (from 2)
    int64_t work = 0;                  // contraction steps x column groups over the level classes
};

struct FmmTree::M2lLevel {
    int level;
    size_t first_class; // of the level in m2l_host_
    const M2lLists &lists;
    const M2lSlotLayout &lay;
};

struct FmmTree::M2lBuildState {
    std::vector<int32_t> pos_in_class;                      // per cell: its position in the cell list of its class
    std::vector<std::vector<M2lTileDesc>> tiles1_of_batch;  // stage-1 tiles; level_class < 0: variant -1 - level_class
    std::vector<int32_t> variant_batch;                     // batch of every entry of m2l_variants_
    std::vector<std::vector<int32_t>> zero_of_batch;        // (slot / 2, length / 2) of the absent pairs' segments
    int64_t bad_pairs = 0;                                  // V pairs outside the admissible set
};

namespace {
inline int tv_comp(const Operators &ops, int tv, int a) { return ops.all_vecs[static_cast<size_t>(tv) * ops.d + a]; }

// octant class of the target B = V + t of a source V of class o
int target_class(const Operators &ops, int o, int tv) {
    int oc = 0;
    for (int a = 0; a < ops.d; ++a) {
        const int v = ((o >> a) & 1) + tv_comp(ops, tv, a);
        oc |= (((v % 2) + 2) % 2) << a;
    }
    return oc;
}

M2lTileDesc m2l_tile(int32_t level_class, int32_t first, int32_t count, int32_t pad, int32_t q_first = 0, int32_t q_count = 0) {
    M2lTileDesc td;
    std::memset(&td, 0, sizeof td);
    td.level_class = level_class;
    td.first = first;
    td.count = count;
    td.pad = pad;
    td.q_first = q_first;
    td.q_count = q_count;
    return td;
}

// The four parts ee, eo, oe, oo of the two-axis parity basis: h = ceil(p / 2) even and f = floor(p / 2) odd representatives
// per axis, p2 nodes per (i0, i1).
struct M2lParts {
    int p, p2, h, f, len[4];
    explicit M2lParts(const Operators &ops) : p(ops.p), p2(ops.n / (ops.p * ops.p)), h((ops.p + 1) / 2), f(ops.p / 2) {
        const int l[4] = {h * h * p2, h * f * p2, f * h * p2, f * f * p2};
        std::copy(l, l + 4, len);
    }
};

// Orbits of the nodes under {rho_x, rho_y}: for every representative (i0, i1, r) and every part it has a member in,
// entry index(part, j) of the tables (j: its number among the part's representatives) gets the up to four nodes m,
// rho_x m, rho_y m, rho_x rho_y m (-1: the node lies on a centre plane and is its own reflection) and their signs in the
// part; part_of (may be NULL) the part.  Entries no representative reaches stay padding (-1, 0, -1).
template <class Index>
void m2l_orbit_tables(const M2lParts &q, int n_index, Index index, std::vector<int32_t> *node, std::vector<int8_t> *sign, std::vector<int8_t> *part_of) {
    node->assign(static_cast<size_t>(n_index) * 4, -1);
    sign->assign(static_cast<size_t>(n_index) * 4, 0);
    if (part_of) part_of->assign(static_cast<size_t>(n_index), -1);
    for (int i0 = 0; i0 < q.h; ++i0)
        for (int i1 = 0; i1 < q.h; ++i1)
            for (int r = 0; r < q.p2; ++r) {
                const bool cx = i0 >= q.f, cy = i1 >= q.f;
                const int r0 = q.p - 1 - i0, r1 = q.p - 1 - i1; // the reflected digits
                const int nodes[4] = {(i0 * q.p + i1) * q.p2 + r, (r0 * q.p + i1) * q.p2 + r, (i0 * q.p + r1) * q.p2 + r, (r0 * q.p + r1) * q.p2 + r};
                const int je = (i0 * q.h + i1) * q.p2 + r, jo = (i0 * q.f + i1) * q.p2 + r;
                for (int part = 0; part < 4; ++part) {
                    const bool ox = part >= 2, oy = part & 1; // odd along x / y
                    if ((ox && cx) || (oy && cy)) continue;
                    const size_t k = static_cast<size_t>(index(part, oy ? jo : je));
                    if (part_of) (*part_of)[k] = static_cast<int8_t>(part);
                    for (int g = 0; g < 4; ++g) {
                        const bool gx = g & 1, gy = g & 2; // the node reflected along x / y
                        if ((gx && cx) || (gy && cy)) continue;
                        (*node)[4 * k + g] = nodes[g];
                        (*sign)[4 * k + g] = static_cast<int8_t>(((gx && ox) != (gy && oy)) ? -1 : 1);
                    }
                }
            }
}
} // namespace

// Writes: every table and scalar build_m2l_tables() produces, back to empty.
void FmmTree::clear_m2l_tables() {
    m2l_host_.clear();
    m2l_variants_.clear();
    m2l_tiles1_h_.clear();
    m2l_tile_idx1_h_.clear();
    m2l_classes_h_.clear();
    m2l_tiles_h_.clear();
    m2l_tiles2_h_.clear();
    m2l_qlist_h_.clear();
    m2l_batches_.clear();
    m2l_batch_of_class_.clear();
    m2l_group_ops_.clear();
    cbuf_batch_len_ = 0;
    cbuf_total_len_ = 0;
    m2l_flops_k1_ = 0;
    m2l_flops_level_.clear();
}

// Reflected pairs.  t and R t (component `axis` negated) use the same reference operator, and their permutations differ
// by the node reflection rho of that axis: invperm_{Rt}[m] = invperm_t[rho m], hence Vt_{Rt}[kk][m] = Vt_t[kk][rho m]
// (stage 1) and UAll_Rt[kk][i] = U_ref[kk][invperm_Rt[i]] = UAll_t[kk][rho i] (stage 2), the same reference entries bit
// for bit.  The identity is checked here for every candidate; a pair that fails it stays two singles.  Per transfer
// vector: R t, or -1.
std::vector<int32_t> FmmTree::m2l_reflection_partners(int axis) const {
    const int d = ops_.d, n = ops_.n, nvec = ops_.n_vec;
    std::vector<int32_t> partner(static_cast<size_t>(nvec), -1);
    for (int tv = 0; tv < nvec && (m2l_pairs_ || m2l_pairs2_); ++tv) {
        if (tv_comp(ops_, tv, axis) == 0) continue;
        int rt = -1;
        for (int u = 0; u < nvec && rt < 0; ++u) {
            bool same = true;
            for (int a = 0; a < d; ++a) same = same && tv_comp(ops_, u, a) == (a == axis ? -1 : 1) * tv_comp(ops_, tv, a);
            if (same) rt = u;
        }
        if (rt < 0 || ops_.ref_lookup[rt] != ops_.ref_lookup[tv]) continue;
        const int32_t *it = &ops_.invperm[static_cast<size_t>(ops_.perm_lookup[tv]) * n];
        const int32_t *ir = &ops_.invperm[static_cast<size_t>(ops_.perm_lookup[rt]) * n];
        bool ok = true;
        for (int m = 0; m < n && ok; ++m) ok = ir[m] == it[axis == 0 ? m2l_rho(m) : m2l_rho_y(m)];
        if (ok) partner[static_cast<size_t>(tv)] = rt;
    }
    return partner;
}

// Writes: m2l_pairs_, m2l_pairs2_, m2l_s1_block_, m2l_ne_, m2l_no_, m2l_ne16_, m2l_npar_ (the one-axis basis),
// m2l_s2_plan_ (the one-axis plan), m2l_partner_, m2l_partner_y_.
void FmmTree::init_m2l_parity_basis(const M2lSwitches &sw) {
    const bool can_pair = ops_.compression != kCompressionNone && !shared_basis_ && d_ >= 2 && ops_.p >= 2;
    m2l_pairs_ = sw.s1_pairs && can_pair;
    m2l_pairs2_ = sw.s2_pairs && can_pair;
    m2l_s1_block_ = m2l_pairs_ ? kM2lS1BlockPairs : kM2lS1Block;
    const int p1 = ops_.n / ops_.p;
    m2l_ne_ = (ops_.p + 1) / 2 * p1;
    m2l_no_ = ops_.p / 2 * p1;
    m2l_ne16_ = round_up(m2l_ne_, 16);
    m2l_npar_ = m2l_ne16_ + round_up(m2l_no_, 16);
    m2l_s2_plan_ = m2l_s2_pairs_plan(m2l_ne16_ / 16, round_up(m2l_no_, 16) / 16);
    m2l_partner_ = m2l_reflection_partners(0);
    // along axis 1 only vectors that no x pair of the list at hand holds pair up (m2l_split_pairs)
    m2l_partner_y_ = m2l_reflection_partners(1);
}

// The pairing pass that every ordering shares.  x pairs: t and R_x t both in the list and verified, the member with
// t0 > 0 first, in the order the walk meets their first member; y pairs (with_y): the same along axis 1 among the
// positions no x pair holds; singles: the rest in list order.  The order of the unpaired positions among themselves is
// the list's, so the split of a list is also the split of the same list with its x pairs moved to the front.
FmmTree::M2lPairSplit FmmTree::m2l_split_pairs(const std::vector<int> &list, bool with_y) const {
    const size_t nl = list.size();
    std::vector<int> where(static_cast<size_t>(ops_.n_vec), -1);
    for (size_t i = 0; i < nl; ++i) where[static_cast<size_t>(list[i])] = static_cast<int>(i);
    std::vector<uint8_t> used(nl, 0);
    M2lPairSplit ps;
    for (int pass = 0; pass < (with_y ? 2 : 1); ++pass) {
        const std::vector<int32_t> &partner = pass == 0 ? m2l_partner_ : m2l_partner_y_;
        std::vector<size_t> &dst = pass == 0 ? ps.x : ps.y;
        for (size_t i = 0; i < nl; ++i) {
            if (used[i]) continue;
            const int tv = list[i], rt = partner[static_cast<size_t>(tv)];
            const int j = rt >= 0 ? where[static_cast<size_t>(rt)] : -1;
            if (j < 0 || used[static_cast<size_t>(j)] || partner[static_cast<size_t>(rt)] != tv) continue;
            const bool lead = tv_comp(ops_, tv, pass) > 0;
            dst.push_back(lead ? i : static_cast<size_t>(j));
            dst.push_back(lead ? static_cast<size_t>(j) : i);
            used[i] = used[static_cast<size_t>(j)] = 1;
        }
    }
    for (size_t i = 0; i < nl; ++i)
        if (!used[i]) ps.singles.push_back(i);
    return ps;
}

// A source list in stage-1 order: [x pairs | singles], with two axes [x pairs | singles | y pairs] (R t directly behind
// t).  `carry` (may be NULL) is permuted along with the list.
void FmmTree::m2l_order_stage1(bool with_y, std::vector<int> *list, std::vector<int> *carry) const {
    M2lPairSplit ps = m2l_split_pairs(*list, with_y);
    std::vector<size_t> &order = ps.x;
    order.insert(order.end(), ps.singles.begin(), ps.singles.end());
    order.insert(order.end(), ps.y.begin(), ps.y.end());
    for (std::vector<int> *v : {list, carry}) {
        if (!v) continue;
        std::vector<int> permuted(order.size());
        for (size_t i = 0; i < order.size(); ++i) permuted[i] = (*v)[order[i]];
        v->swap(permuted);
    }
}

// Pairs of a source list by adjacency (an x pair: Rt directly behind t; with two axes a y pair the same way; a variant or
// a group operator that lost one of the two keeps the other as a single), and the stacked rows of the list at `level`:
// every vector that owns rows starts at an even row (the scatter stores pairs of adjacent rows as 16 bytes).  The
// kernel's slot table holds kM2lSlotWindow list positions per column block: where the ranks are so low that a block would
// span more (160 columns of rank-2 pairs: 160 positions), the next vector starts a new block and the rest of the old one
// stays padding.  A column block walks the contraction in one order, so the first y pair starts a new block when the
// block at hand holds columns of an x pair (the singles between them fill the straddling block where there are enough).
FmmTree::M2lStage1Marks FmmTree::m2l_mark_stage1(int level, int axes, const std::vector<int> &tvs) const {
    const auto &lops = ops_.m2l[level];
    M2lStage1Marks mk;
    mk.pair.assign(tvs.size(), -1);
    mk.kind.assign(tvs.size(), 0);
    mk.row0.assign(tvs.size(), 0);
    for (size_t pos = 0; m2l_pairs_ && pos + 1 < tvs.size(); ++pos) {
        const size_t a = static_cast<size_t>(tvs[pos]), b = static_cast<size_t>(tvs[pos + 1]);
        const bool px = m2l_partner_[a] == tvs[pos + 1] && m2l_partner_[b] == tvs[pos];
        const bool py = !px && axes == 2 && m2l_partner_y_[a] == tvs[pos + 1] && m2l_partner_y_[b] == tvs[pos];
        if (px || py) {
            mk.pair[pos] = static_cast<int32_t>(pos + 1);
            mk.pair[pos + 1] = -2;
            mk.kind[pos] = mk.kind[pos + 1] = px ? 1 : 2;
            ++pos;
        }
    }
    int rows = 0, blk = -1, blk_first = 0; // blk_first: first list position with rows in block blk
    int last_x_blk = -1;
    for (size_t pos = 0; pos < tvs.size(); ++pos) {
        if (mk.pair[pos] == -2) continue;
        const int r = lops[ops_.ref_lookup[tvs[pos]]].rank;
        if (r == 0) continue;
        if (mk.kind[pos] == 2 && mk.y_blk < 0) {
            if (rows / m2l_s1_block_ <= last_x_blk) {
                mk.pad_rows = round_up(rows, m2l_s1_block_) - rows;
                rows += mk.pad_rows;
            }
            mk.y_blk = rows / m2l_s1_block_;
        }
        const int last = mk.pair[pos] >= 0 ? static_cast<int>(pos) + 1 : static_cast<int>(pos);
        if (rows / m2l_s1_block_ == blk && last - blk_first + 1 > kM2lSlotWindow) rows = round_up(rows, m2l_s1_block_);
        mk.row0[pos] = rows;
        const int b1 = (rows + r - 1) / m2l_s1_block_; // the last block the vector's rows reach
        if (rows / m2l_s1_block_ != blk || b1 != blk) {
            blk = b1;
            blk_first = static_cast<int>(pos); // (also of a block the vector only reaches into: it is the first there)
        }
        if (mk.kind[pos] == 1) last_x_blk = b1;
        rows = round_up(rows + r, 2);
    }
    mk.rows = rows;
    return mk;
}

std::vector<uint8_t> FmmTree::m2l_classes_present(int level) const { // per class: whether the level has a cell of it
    std::vector<uint8_t> has(size_t(1) << d_, 0);
    for (int64_t c = tree_.level_ptr[level]; c < tree_.level_ptr[level + 1]; ++c) has[tree_.octant[c]] = 1;
    return has;
}

// BBFMM_M2L_S1_AXES: 1 the x pairs alone, 2 also the y pairs; unset: by executed work, the sum over the level classes of
// column blocks x contraction steps -- two axes only where that is strictly smaller (the four parts pad to 16 each: at
// low orders that costs more steps than the pairs save columns).
// Writes: m2l_axes_, m2l_work_, m2l_s1_off_, m2l_s_ee_, m2l_s_eo_, m2l_par_node_, m2l_par_sign_; with two axes m2l_ne16_
// (now the x-even parts ee + eo) and m2l_npar_ (all four parts).  lists->src: in the order of the picked layout.
void FmmTree::choose_m2l_stage1_axes(const M2lSwitches &sw, M2lLists *lists) {
    m2l_axes_ = 1;
    m2l_s_ee_ = m2l_s_eo_ = 0;
    m2l_s1_off_ = M2lParityOffsets{{0, m2l_ne16_, m2l_ne16_, m2l_npar_}};
    m2l_work_[0] = m2l_work_[1] = 0;
    m2l_par_node_.clear();
    m2l_par_sign_.clear();
    if (!m2l_pairs_) return;
    const M2lParts q(ops_);
    M2lParityOffsets off2{{0, 0, 0, 0}};
    for (int i = 1; i < 4; ++i) off2.v[i] = off2.v[i - 1] + round_up(q.len[i - 1], 16);
    const int npar2 = off2.v[3] + round_up(q.len[3], 16);
    std::vector<std::vector<int>> src_x = lists->src, src_xy = lists->src; // the two candidates
    for (size_t o = 0; o < src_x.size(); ++o) {
        m2l_order_stage1(false, &src_x[o], nullptr);
        m2l_order_stage1(true, &src_xy[o], nullptr);
    }
    auto blocks = [&](int rows) { return static_cast<int64_t>(round_up(std::max(rows, 1), m2l_s1_block_) / m2l_s1_block_); };
    for (int level = 2; level <= tree_.depth; ++level) {
        const std::vector<uint8_t> has = m2l_classes_present(level);
        for (size_t o = 0; o < has.size(); ++o) {
            if (!has[o]) continue;
            m2l_work_[0] += blocks(m2l_mark_stage1(level, 1, src_x[o]).rows) * (m2l_npar_ / 16);
            m2l_work_[1] += blocks(m2l_mark_stage1(level, 2, src_xy[o]).rows) * (npar2 / 16);
        }
    }
    const bool two = sw.s1_axes == 2 || (sw.s1_axes != 1 && m2l_work_[1] < m2l_work_[0]);
    lists->src = std::move(two ? src_xy : src_x);
    if (!two) return;
    m2l_axes_ = 2;
    m2l_s1_off_ = off2;
    m2l_ne16_ = off2.v[2];
    m2l_npar_ = npar2;
    m2l_s_ee_ = off2.v[1] / 16;
    m2l_s_eo_ = (off2.v[2] - off2.v[1]) / 16;
    // basis index -> the nodes of its orbit under {rho_x, rho_y} and their signs (device: m2l_parity2_kernel)
    m2l_orbit_tables(q, npar2, [&](int part, int j) { return off2.v[part] + j; }, &m2l_par_node_, &m2l_par_sign_, nullptr);
}

// The target lists of every class in the order of stage 2 with `axes` reflection axes (0: no pairs, the lists as they
// are; 1: [x pairs | singles]; 2: [x pairs | y pairs | singles], R t directly behind t), their marks, and the slot layout
// of every level under that order.
FmmTree::M2lTargetOrder FmmTree::m2l_target_order(const std::vector<std::vector<int>> &tgt, int axes) const {
    M2lTargetOrder to;
    const size_t ncls = tgt.size();
    to.tgt.resize(ncls);
    to.pair.resize(ncls);
    to.kind.resize(ncls);
    for (size_t o = 0; o < ncls; ++o) {
        if (axes == 0) {
            to.tgt[o] = tgt[o];
            to.pair[o].assign(tgt[o].size(), -1);
            to.kind[o].assign(tgt[o].size(), 0);
            continue;
        }
        const M2lPairSplit ps = m2l_split_pairs(tgt[o], axes == 2);
        for (int part = 0; part < 3; ++part) {
            const std::vector<size_t> &src = part == 0 ? ps.x : part == 1 ? ps.y : ps.singles;
            for (size_t i = 0; i < src.size(); ++i) {
                const int32_t pos = static_cast<int32_t>(to.tgt[o].size());
                to.tgt[o].push_back(tgt[o][src[i]]);
                to.pair[o].push_back(part == 2 ? -1 : (i & 1) ? -2 : pos + 1);
                to.kind[o].push_back(static_cast<int8_t>(part == 2 ? 0 : part + 1));
            }
        }
    }
    to.layout.resize(static_cast<size_t>(tree_.depth) + 1);
    for (int level = 2; level <= tree_.depth; ++level) to.layout[static_cast<size_t>(level)] = m2l_slot_layout(level, to);
    return to;
}

FmmTree::M2lSlotLayout FmmTree::m2l_slot_layout(int level, const M2lTargetOrder &to) const {
    const auto &lops = ops_.m2l[level];
    const size_t ncls = to.tgt.size();
    M2lSlotLayout lay;
    lay.off_tgt.assign(ncls, {});
    for (auto *v : {&lay.k_pad, &lay.kp, &lay.kpy, &lay.pad}) v->assign(ncls, 0);
    for (size_t o = 0; o < ncls; ++o) {
        const std::vector<int> &tl = to.tgt[o];
        auto seg = [&](size_t pos) { return round_up(lops[ops_.ref_lookup[tl[pos]]].rank, 2); }; // 16-byte aligned segments
        int lead = 0, lead_y = 0;
        bool has_y = false;
        for (size_t pos = 0; pos < tl.size(); ++pos)
            if (to.pair[o][pos] >= 0) {
                (to.kind[o][pos] == 2 ? lead_y : lead) += seg(pos);
                has_y = has_y || to.kind[o][pos] == 2;
            }
        const int kp = has_y ? round_up(round_up(lead, 16) + lead_y, 16) : round_up(lead, 16);
        const int kpy = has_y ? round_up(lead, 16) : kp;
        int off = 0, off_s = 2 * kp;
        bool in_y = false;
        for (size_t pos = 0; pos < tl.size(); ++pos) {
            if (to.pair[o][pos] >= 0) {
                if (to.kind[o][pos] == 2 && !in_y) { // the first y leader
                    off = kpy;
                    in_y = true;
                }
                lay.off_tgt[o].push_back(off);
            } else if (to.pair[o][pos] == -2) {
                lay.off_tgt[o].push_back(kp + off);
                off += seg(pos);
            } else {
                lay.off_tgt[o].push_back(off_s);
                off_s += seg(pos);
            }
        }
        lay.k_pad[o] = round_up(std::max(off_s, 16), 16);
        lay.kp[o] = kp;
        lay.kpy[o] = kpy;
        lay.pad[o] = has_y ? kpy - lead : 0;
    }
    return lay;
}

// BBFMM_M2L_S2_AXES: 1 the x pairs alone, 2 also the y pairs of the vectors that x leaves alone; unset: by executed work,
// the sum over the level classes of contraction steps x column groups (padding included) -- two axes only where that is
// strictly smaller.
// Writes: m2l_s2_axes_, m2l_s2_work_, m2l_s2_node_, m2l_s2_sign_, m2l_s2_part_; with two axes m2l_s2_plan_.
// lists->tgt, tgt_pair, tgt_kind: the picked order; *layouts: its slot layout per level.
void FmmTree::choose_m2l_stage2_axes(const M2lSwitches &sw, M2lLists *lists, std::vector<M2lSlotLayout> *layouts) {
    m2l_s2_axes_ = 1;
    m2l_s2_work_[0] = m2l_s2_work_[1] = 0;
    m2l_s2_node_.clear();
    m2l_s2_sign_.clear();
    m2l_s2_part_.clear();
    M2lTargetOrder one = m2l_target_order(lists->tgt, m2l_pairs2_ ? 1 : 0), two;
    bool pick_two = false;
    if (m2l_pairs2_) {
        const M2lParts q(ops_);
        int grp[4];
        for (int i = 0; i < 4; ++i) grp[i] = std::max(1, round_up(q.len[i], 16) / 16);
        const M2lS2PairsPlan plan2 = m2l_s2_pairs_plan2(grp);
        two = m2l_target_order(lists->tgt, 2);
        auto work_of = [&](const M2lTargetOrder &to, int groups) {
            int64_t w = 0;
            for (int level = 2; level <= tree_.depth; ++level) {
                const std::vector<uint8_t> has = m2l_classes_present(level);
                const M2lSlotLayout &lay = to.layout[static_cast<size_t>(level)];
                for (size_t o = 0; o < has.size(); ++o)
                    if (has[o]) w += static_cast<int64_t>((lay.k_pad[o] - lay.kp[o]) / 16) * groups;
            }
            return w;
        };
        m2l_s2_work_[0] = work_of(one, m2l_s2_plan_.n_par() / 16);
        m2l_s2_work_[1] = work_of(two, plan2.n_par() / 16);
        pick_two = sw.s2_axes == 2 || (sw.s2_axes != 1 && m2l_s2_work_[1] < m2l_s2_work_[0]);
        if (pick_two) {
            m2l_s2_axes_ = 2;
            m2l_s2_plan_ = plan2;
            // column of Lp / the operators -> the nodes of its orbit under {rho_x, rho_y}, their signs, its part
            m2l_orbit_tables(q, plan2.n_par(), [&](int part, int j) { return plan2.col(part, j); }, &m2l_s2_node_, &m2l_s2_sign_, &m2l_s2_part_);
        }
    }
    M2lTargetOrder &pick = pick_two ? two : one;
    lists->tgt = std::move(pick.tgt);
    lists->tgt_pair = std::move(pick.pair);
    lists->tgt_kind = std::move(pick.kind);
    *layouts = std::move(pick.layout);
}

// ---- batches.  The slots of all targets (one per cell, sum_t r_t doubles: 37 KB at order 7) are what the two
// stages exchange -- 10.9 GB per right-hand side at 10M points, 76 GB for the finest level of an 80M-point tree.
// They go through one buffer of at most m2l_budget_bytes_: consecutive levels share a batch while they fit; a
// level that does not fit alone is cut into 2, 4 or 8 groups of target classes, and the sources of that level
// get one stacked stage-1 operator per group (the transfer vectors that end in the group's classes: the same
// tables over fewer transfer vectors, like the boundary variants).
// Writes: m2l_batches_ (levels and groups; len and the tile ranges come later), cbuf_total_len_.
// lists->level_groups, lists->batch_of.
void FmmTree::plan_m2l_batches(const M2lSwitches &sw, const std::vector<M2lSlotLayout> &layouts, M2lLists *lists) {
    const HostTree &t = tree_;
    const int ncls = 1 << d_;
    lists->level_groups.assign(static_cast<size_t>(t.depth) + 1, 1);
    lists->batch_of.assign(static_cast<size_t>(t.depth) + 1, std::vector<int>(ncls, -1));
    const int64_t budget = std::max<int64_t>(m2l_budget_bytes_ / 8 - 128, 1);
    int64_t cur_len = 0;
    for (int level = 2; level <= t.depth; ++level) {
        std::vector<int64_t> class_len(ncls, 0);
        for (int64_t c = t.level_ptr[level]; c < t.level_ptr[level + 1]; ++c) class_len[t.octant[c]] += layouts[static_cast<size_t>(level)].k_pad[t.octant[c]];
        int64_t len = 0;
        for (int64_t v : class_len) len += v;
        cbuf_total_len_ += len;
        int G = 1;
        if (len > budget)
            for (G = 2; G < ncls; G *= 2) {
                int64_t worst = 0;
                for (int g = 0; g < G; ++g) {
                    int64_t gl = 0;
                    for (int o = g * ncls / G; o < (g + 1) * ncls / G; ++o) gl += class_len[o];
                    worst = std::max(worst, gl);
                }
                if (worst <= budget) break;
            }
        if (G >= ncls) { // one group per class is the finest cut there is: the largest class may still not fit
            G = ncls;
            const int64_t worst = *std::max_element(class_len.begin(), class_len.end());
            if (worst > budget && sw.verbose)
                std::fprintf(stderr, "[bbfmm] warning: level %d needs %.1f MB of M2L intermediate per right-hand side even "
                                     "with one batch per target class; the budget of %.1f MB (BBFMM_M2L_CBUF_MB) is exceeded\n",
                             level, worst * 8.0 / 1048576.0, m2l_budget_bytes_ / 1048576.0);
        }
        lists->level_groups[level] = G;
        if (G == 1 && !m2l_batches_.empty() && m2l_batches_.back().groups == 1 && cur_len + len <= budget) {
            m2l_batches_.back().level_hi = level; // shares the batch of the level above
            cur_len += len;
            for (int o = 0; o < ncls; ++o) lists->batch_of[level][o] = static_cast<int>(m2l_batches_.size()) - 1;
            continue;
        }
        for (int g = 0; g < G; ++g) {
            M2lBatch b;
            b.level_lo = b.level_hi = level;
            b.groups = G;
            b.group = g;
            for (int o = g * ncls / G; o < (g + 1) * ncls / G; ++o) lists->batch_of[level][o] = static_cast<int>(m2l_batches_.size());
            m2l_batches_.push_back(b);
        }
        cur_len = len;
    }
}

// ---- per level: the classes, their cells and slots, the tiles of stage 2, the operators and tiles of stage 1

// The cells of the level into the lists of their classes, ordered by V-list pattern (complete lists first, equal patterns
// together, Morton order inside a pattern): the 128-cell tiles then hold cells that miss the same transfer vectors
// (domain boundary, coarse neighbours), which lets stage 2 skip the contraction steps no cell of a tile needs.
// Writes: cells of the level's classes in m2l_host_; st->pos_in_class of the level's cells.
void FmmTree::sort_m2l_class_cells(const M2lLevel &lv, M2lBuildState *st) {
    const HostTree &t = tree_;
    const int64_t c_lo = t.level_ptr[lv.level], c_hi = t.level_ptr[lv.level + 1];
    for (int64_t c = c_lo; c < c_hi; ++c) m2l_host_[lv.first_class + t.octant[c]].cells.push_back(static_cast<int32_t>(c));
    std::vector<uint64_t> key(static_cast<size_t>(c_hi - c_lo));
    for (int64_t c = c_lo; c < c_hi; ++c) {
        uint64_t hsh = 1469598103934665603ull;
        const int64_t nv = t.v.ptr[c + 1] - t.v.ptr[c];
        uint64_t bits[6] = {0, 0, 0, 0, 0, 0}; // presence over the 7^d transfer vectors
        for (int64_t q = t.v.ptr[c]; q < t.v.ptr[c + 1]; ++q) {
            const int tv = t.v_tidx[q];
            if (tv >= 0 && tv < 384) bits[tv >> 6] |= 1ull << (tv & 63);
        }
        for (uint64_t b : bits) hsh = (hsh ^ b) * 1099511628211ull;
        // complete lists first; the hash only has to keep equal patterns together
        key[static_cast<size_t>(c - c_lo)] = (static_cast<uint64_t>(1023 - std::min<int64_t>(nv, 1023)) << 54) | (hsh >> 10);
    }
    std::vector<int32_t> &pos_in_class = st->pos_in_class;
    parallel_for(int64_t(1) << d_, 1, [&](int64_t o) { // the classes are disjoint cell sets
        auto &cells = m2l_host_[lv.first_class + static_cast<size_t>(o)].cells;
        std::stable_sort(cells.begin(), cells.end(), [&](int32_t a, int32_t b) {
            return key[static_cast<size_t>(a - c_lo)] < key[static_cast<size_t>(b - c_lo)];
        });
        for (size_t i = 0; i < cells.size(); ++i) pos_in_class[cells[i]] = static_cast<int32_t>(i);
    });
}

// Stage-1 row tables of a class-o operator stacked over the transfer vectors `tvs` (the whole admissible list for the
// class itself, fewer for a boundary variant or a group operator); the rows point at the slot offsets of the targets'
// classes (lv.lay through lv.lists.tpos_tgt).  false: a slot too long for the packed row table.
// Writes: *hc (n_t, the src_* lists, the row tables, yb0, pad_cols); m2l_max_blocks_, m2l_slot_t_ (their maxima).
bool FmmTree::m2l_stage1_rows(const M2lLevel &lv, int o, const std::vector<int> &tvs, HostM2lClass *hcp) {
    HostM2lClass &hc = *hcp;
    const auto &lops = ops_.m2l[lv.level];
    auto rank_of = [&](int tv) { return lops[ops_.ref_lookup[tv]].rank; };
    auto slot_off = [&](int tv) {
        const int oc = target_class(ops_, o, tv);
        return lv.lay.off_tgt[oc][lv.lists.tpos_tgt[oc][tv]];
    };
    M2lStage1Marks mk = m2l_mark_stage1(lv.level, m2l_axes_, tvs);
    hc.n_t = static_cast<int>(tvs.size());
    hc.n_rows = mk.rows;
    hc.src_pair = std::move(mk.pair);
    hc.src_kind = std::move(mk.kind);
    hc.pad_cols = mk.pad_rows;
    hc.r_pad16 = round_up(std::max(hc.n_rows, 1), m2l_s1_block_);
    hc.yb0 = mk.y_blk >= 0 ? mk.y_blk : hc.r_pad16 / m2l_s1_block_; // no y pairs: every block walks in x order
    hc.row_tpos.assign(hc.r_pad16, -1);
    hc.row_off.assign(hc.r_pad16, 0);
    hc.row_tpos2.assign(hc.r_pad16, -1);
    hc.row_off2.assign(hc.r_pad16, 0);
    hc.src_tv = tvs;
    int row = 0;
    hc.src_row0.assign(tvs.size(), 0);
    hc.src_row1.assign(tvs.size(), 0);
    for (size_t pos = 0; pos < tvs.size(); ++pos) {
        if (hc.src_pair[pos] == -2) { // the rows of the first of the pair
            hc.src_row0[pos] = hc.src_row0[pos - 1];
            hc.src_row1[pos] = hc.src_row1[pos - 1];
            continue;
        }
        const int tv = tvs[pos];
        const int base_off = slot_off(tv), base_off2 = hc.src_pair[pos] >= 0 ? slot_off(tvs[pos + 1]) : 0;
        if (rank_of(tv) > 0) row = mk.row0[pos];
        hc.src_row0[pos] = row;
        for (int kk = 0; kk < rank_of(tv); ++kk, ++row) {
            hc.row_tpos[row] = static_cast<int32_t>(pos);
            hc.row_off[row] = base_off + kk;
            if (hc.src_pair[pos] >= 0) {
                hc.row_tpos2[row] = static_cast<int32_t>(pos + 1);
                hc.row_off2[row] = base_off2 + kk;
            }
        }
        hc.src_row1[pos] = row;
        row = round_up(row, 2); // the padding row keeps tpos -1 (never stored on its own)
    }
    // per column block: first transfer-vector position, and the packed row table
    const int n_blk = hc.r_pad16 / m2l_s1_block_;
    m2l_max_blocks_ = std::max(m2l_max_blocks_, n_blk);
    hc.blk_t0.assign(n_blk, 0);
    hc.row_dst.assign(hc.r_pad16, -1);
    hc.row_dst2.assign(hc.r_pad16, -1);
    for (int b = 0; b < n_blk; ++b) {
        int t0 = -1, t1 = -1;
        bool two = false; // some column of the block has a second destination
        for (int r = b * m2l_s1_block_; r < (b + 1) * m2l_s1_block_; ++r) {
            if (hc.row_tpos[r] < 0) continue;
            if (t0 < 0) t0 = hc.row_tpos[r];
            t1 = std::max(hc.row_tpos[r], hc.row_tpos2[r]); // (positions ascend with the rows; a partner is pos + 1)
            two = two || hc.row_tpos2[r] >= 0;
        }
        if (t0 < 0) continue;
        hc.blk_t0[b] = t0 | (two ? kM2lBlkTwoDst : 0);
        m2l_slot_t_ = std::max(m2l_slot_t_, t1 - t0 + 1);
        for (int r = b * m2l_s1_block_; r < (b + 1) * m2l_s1_block_; ++r) {
            if (hc.row_tpos[r] < 0) continue;
            if (hc.row_off[r] >= (1 << 24) || hc.row_off2[r] >= (1 << 24)) return false;
            hc.row_dst[r] = ((hc.row_tpos[r] - t0) << 24) | hc.row_off[r];
            if (hc.row_tpos2[r] >= 0) hc.row_dst2[r] = ((hc.row_tpos2[r] - t0) << 24) | hc.row_off2[r];
        }
    }
    return true;
}

// The classes of the level: their lists, marks and slot lengths, the stage-1 rows over the whole source list, the slot
// base of every cell (relative to the class's batch) and cslot cleared to -1.
// Writes: the level's entries of m2l_host_ (all but cells and the cslot values); len of the level's batches.
int FmmTree::fill_m2l_classes(const M2lLevel &lv) {
    const M2lLists &ls = lv.lists;
    for (int o = 0; o < (1 << d_); ++o) {
        HostM2lClass &hc = m2l_host_[lv.first_class + o];
        hc.level = lv.level;
        hc.octant = o;
        hc.k_pad = lv.lay.k_pad[o];
        hc.kp = lv.lay.kp[o];
        hc.kpy = lv.lay.kpy[o];
        hc.tgt_pad = lv.lay.pad[o];
        hc.tgt_pair = ls.tgt_pair[o];
        hc.tgt_kind = ls.tgt_kind[o];
        if (!m2l_stage1_rows(lv, o, ls.src[o], &hc)) return fail(BBFMM_BAD_ARGUMENT, "M2L slot too long for the packed row table");
        if (hc.cells.empty()) continue;
        hc.tgt_tv = ls.tgt[o];
        hc.tgt_off = lv.lay.off_tgt[o];
        if (host_only_) fill_m2l_operator_arrays(hc, &hc.vt_all, &hc.u_all);
        hc.cbase.resize(hc.cells.size());
        int64_t &cursor = m2l_batches_[static_cast<size_t>(ls.batch_of[lv.level][o])].len; // slot addresses are relative to the batch
        for (size_t i = 0; i < hc.cells.size(); ++i) {
            hc.cbase[i] = cursor;
            cursor += hc.k_pad;
        }
        hc.cslot.resize(hc.cells.size() * static_cast<size_t>(hc.n_t));
        int32_t *cs = hc.cslot.data();
        parallel_for_chunks(static_cast<int64_t>(hc.cslot.size()), int64_t(1) << 18, [&](int64_t b, int64_t e) {
            std::fill(cs + b, cs + e, int32_t(-1));
        });
    }
    return BBFMM_OK;
}

// cslot: for every V pair (B <- V, t) the slot of B as seen from V (threaded: every (V, t) slot has exactly one writer;
// flop and error counts are reduced per chunk, in a fixed order).
// Writes: the cslot values of the level's classes; m2l_flops_k1_, m2l_flops_level_[level]; st->bad_pairs.
void FmmTree::fill_m2l_cslot(const M2lLevel &lv, M2lBuildState *st) {
    const HostTree &t = tree_;
    const int n = ops_.n, nvec = ops_.n_vec, level = lv.level;
    const bool compressed = ops_.compression != kCompressionNone;
    const auto &lops = ops_.m2l[level];
    const M2lLists &ls = lv.lists;
    const std::vector<int32_t> &pos_in_class = st->pos_in_class;
    const int64_t b0 = t.level_ptr[level], nb_cells = t.level_ptr[level + 1] - b0;
    constexpr int64_t kChunkB = 2048;
    const int64_t nch = (nb_cells + kChunkB - 1) / kChunkB;
    std::vector<double> flops_part(static_cast<size_t>(std::max<int64_t>(nch, 1)), 0.0);
    std::vector<int64_t> bad_part(static_cast<size_t>(std::max<int64_t>(nch, 1)), 0);
    parallel_for_chunks(nb_cells, kChunkB, [&](int64_t lo, int64_t hi) {
        double fl = 0.0;
        int64_t bad = 0;
        for (int64_t B = b0 + lo; B < b0 + hi; ++B) {
            const HostM2lClass &hb = m2l_host_[lv.first_class + t.octant[B]];
            const int64_t base = hb.cbase[pos_in_class[B]];
            for (int64_t q = t.v.ptr[B]; q < t.v.ptr[B + 1]; ++q) {
                const int32_t V = t.v.idx[q];
                const int tv = t.v_tidx[q];
                HostM2lClass &hv = m2l_host_[lv.first_class + t.octant[V]];
                const int ps = (tv >= 0 && tv < nvec) ? ls.tpos_src[t.octant[V]][tv] : -1;
                if (ps < 0 || t.level[V] != level || ls.tpos_tgt[t.octant[B]][tv] < 0) {
                    ++bad;
                    continue;
                }
                hv.cslot[static_cast<size_t>(pos_in_class[V]) * hv.n_t + ps] = static_cast<int32_t>(base / 2);
                fl += compressed ? 4.0 * n * lops[ops_.ref_lookup[tv]].rank : 2.0 * n * static_cast<double>(n);
            }
        }
        flops_part[static_cast<size_t>(lo / kChunkB)] = fl;
        bad_part[static_cast<size_t>(lo / kChunkB)] = bad;
    });
    double level_flops = 0.0;
    for (double f : flops_part) level_flops += f; // fixed order: same total on every run
    m2l_flops_k1_ += level_flops;
    if (m2l_flops_level_.size() <= static_cast<size_t>(level)) m2l_flops_level_.resize(static_cast<size_t>(level) + 1, 0.0);
    m2l_flops_level_[static_cast<size_t>(level)] = level_flops;
    for (int64_t b : bad_part) st->bad_pairs += b;
}

// Batches share one buffer, so a slot segment whose pair does not exist (domain boundary, coarser neighbour) holds
// another batch's values when stage 2 reads it: such segments are zeroed before every pass (launch_m2l_zero_segments).
// A single batch keeps the zeros the buffer was allocated with.  Appends to st->zero_of_batch.
void FmmTree::m2l_zero_segments(const M2lLevel &lv, M2lBuildState *st) const {
    const HostTree &t = tree_;
    const auto &lops = ops_.m2l[lv.level];
    for (int o = 0; o < (1 << d_); ++o) {
        const HostM2lClass &hc = m2l_host_[lv.first_class + o];
        const std::vector<int> &tl = lv.lists.tgt[o], &tpos = lv.lists.tpos_tgt[o];
        std::vector<int32_t> &zs = st->zero_of_batch[static_cast<size_t>(lv.lists.batch_of[lv.level][o])];
        std::vector<uint8_t> present(tl.size());
        for (size_t i = 0; i < hc.cells.size(); ++i) {
            const int64_t B = hc.cells[i];
            std::fill(present.begin(), present.end(), uint8_t(0));
            for (int64_t q = t.v.ptr[B]; q < t.v.ptr[B + 1]; ++q) {
                const int tv = t.v_tidx[q];
                const int pos = tv >= 0 && tv < ops_.n_vec ? tpos[tv] : -1;
                if (pos >= 0) present[static_cast<size_t>(pos)] = 1;
            }
            for (size_t pos = 0; pos < present.size(); ++pos)
                if (!present[pos]) {
                    zs.push_back(static_cast<int32_t>((hc.cbase[i] + lv.lay.off_tgt[o][pos]) / 2));
                    zs.push_back(round_up(lops[ops_.ref_lookup[tl[pos]]].rank, 2) / 2);
                }
        }
    }
}

// The stage-2 tiles of the level's classes, each with the contraction steps (16 slot entries) that hold at least one
// V-list entry of the tile.  Appends to m2l_tiles_h_ and m2l_qlist_h_.
void FmmTree::m2l_stage2_tiles(const M2lLevel &lv) {
    const HostTree &t = tree_;
    const auto &lops = ops_.m2l[lv.level];
    for (int o = 0; o < (1 << d_); ++o) {
        const HostM2lClass &hc = m2l_host_[lv.first_class + o];
        const std::vector<int> &tpos = lv.lists.tpos_tgt[o], &off_tgt = lv.lay.off_tgt[o];
        const int nq = (hc.k_pad - hc.kp) / 16; // steps of the operator's rows (a pair step serves both members)
        const int32_t nc = static_cast<int32_t>(hc.cells.size());
        const int64_t n_tiles_cls = (static_cast<int64_t>(nc) + kM2lTile - 1) / kM2lTile;
        std::vector<std::vector<uint16_t>> tile_q(static_cast<size_t>(n_tiles_cls));
        parallel_for(n_tiles_cls, 4, [&](int64_t ti) {
            const int32_t first = static_cast<int32_t>(ti * kM2lTile), count = std::min<int32_t>(kM2lTile, nc - first);
            std::vector<uint8_t> act(static_cast<size_t>(nq), 0);
            for (int32_t i = 0; i < count; ++i) {
                const int64_t B = hc.cells[first + i];
                for (int64_t q = t.v.ptr[B]; q < t.v.ptr[B + 1]; ++q) {
                    const int tv = t.v_tidx[q];
                    const int pos = tpos[tv];
                    if (pos < 0) continue;
                    const int a = off_tgt[pos] - (off_tgt[pos] >= hc.kp ? hc.kp : 0), b = a + lops[ops_.ref_lookup[tv]].rank; // operator rows
                    for (int sq = a / 16; sq <= (b - 1) / 16; ++sq) act[sq] = 1;
                }
            }
            for (int sq = 0; sq < nq; ++sq)
                if (act[sq]) tile_q[static_cast<size_t>(ti)].push_back(static_cast<uint16_t>(sq));
        });
        for (int64_t ti = 0; ti < n_tiles_cls; ++ti) {
            const std::vector<uint16_t> &tq = tile_q[static_cast<size_t>(ti)];
            const int32_t first = static_cast<int32_t>(ti * kM2lTile);
            m2l_tiles_h_.push_back(m2l_tile(static_cast<int32_t>(lv.first_class + o), first, std::min<int32_t>(kM2lTile, nc - first), 0,
                                            static_cast<int32_t>(m2l_qlist_h_.size()), static_cast<int32_t>(tq.size())));
            m2l_qlist_h_.insert(m2l_qlist_h_.end(), tq.begin(), tq.end());
        }
    }
}

// The stage-1 operator of the source class `hc` restricted to the transfer vectors tvs = hc.src_tv[keep[.]], for the
// `count` cells from class position `first`: the same reference operators over fewer transfer vectors (gathered on the
// device), its row tables, and the kept columns of the cells' cslot rows.  false: see m2l_stage1_rows.
bool FmmTree::m2l_restricted_operator(const M2lLevel &lv, const HostM2lClass &hc, const std::vector<int> &tvs, const std::vector<int> &keep,
                                      size_t first, size_t count, HostM2lClass *v) {
    v->level = lv.level;
    v->octant = hc.octant;
    v->k_pad = 16;
    if (!m2l_stage1_rows(lv, hc.octant, tvs, v)) return false;
    v->cells.assign(hc.cells.begin() + static_cast<std::ptrdiff_t>(first), hc.cells.begin() + static_cast<std::ptrdiff_t>(first + count));
    const size_t nk = keep.size(), nt = static_cast<size_t>(hc.n_t);
    v->cslot.resize(count * nk);
    int32_t *dst = v->cslot.data();
    const int32_t *src = hc.cslot.data() + first * nt;
    parallel_for_chunks(static_cast<int64_t>(count), 4096, [&](int64_t lo, int64_t hi) {
        for (int64_t k = lo; k < hi; ++k)
            for (size_t q = 0; q < nk; ++q) dst[static_cast<size_t>(k) * nk + q] = src[static_cast<size_t>(k) * nt + keep[q]];
    });
    if (host_only_) fill_m2l_operator_arrays(*v, &v->vt_all, &v->u_all);
    return true;
}

// A level cut into groups of target classes: per (group, source class) one stacked operator over the transfer vectors
// whose targets lie in the group, all cells of the class as its tiles.
// Writes: appends to m2l_variants_, m2l_group_ops_ of the level's classes; st->tiles1_of_batch, st->variant_batch.
int FmmTree::m2l_group_operators(const M2lLevel &lv, M2lBuildState *st) {
    const int ncls = 1 << d_, G = lv.lists.level_groups[lv.level];
    for (int g = 0; g < G; ++g) {
        const int o_lo = g * ncls / G, o_hi = (g + 1) * ncls / G;
        const int bidx = lv.lists.batch_of[lv.level][o_lo];
        for (int o = 0; o < ncls; ++o) {
            const HostM2lClass &hc = m2l_host_[lv.first_class + o];
            const size_t nc = hc.cells.size();
            if (nc == 0) continue;
            std::vector<int> tvs, keep;
            for (int ps = 0; ps < hc.n_t; ++ps) {
                const int oc = target_class(ops_, o, hc.src_tv[ps]);
                if (oc >= o_lo && oc < o_hi) {
                    tvs.push_back(hc.src_tv[ps]);
                    keep.push_back(ps);
                }
            }
            if (tvs.empty()) continue;
            if (m2l_axes_ == 2) m2l_order_stage1(true, &tvs, &keep); // (t and R_y t end in the same target class, hence group)
            HostM2lClass v;
            if (!m2l_restricted_operator(lv, hc, tvs, keep, 0, nc, &v)) return fail(BBFMM_BAD_ARGUMENT, "M2L slot too long for the packed row table");
            const int32_t id = -1 - static_cast<int32_t>(m2l_variants_.size()); // fixed up in finish_m2l_launch_lists
            for (size_t f = 0; f < nc; f += kM2lTile)
                st->tiles1_of_batch[static_cast<size_t>(bidx)].push_back(m2l_tile(id, static_cast<int32_t>(f), static_cast<int32_t>(std::min<size_t>(kM2lTile, nc - f)), 0));
            m2l_group_ops_[lv.first_class + o].push_back(static_cast<int32_t>(m2l_variants_.size()));
            st->variant_batch.push_back(bidx);
            m2l_variants_.push_back(std::move(v));
        }
    }
    return BBFMM_OK;
}

// ---- stage-1 variants (boundary classes) of a level in one batch.  A source cell computes the compressed vectors of ALL
// admissible transfer vectors of its class, also of those whose target does not exist (domain boundary, coarse
// neighbours): 6 % of the stage-1 flops of a uniform cube, far more on clustered data.  Cells of a class are sorted by
// V-list pattern, so cells that miss the same targets sit together: a run of at least sw.variant_min_tiles (default 4: a
// variant costs setup time -- tables, one more operator -- that only a long run of tiles earns back) full tiles of such
// cells gets its own stacked operator with the missing transfer vectors left out; the remaining cells keep the class
// operator.  Only the unrestricted stage 1 (the matvec) uses the variants; plans keep the class tables.
// Writes: appends to m2l_variants_, m2l_tile_idx1_h_; st->tiles1_of_batch, st->variant_batch.
int FmmTree::m2l_boundary_variants(const M2lLevel &lv, const M2lSwitches &sw, M2lBuildState *st) {
    for (int o = 0; o < (1 << d_); ++o) {
        const HostM2lClass &hc = m2l_host_[lv.first_class + o];
        const size_t nc = hc.cells.size();
        if (nc == 0) continue;
        const int nt = hc.n_t, bidx = lv.lists.batch_of[lv.level][o];
        std::vector<M2lTileDesc> &tiles1_out = st->tiles1_of_batch[static_cast<size_t>(bidx)];
        // pattern signature per cell (which targets exist)
        std::vector<uint64_t> sig(nc);
        parallel_for(static_cast<int64_t>(nc), 256, [&](int64_t i) {
            uint64_t h = 1469598103934665603ull;
            const int32_t *row = &hc.cslot[static_cast<size_t>(i) * nt];
            uint64_t word = 0;
            for (int ps = 0; ps < nt; ++ps) {
                word = (word << 1) | (row[ps] >= 0 ? 1u : 0u);
                if ((ps & 63) == 63 || ps == nt - 1) {
                    h = (h ^ word) * 1099511628211ull;
                    word = 0;
                }
            }
            sig[static_cast<size_t>(i)] = h;
        });
        auto same_pattern = [&](size_t a, size_t b) {
            if (sig[a] != sig[b]) return false;
            const int32_t *ra = &hc.cslot[a * nt], *rb = &hc.cslot[b * nt];
            for (int ps = 0; ps < nt; ++ps)
                if ((ra[ps] >= 0) != (rb[ps] >= 0)) return false;
            return true;
        };
        auto n_pairs = [](const std::vector<int32_t> &m) { return std::count_if(m.begin(), m.end(), [](int32_t v) { return v >= 0; }); };
        std::vector<int32_t> rest; // class positions that keep the class operator
        for (size_t i = 0, j; i < nc; i = j) {
            for (j = i + 1; j < nc && same_pattern(i, j);) ++j;
            size_t full = 0;
            if (sw.variant_min_tiles > 0 && j - i >= static_cast<size_t>(sw.variant_min_tiles) * kM2lTile) {
                std::vector<int> tvs, keep;
                for (int ps = 0; ps < nt; ++ps)
                    if (hc.cslot[i * nt + ps] >= 0) {
                        tvs.push_back(hc.src_tv[ps]);
                        keep.push_back(ps);
                    }
                // (two axes: vectors whose x partner is absent may pair along y among themselves)
                if (m2l_axes_ == 2) m2l_order_stage1(true, &tvs, &keep);
                const M2lStage1Marks present = m2l_mark_stage1(lv.level, m2l_axes_, tvs);
                // worth a variant: at least one column block saved -- or, in the parity basis, pairs that lost their
                // partner (the cells of an x face): no columns go, but the blocks of the singles that remain issue
                // one store per column instead of two (the epilogue is bound by the number of stores)
                if (!tvs.empty() && (round_up(present.rows, m2l_s1_block_) < hc.r_pad16 || n_pairs(present.pair) < n_pairs(hc.src_pair))) {
                    full = (j - i) / kM2lTile * kM2lTile;
                    HostM2lClass v;
                    if (!m2l_restricted_operator(lv, hc, tvs, keep, i, full, &v)) return fail(BBFMM_BAD_ARGUMENT, "M2L slot too long for the packed row table");
                    const int32_t id = -1 - static_cast<int32_t>(m2l_variants_.size()); // fixed up in finish_m2l_launch_lists
                    for (size_t f = 0; f < full; f += kM2lTile) tiles1_out.push_back(m2l_tile(id, static_cast<int32_t>(f), kM2lTile, 0));
                    st->variant_batch.push_back(bidx);
                    m2l_variants_.push_back(std::move(v));
                }
            }
            for (size_t k = i + full; k < j; ++k) rest.push_back(static_cast<int32_t>(k));
        }
        for (size_t f = 0; f < rest.size(); f += kM2lTile) // pad = 1: first indexes the position list
            tiles1_out.push_back(m2l_tile(static_cast<int32_t>(lv.first_class + o), static_cast<int32_t>(m2l_tile_idx1_h_.size() + f),
                                          static_cast<int32_t>(std::min<size_t>(kM2lTile, rest.size() - f)), 1));
        m2l_tile_idx1_h_.insert(m2l_tile_idx1_h_.end(), rest.begin(), rest.end());
    }
    return BBFMM_OK;
}

int FmmTree::build_m2l_level(const M2lLevel &lv, const M2lSwitches &sw, M2lBuildState *st) {
    m2l_host_.resize(lv.first_class + (size_t(1) << d_));
    m2l_group_ops_.resize(m2l_host_.size());
    sort_m2l_class_cells(lv, st);
    CHK(fill_m2l_classes(lv));
    fill_m2l_cslot(lv, st);
    if (m2l_batches_.size() > 1) m2l_zero_segments(lv, st);
    m2l_stage2_tiles(lv);
    return lv.lists.level_groups[lv.level] > 1 ? m2l_group_operators(lv, st) : m2l_boundary_variants(lv, sw, st);
}

// The device class table (level classes, then variants / group operators; every entry works for one batch) and the
// launch lists, batch by batch: stage 1 from the per-batch lists, stage 2 = the class tiles (the classes of a batch are
// consecutive) with the tail of every batch split; the zero lists; the buffer length.
// Writes: m2l_batch_of_class_, m2l_tiles1_h_, m2l_tiles2_h_, the tile ranges of m2l_batches_, m2l_zero_h_, m2l_zero_ptr_,
// cbuf_batch_len_.
int FmmTree::finish_m2l_launch_lists(const M2lLists &lists, const M2lBuildState &st) {
    if (st.bad_pairs > 0)
        return fail(BBFMM_UNSUPPORTED,
                    "V-list pairs outside the admissible transfer-vector set (source points outside the root box?)");
    m2l_batch_of_class_.assign(m2l_host_.size() + m2l_variants_.size(), 0);
    for (size_t lc = 0; lc < m2l_host_.size(); ++lc)
        m2l_batch_of_class_[lc] = lists.batch_of[static_cast<size_t>(m2l_host_[lc].level)][static_cast<size_t>(m2l_host_[lc].octant)];
    for (size_t v = 0; v < m2l_variants_.size(); ++v) m2l_batch_of_class_[m2l_host_.size() + v] = st.variant_batch[v];
    size_t next = 0;
    for (size_t b = 0; b < m2l_batches_.size(); ++b) {
        M2lBatch &mb = m2l_batches_[b];
        mb.t1_first = static_cast<int32_t>(m2l_tiles1_h_.size());
        for (M2lTileDesc td : st.tiles1_of_batch[b]) {
            if (td.level_class < 0) td.level_class = static_cast<int32_t>(m2l_host_.size()) + (-1 - td.level_class);
            m2l_tiles1_h_.push_back(td);
        }
        mb.t1_count = static_cast<int32_t>(m2l_tiles1_h_.size()) - mb.t1_first;
        std::vector<M2lTileDesc> part;
        while (next < m2l_tiles_h_.size() && m2l_batch_of_class_[static_cast<size_t>(m2l_tiles_h_[next].level_class)] == static_cast<int32_t>(b))
            part.push_back(m2l_tiles_h_[next++]);
        split_tile_tail(&part, n_cu_);
        mb.t2_first = static_cast<int32_t>(m2l_tiles2_h_.size());
        mb.t2_count = static_cast<int32_t>(part.size());
        m2l_tiles2_h_.insert(m2l_tiles2_h_.end(), part.begin(), part.end());
        cbuf_batch_len_ = std::max(cbuf_batch_len_, mb.len);
    }
    if (next != m2l_tiles_h_.size()) return fail(BBFMM_DEVICE_ERROR, "internal: M2L tiles out of batch order");
    m2l_zero_h_.clear();
    m2l_zero_ptr_.assign(m2l_batches_.size() + 1, 0);
    for (size_t b = 0; b < m2l_batches_.size(); ++b) {
        m2l_zero_h_.insert(m2l_zero_h_.end(), st.zero_of_batch[b].begin(), st.zero_of_batch[b].end());
        m2l_zero_ptr_[b + 1] = static_cast<int64_t>(m2l_zero_h_.size() / 2);
    }
    cbuf_batch_len_ += 128; // + dump area for the branch-free stage-1 scatter (never read)
    if (cbuf_batch_len_ / 2 >= (int64_t(1) << 31))
        return fail(BBFMM_UNSUPPORTED, "M2L intermediate buffer of one batch too large (raise the number of groups: lower BBFMM_M2L_CBUF_MB)");
    return BBFMM_OK;
}

int FmmTree::build_m2l_tables() {
    clear_m2l_tables();
    if (tree_.depth < 2) return BBFMM_OK;
    const M2lSwitches sw = M2lSwitches::read();
    // budget of the intermediate: a sixteenth of the device's memory (18 GiB on a 288 GB MI355X: the slots of one
    // right-hand side of a 10M-point tree fit at orders 7 and 9), at least 4 GiB; 16 GiB without a device
    if (!host_only_) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0)
            m2l_budget_bytes_ = std::max<int64_t>(int64_t(4) << 30, static_cast<int64_t>(total_b / 16));
    }
    if (sw.cbuf_mb > 0) m2l_budget_bytes_ = static_cast<int64_t>(sw.cbuf_mb * 1048576.0);
    init_m2l_parity_basis(sw);
    // admissible transfer vectors per class (B = V + t, both children of neighbouring parents), far ones only
    const int ncls = 1 << d_;
    M2lLists lists;
    lists.src.resize(ncls);
    lists.tgt.resize(ncls);
    for (int o = 0; o < ncls; ++o)
        for (int tv = 0; tv < ops_.n_vec; ++tv) {
            int mx = 0;
            bool okt = true, oks = true;
            for (int a = 0; a < d_; ++a) {
                const int oa = (o >> a) & 1, ta = tv_comp(ops_, tv, a);
                mx = std::max(mx, std::abs(ta));
                okt = okt && ta >= oa - 3 && ta <= oa + 2;
                oks = oks && ta >= -2 - oa && ta <= 3 - oa;
            }
            if (mx >= 2 && okt) lists.tgt[o].push_back(tv);
            if (mx >= 2 && oks) lists.src[o].push_back(tv);
        }
    std::vector<M2lSlotLayout> layouts; // per level, under the picked order of the target lists
    choose_m2l_stage1_axes(sw, &lists);
    choose_m2l_stage2_axes(sw, &lists, &layouts);
    lists.index(ops_.n_vec);
    plan_m2l_batches(sw, layouts, &lists);
    M2lBuildState st;
    st.pos_in_class.assign(static_cast<size_t>(tree_.n_cells()), -1);
    st.tiles1_of_batch.resize(m2l_batches_.size());
    st.zero_of_batch.resize(m2l_batches_.size());
    for (int level = 2; level <= tree_.depth; ++level)
        CHK(build_m2l_level(M2lLevel{level, m2l_host_.size(), lists, layouts[static_cast<size_t>(level)]}, sw, &st));
    return finish_m2l_launch_lists(lists, st);
}

} // namespace bbfmm
