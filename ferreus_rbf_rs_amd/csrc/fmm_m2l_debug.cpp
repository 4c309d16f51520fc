// FmmTree: the read-only test hooks of the M2L tables.  See fmm_tree.hpp.
#include "fmm_tree_impl.hpp"

#include <type_traits>

namespace bbfmm {

namespace {
// 64-bit FNV-1a over the bytes of integers; a vector contributes its length before its elements
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    template <class T> void put(T v) {
        static_assert(std::is_integral<T>::value, "integer tables only");
        unsigned char b[sizeof(T)];
        std::memcpy(b, &v, sizeof(T));
        for (unsigned char c : b) h = (h ^ c) * 1099511628211ull;
    }
    template <class V> void vec(const V &v) {
        put(static_cast<uint64_t>(v.size()));
        for (auto x : v) put(x);
    }
    void tiles(const std::vector<M2lTileDesc> &v) {
        put(static_cast<uint64_t>(v.size()));
        for (const M2lTileDesc &t : v) {
            put(t.level_class);
            put(t.first);
            put(t.count);
            put(t.q_first);
            put(t.q_count);
            put(t.pad);
        }
    }
};
} // namespace

// Test hook: see fmm_tree.hpp for the families and their order.
void FmmTree::debug_m2l_table_digests(std::vector<uint64_t> *out) const {
    Fnv f[kM2lDigestFamilies];
    { // 0: scalars
        Fnv &s = f[0];
        s.put<int32_t>(m2l_pairs_);
        s.put<int32_t>(m2l_pairs2_);
        for (int v : {m2l_axes_, m2l_s2_axes_, m2l_ne_, m2l_no_, m2l_ne16_, m2l_npar_}) s.put<int32_t>(v);
        for (int32_t v : m2l_s1_off_.v) s.put(v);
        for (int v : {m2l_s_ee_, m2l_s_eo_, m2l_s1_block_, m2l_slot_t_, m2l_max_blocks_}) s.put<int32_t>(v);
        for (int64_t v : {m2l_work_[0], m2l_work_[1], m2l_s2_work_[0], m2l_s2_work_[1]}) s.put(v);
        for (int v : {m2l_s2_plan_.ga, m2l_s2_plan_.gb, m2l_s2_plan_.ce, m2l_s2_plan_.co, m2l_s2_plan_.ya, m2l_s2_plan_.yb}) s.put<int32_t>(v);
        s.put(cbuf_batch_len_);
        s.put(cbuf_total_len_);
    }
    f[1].vec(m2l_partner_);
    f[1].vec(m2l_partner_y_);
    f[1].vec(m2l_par_node_);
    f[1].vec(m2l_par_sign_);
    f[1].vec(m2l_s2_node_);
    f[1].vec(m2l_s2_sign_);
    f[1].vec(m2l_s2_part_);
    f[2].put(static_cast<uint64_t>(m2l_host_.size()));
    f[2].put(static_cast<uint64_t>(m2l_variants_.size()));
    for (size_t i = 0; i < m2l_host_.size() + m2l_variants_.size(); ++i) {
        const HostM2lClass &h = i < m2l_host_.size() ? m2l_host_[i] : m2l_variants_[i - m2l_host_.size()];
        f[2].vec(h.src_tv);
        f[2].vec(h.src_pair);
        f[2].vec(h.src_kind);
        f[2].vec(h.src_row0);
        f[2].vec(h.src_row1);
        f[2].vec(h.tgt_tv);
        f[2].vec(h.tgt_off);
        f[2].vec(h.tgt_pair);
        f[2].vec(h.tgt_kind);
        for (int v : {h.level, h.octant, h.n_rows, h.r_pad16, h.n_t, h.k_pad, h.yb0, h.pad_cols, h.kp, h.kpy, h.tgt_pad}) f[2].put<int32_t>(v);
        f[3].vec(h.row_dst);
        f[3].vec(h.row_dst2);
        f[3].vec(h.blk_t0);
        f[3].vec(h.row_tpos);
        f[3].vec(h.row_off);
        f[3].vec(h.row_tpos2);
        f[3].vec(h.row_off2);
        f[4].vec(h.cells);
        f[4].vec(h.cbase);
        f[4].vec(h.cslot);
    }
    f[5].tiles(m2l_tiles1_h_);
    f[5].vec(m2l_tile_idx1_h_);
    f[6].tiles(m2l_tiles_h_);
    f[6].tiles(m2l_tiles2_h_);
    f[6].vec(m2l_qlist_h_);
    f[7].put(static_cast<uint64_t>(m2l_batches_.size()));
    for (const M2lBatch &b : m2l_batches_) {
        for (int v : {b.level_lo, b.level_hi, b.groups, b.group}) f[7].put<int32_t>(v);
        f[7].put(b.len);
        for (int32_t v : {b.t1_first, b.t1_count, b.t2_first, b.t2_count}) f[7].put(v);
    }
    f[7].vec(m2l_batch_of_class_);
    f[7].put(static_cast<uint64_t>(m2l_group_ops_.size()));
    for (const std::vector<int32_t> &g : m2l_group_ops_) f[7].vec(g);
    f[7].vec(m2l_zero_h_);
    f[7].vec(m2l_zero_ptr_);
    out->clear();
    for (const Fnv &x : f) out->push_back(x.h);
}

// Test hook: apply the stacked M2L tables on the host (plain loops).  Validates the table
// construction without a GPU; never reached from a compute entry point.
int FmmTree::debug_apply_m2l_tables_host(const double *M, double *L) const {
    const int n = ops_.n, n_pad = round_up(n, 32);
    // the multipoles in the parity basis, as the device's change-of-basis pass writes them: [M_e | pad | M_o | pad]
    std::vector<double> Mp;
    if (m2l_pairs_) {
        Mp.assign(static_cast<size_t>(tree_.n_cells()) * m2l_npar_, 0.0);
        for (int64_t c = 0; c < tree_.n_cells(); ++c) {
            const double *Mv = M + static_cast<size_t>(c) * n;
            double *mp = &Mp[static_cast<size_t>(c) * m2l_npar_];
            for (int k = 0; m2l_axes_ == 2 && k < m2l_npar_; ++k) // [M_ee | M_eo | M_oe | M_oo]: the signed sums over the orbits
                for (int g = 0; g < 4; ++g)
                    if (m2l_par_node_[static_cast<size_t>(4 * k + g)] >= 0)
                        mp[k] += m2l_par_sign_[static_cast<size_t>(4 * k + g)] * Mv[m2l_par_node_[static_cast<size_t>(4 * k + g)]];
            for (int j = 0; m2l_axes_ == 1 && j < m2l_ne_; ++j) {
                if (j < m2l_no_) {
                    mp[j] = Mv[j] + Mv[m2l_rho(j)];
                    mp[m2l_ne16_ + j] = Mv[j] - Mv[m2l_rho(j)];
                } else {
                    mp[j] = Mv[j];
                }
            }
        }
    }
    // exactly as the unrestricted device launches walk them: batch by batch through ONE buffer of the largest
    // batch's length (slot addresses are relative to the batch), stage 1 over the batch's tile list (boundary
    // variants, group operators), stage 2 over the classes of the batch.  The buffer is NOT cleared between batches:
    // what the zero-fill lists do not reset is left as the previous batch wrote it, like on the device.
    std::vector<double> cbuf(static_cast<size_t>(std::max<int64_t>(cbuf_batch_len_, 1)), 0.0);
    std::vector<int32_t> seen(static_cast<size_t>(tree_.n_cells()), 0);
    const bool have_zero_lists = m2l_batches_.size() > 1 && !m2l_zero_h_.empty();
    for (size_t b = 0; b < m2l_batches_.size(); ++b) {
        const M2lBatch &mb = m2l_batches_[b];
        if (have_zero_lists)
            for (int64_t z = m2l_zero_ptr_[b]; z < m2l_zero_ptr_[b + 1]; ++z)
                std::fill(cbuf.begin() + 2 * static_cast<int64_t>(m2l_zero_h_[static_cast<size_t>(2 * z)]),
                          cbuf.begin() + 2 * (static_cast<int64_t>(m2l_zero_h_[static_cast<size_t>(2 * z)]) + m2l_zero_h_[static_cast<size_t>(2 * z + 1)]), 0.0);
        for (int32_t ti = mb.t1_first; ti < mb.t1_first + mb.t1_count; ++ti) {
            const M2lTileDesc &td = m2l_tiles1_h_[static_cast<size_t>(ti)];
            const bool variant = static_cast<size_t>(td.level_class) >= m2l_host_.size();
            const HostM2lClass &hc = variant ? m2l_variants_[static_cast<size_t>(td.level_class) - m2l_host_.size()]
                                             : m2l_host_[static_cast<size_t>(td.level_class)];
            if (hc.vt_all.empty()) return BBFMM_UNSUPPORTED; // tables were released after upload
            if (m2l_batch_of_class_[static_cast<size_t>(td.level_class)] != static_cast<int32_t>(b)) return BBFMM_BAD_ARGUMENT;
            for (int32_t q = 0; q < td.count; ++q) {
                const size_t pos = static_cast<size_t>(td.pad ? m2l_tile_idx1_h_[static_cast<size_t>(td.first + q)] : td.first + q);
                ++seen[hc.cells[pos]];
                const double *Mv = M + static_cast<size_t>(hc.cells[pos]) * n;
                for (int row = 0; row < hc.n_rows; ++row) {
                    if (hc.row_tpos[row] < 0) continue; // padding row
                    const int32_t slot = hc.cslot[pos * hc.n_t + hc.row_tpos[row]];
                    if (m2l_pairs_) { // a over the even part, b over the odd part; a + b to the row's vector, a - b to its partner
                        const int32_t slot2 = hc.row_tpos2[row] >= 0 ? hc.cslot[pos * hc.n_t + hc.row_tpos2[row]] : -1;
                        if (slot < 0 && slot2 < 0) continue;
                        const double *mp = &Mp[static_cast<size_t>(hc.cells[pos]) * m2l_npar_];
                        double a = 0.0, bsum = 0.0;
                        if (row / m2l_s1_block_ >= hc.yb0) { // a block in y order: a over the y-even parts ee and oe, b over eo and oo
                            for (int j = 0; j < m2l_npar_; ++j) {
                                const bool y_odd = (j >= m2l_s1_off_.v[1] && j < m2l_s1_off_.v[2]) || j >= m2l_s1_off_.v[3];
                                (y_odd ? bsum : a) += hc.vt_all[static_cast<size_t>(j) * hc.r_pad16 + row] * mp[j];
                            }
                        } else {
                            for (int j = 0; j < m2l_ne16_; ++j) a += hc.vt_all[static_cast<size_t>(j) * hc.r_pad16 + row] * mp[j];
                            for (int j = m2l_ne16_; j < m2l_npar_; ++j) bsum += hc.vt_all[static_cast<size_t>(j) * hc.r_pad16 + row] * mp[j];
                        }
                        if (slot >= 0) cbuf[static_cast<size_t>(slot) * 2 + hc.row_off[row]] = a + bsum;
                        if (slot2 >= 0) cbuf[static_cast<size_t>(slot2) * 2 + hc.row_off2[row]] = a - bsum;
                        continue;
                    }
                    if (slot < 0) continue;
                    double s = 0.0;
                    for (int m = 0; m < n; ++m) s += hc.vt_all[static_cast<size_t>(m) * hc.r_pad16 + row] * Mv[m];
                    cbuf[static_cast<size_t>(slot) * 2 + hc.row_off[row]] = s;
                }
            }
        }
        for (size_t lc = 0; lc < m2l_host_.size(); ++lc) {
            if (m2l_batch_of_class_[lc] != static_cast<int32_t>(b)) continue;
            const HostM2lClass &hc = m2l_host_[lc];
            for (size_t pos = 0; pos < hc.cells.size(); ++pos) {
                double *Lb = L + static_cast<size_t>(hc.cells[pos]) * n;
                const double *cc = &cbuf[static_cast<size_t>(hc.cbase[pos])];
                if (m2l_pairs2_) { // operator row r < kp: slot[r] + slot[kp + r] against U_e, their difference against U_o;
                    // r >= kp: slot[kp + r] against both; then back to the node order
                    const int n_par = m2l_s2_plan_.n_par(), ne16 = m2l_s2_plan_.ne16(), rows = hc.k_pad - hc.kp;
                    std::vector<double> sm(static_cast<size_t>(rows)), df(static_cast<size_t>(rows));
                    for (int r = 0; r < rows; ++r) {
                        sm[static_cast<size_t>(r)] = r < hc.kp ? cc[r] + cc[hc.kp + r] : cc[hc.kp + r];
                        df[static_cast<size_t>(r)] = r < hc.kp ? cc[r] - cc[hc.kp + r] : cc[hc.kp + r];
                    }
                    if (m2l_s2_axes_ == 2) { // rows below kpy: x pairs, the sum to [ee | eo], the difference to [oe | oo]; rows
                        // [kpy, kp): y pairs, the sum to [ee | oe], the difference to [eo | oo]; then the signed orbit sums back
                        for (int k = 0; k < n_par; ++k) {
                            const int part = m2l_s2_part_[static_cast<size_t>(k)];
                            if (part < 0) continue;
                            double acc = 0.0;
                            for (int r = 0; r < rows; ++r) {
                                const bool odd = r < hc.kpy ? part >= 2 : (part & 1);
                                acc += hc.u_all[static_cast<size_t>(r) * n_par + k] * (odd ? df : sm)[static_cast<size_t>(r)];
                            }
                            for (int g = 0; g < 4; ++g)
                                if (m2l_s2_node_[static_cast<size_t>(4 * k + g)] >= 0)
                                    Lb[m2l_s2_node_[static_cast<size_t>(4 * k + g)]] += m2l_s2_sign_[static_cast<size_t>(4 * k + g)] * acc;
                        }
                        continue;
                    }
                    for (int i = 0; i < m2l_ne_; ++i) {
                        double le = 0.0, lo = 0.0;
                        for (int r = 0; r < rows; ++r) {
                            le += hc.u_all[static_cast<size_t>(r) * n_par + i] * sm[static_cast<size_t>(r)];
                            // (the centre plane has no odd part: ne16 + i would lie past the row's end at order 5)
                            if (i < m2l_no_) lo += hc.u_all[static_cast<size_t>(r) * n_par + ne16 + i] * df[static_cast<size_t>(r)];
                        }
                        if (i >= m2l_no_) {
                            Lb[i] += le;
                        } else {
                            Lb[i] += le + lo;
                            Lb[m2l_rho(i)] += le - lo;
                        }
                    }
                    continue;
                }
                for (int i = 0; i < n; ++i) {
                    double s = 0.0;
                    for (int k = 0; k < hc.k_pad; ++k) s += hc.u_all[static_cast<size_t>(k) * n_pad + i] * cc[k];
                    Lb[i] += s;
                }
            }
        }
    }
    // every source cell of a level with M2L work belongs to exactly one stage-1 tile per batch of its level
    for (const HostM2lClass &hc : m2l_host_)
        for (int32_t c : hc.cells) {
            // (on a level cut into groups a class has one operator per group its transfer vectors reach -- a class
            // whose vectors miss a group has none for it, as build_downward_plan anticipates)
            const size_t lc = static_cast<size_t>(&hc - m2l_host_.data());
            const M2lBatch &mb = m2l_batches_[static_cast<size_t>(m2l_batch_of_class_[lc])];
            const int want = mb.groups == 1 || m2l_group_ops_[lc].empty() ? mb.groups : static_cast<int>(m2l_group_ops_[lc].size());
            if (seen[c] != want) return BBFMM_BAD_ARGUMENT;
        }
    return BBFMM_OK;
}

void FmmTree::debug_m2l_pairs(std::vector<int32_t> *out) const {
    out->clear();
    const int d = d_;
    for (size_t i = 0; i < m2l_host_.size() + m2l_variants_.size(); ++i) {
        const HostM2lClass &h = i < m2l_host_.size() ? m2l_host_[i] : m2l_variants_[i - m2l_host_.size()];
        if (h.cells.empty()) continue;
        out->push_back(h.level);
        out->push_back(h.octant);
        out->push_back(i < m2l_host_.size() ? 0 : 1);
        const size_t n_at = out->size();
        out->push_back(0);
        int32_t n_entries = 0;
        for (size_t pos = 0; pos < h.src_tv.size(); ++pos) { // (the members of a y pair are listed as two singles)
            const bool x_pair = h.src_pair[pos] >= 0 && h.src_kind[pos] == 1;
            if (h.src_pair[pos] == -2 && h.src_kind[pos] == 1) continue;
            out->push_back(x_pair ? 1 : 0);
            for (int a = 0; a < d; ++a) out->push_back(ops_.all_vecs[static_cast<size_t>(h.src_tv[pos]) * d + a]);
            ++n_entries;
        }
        (*out)[n_at] = n_entries;
    }
}

void FmmTree::debug_m2l_pairs_axes(std::vector<int32_t> *out) const {
    out->clear();
    const int d = d_;
    out->push_back(m2l_pairs_ ? m2l_axes_ : 0);
    out->push_back(static_cast<int32_t>(m2l_work_[0]));
    out->push_back(static_cast<int32_t>(m2l_work_[1]));
    for (size_t i = 0; i < m2l_host_.size() + m2l_variants_.size(); ++i) {
        const HostM2lClass &h = i < m2l_host_.size() ? m2l_host_[i] : m2l_variants_[i - m2l_host_.size()];
        if (h.cells.empty()) continue;
        const int n_blk = h.r_pad16 / m2l_s1_block_;
        out->push_back(h.level);
        out->push_back(h.octant);
        out->push_back(i < m2l_host_.size() ? 0 : 1);
        out->push_back(h.pad_cols);
        out->push_back(h.yb0);
        out->push_back(n_blk);
        const size_t n_at = out->size();
        out->push_back(0);
        for (int b = 0; b < n_blk; ++b) out->push_back(b >= h.yb0 ? 1 : 0);
        int32_t n_entries = 0;
        for (size_t pos = 0; pos < h.src_tv.size(); ++pos) {
            if (h.src_pair[pos] == -2) continue;
            out->push_back(h.src_pair[pos] >= 0 ? h.src_kind[pos] : 0);
            const bool rows = h.src_row1[pos] > h.src_row0[pos]; // (a vector of rank 0 owns no column: -1, -1)
            out->push_back(rows ? h.src_row0[pos] / m2l_s1_block_ : -1);
            out->push_back(rows ? (h.src_row1[pos] - 1) / m2l_s1_block_ : -1);
            for (int a = 0; a < d; ++a) out->push_back(ops_.all_vecs[static_cast<size_t>(h.src_tv[pos]) * d + a]);
            ++n_entries;
        }
        (*out)[n_at] = n_entries;
    }
}

void FmmTree::debug_m2l_pairs_stage2(std::vector<int32_t> *out) const {
    out->clear();
    const int d = d_;
    for (const HostM2lClass &h : m2l_host_) {
        if (h.cells.empty()) continue;
        out->push_back(h.level);
        out->push_back(h.octant);
        out->push_back(0);
        const size_t n_at = out->size();
        out->push_back(0);
        int32_t n_entries = 0;
        for (size_t pos = 0; pos < h.tgt_tv.size(); ++pos) { // (the members of a y pair are listed as two singles)
            const bool x_member = h.tgt_kind[pos] == 1;
            if (h.tgt_pair[pos] == -2 && x_member) continue;
            out->push_back(h.tgt_pair[pos] >= 0 && x_member ? 1 : 0);
            for (int a = 0; a < d; ++a) out->push_back(ops_.all_vecs[static_cast<size_t>(h.tgt_tv[pos]) * d + a]);
            ++n_entries;
        }
        (*out)[n_at] = n_entries;
    }
}

void FmmTree::debug_m2l_pairs_axes_stage2(std::vector<int32_t> *out) const {
    out->clear();
    const int d = d_;
    out->push_back(m2l_pairs2_ ? m2l_s2_axes_ : 0);
    out->push_back(static_cast<int32_t>(m2l_s2_work_[0]));
    out->push_back(static_cast<int32_t>(m2l_s2_work_[1]));
    for (const HostM2lClass &h : m2l_host_) {
        if (h.cells.empty()) continue;
        const auto &lops = ops_.m2l[h.level];
        out->push_back(h.level);
        out->push_back(h.octant);
        out->push_back(h.kp);
        out->push_back(h.kpy);
        out->push_back(h.k_pad);
        out->push_back(h.tgt_pad);
        const size_t n_at = out->size();
        out->push_back(0);
        int32_t n_entries = 0;
        for (size_t pos = 0; pos < h.tgt_tv.size(); ++pos) {
            if (h.tgt_pair[pos] == -2) continue;
            out->push_back(h.tgt_pair[pos] >= 0 ? h.tgt_kind[pos] : 0);
            out->push_back(h.tgt_off[pos]);
            out->push_back(h.tgt_pair[pos] >= 0 ? h.tgt_off[static_cast<size_t>(h.tgt_pair[pos])] : -1);
            out->push_back(lops[ops_.ref_lookup[h.tgt_tv[pos]]].rank);
            for (int a = 0; a < d; ++a) out->push_back(ops_.all_vecs[static_cast<size_t>(h.tgt_tv[pos]) * d + a]);
            ++n_entries;
        }
        (*out)[n_at] = n_entries;
    }
}

void FmmTree::debug_m2l_s2_plan(int32_t out[6]) const {
    const M2lS2PairsPlan &pl = m2l_s2_plan_;
    const int32_t v[6] = {pl.ga, pl.gb, pl.ce, pl.co, pl.ya, pl.yb}; // (the one-axis plan leaves ya = yb = 0)
    for (int i = 0; i < 6; ++i) out[i] = m2l_pairs2_ ? v[i] : 0;
}

} // namespace bbfmm
