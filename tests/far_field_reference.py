"""The five far-field passes (P2M, M2M, M2L, L2L, L2P), P2L and M2P in extended precision (numpy longdouble), restated from
their mathematical definitions, with the magnitude sums and the derived rounding bounds the cell-by-cell tests need.  A
plain helper module (no tests), the far-field sibling of tests/kernel_reference.py.

Everything is built from what a handle exposes (cells, leaf_sources, interaction_list, stats().center / radius,
m2l_ranks, m2l_factors) and the oracle's key arithmetic (get_center_length, get_m2l_vectors, get_permutation_lookups).
Each pass is restated ONE STEP from the data the device fed into it (P2M from points and weights, M2M from the
children's device M, M2L + L2L from the device's M and parent L, L2P from the device's leaf L): rounding never compounds
and a failure names its pass.

Conventions: node index (i0 P1 + i1) P2 + i2 with P_a = p on the axes of the tree and 1 beyond; nodes ascending,
node_i = cos(pi (p - 1 - i + 1/2) / p); S_j(x) = (2 sum_k T_k(x) T_k(node_j) - 1) / p; coefficient arrays (K, C, n).

THE BOUNDS (u = 2^-53; first order in u; every count is an upper bound on what csrc does, whatever the compiler fuses)

e_S(p), absolute error of one double-evaluated factor S_j(x), |x| <= 1 (device_common.hpp cheb_S_reg; the transfer
tables and T_k(node_j) are evaluated the same way on the host):
  x = (coord - centre) / (len / 2): two roundings, |dT_k/dx| <= k^2            -> |dT_k| <= 2 k^2 u
  T_k = 2 x T_{k-1} - T_{k-2}: local error <= u (|2 x T_{k-1}| + |T_k|) <= 3 u per step, carried to step k by
      U_{k-m}(x), |U_j| <= j + 1                                                 -> <= 3 u k (k - 1) / 2
  so |dT_k(x)| <= 3.5 k^2 u, and the same for the table T_k(node_j) (node rounded, then the recurrence)
  s = sum_k T_k(x) T_k(node_j): table and argument errors 7 u sum_{k<p} k^2 = 7 u (p-1) p (2p-1) / 6, the p products and
      p - 1 additions (p + 1) u sum |T T| <= (p + 1) p u;  S = (2 s - 1) / p: the subtraction (2p + 1) u / p, the division 1.5 u
  e_S(p) = (7/3) (p - 1) (2p - 1) + 2p + 6                                       [100 at p = 5, 1123 at p = 16]
e_dS(p), absolute error of dS_j(x) = (2/p) sum_k T'_k(x) T_k(node_j), |T'_k| <= k^2, |T''_k| <= k^2 (k^2 - 1) / 3:
  dT_k = 2 T_{k-1} + 2 x dT_{k-1} - dT_{k-2}: local error <= 2 u (2 + 2 (k-1)^2 + (k-2)^2) + 2 |dT_{k-1}| <= 13 k^2 u,
      carried as above -> 13 k^4 u / 12; the argument 2 u k^4 / 3; the table k^2 3.5 k^2 u
  e_dS(p) = (2/p) 5.25 p^5 / 5 + (2/3) (p + 2) p^2 = 2.1 p^4 + (2/3) (p + 2) p^2

A tensor entry F0 F1 F2 with factor errors e and two product roundings errs by e (|F1 F2| + |F0 F2| + |F0 F1|) +
2 |F0 F1 F2|: every pass therefore returns TWO magnitude sums per node, s_abs (the contraction with absolute values
throughout) and s_fac (the same with one factor at a time replaced by 1, summed over the tree's axes), and
  P2M   err_j <= u [(n_pts(c) + 3) s_abs_j + e_S s_fac_j]        n_pts additions, 2 products, the weight product
  M2M   err_j <= u [(3p + 3 + n_children) s_abs_j + e_S s_fac_j]  three 1-D sums of p terms, then the child sum
  L2L   err_j <= u [(3p + 3) s_abs_j + e_S s_fac_j] (+ 1 for the += into L, counted in the M2L + L2L total)
  L2P   err_t <= u [(3p + 4) s_abs_t + e_S s_fac_t], per target; a gradient component: (3p + 6) s_abs + e_S s_fac +
        e_dS s_dfac, all times 2 / len (the scale 2 / len itself and its product: the two extra roundings)
  M2L   err_j <= u 4 (n + R_c + c0) s_j, s_j = sum over the V list of |U| (|Vt| sym|perm M_s|), sym = the entry-wise
        maximum over the x and y reflections (identity, R_x, R_y, R_x R_y) of the source cell's nodes.  n + R_c: the terms
        of the two contractions (R_c = the rank columns contracted into cell c).  The factor 4 = 2 per axis: in the
        parity basis the device multiplies (V_i +- V_Ri) / 2 by (M_i +- M_Ri), whose magnitude is <= 2 |V_i| sym|M|_i
        per axis, and adds stage 2's partner terms |U_j| |z_Rt|, which are magnitudes of the node R j <= max_j s_j (so
        the M2L bound uses the cell's LARGEST s_j, for every node).  Held for every switch setting (a superset).
        c0 = 25, counted from device_m2l.hip / fmm_m2l_tables.cpp: 2 the two-level butterfly of m2l_parity2_kernel;
        2 the table combinations 0.5 (s0 +- s1) per axis (assemble_vt_parity2_kernel); 1 stage 1's epilogue a +- b;
        1 stage 2's combination of the partner slots; 1 assemble_u_parity_kernel; 1 m2l_unparity_kernel's e +- o;
        16 the parts of a split stage-2 contraction added atomically (the most m2l_s2_ksplit's automatic rule chooses;
        BBFMM_M2L_S2_KSPLIT may ask for up to 32, which no test here sets and which would add 16 to c0); 1 the L2L +=.
  P2L   err_j <= u [(n_src + a + 4) s_phi_j + (b + 4 + 8 g) s_arg_j], (a, b) = kernel_pointwise.sum_budget and s_phi,
        s_arg the sums of kernel_reference.Dense (as test_gpu_pair_kernels.py bounds a pair sum); g = max |node
        coordinate| / len covers the rounding of the node positions centre + (len / 2) node (see p2l).
  M2P   the mirror image of P2L: the sources are the Chebyshev nodes of the cells of the leaf's W list, with the device's
        M[k, cell, :n] as weights, the targets are points of the leaf.  Per target and right-hand side
        err_t <= u [(N + a + 4) s_phi_t + (b + 4 + 8 g) s_arg_t]
        N = the nodes of the whole W list (n per cell): the product with the weight and a sum of N terms in ANY order --
        m2p_kernel's slices, the tiles of 512 (DIRECT_TILE) or of 768 / 384 columns of the fused kernels, the waves of a
        job and the atomic additions of the jobs that share a target are one sum of those N terms, regrouped.  (a, b) =
        kernel_pointwise.sum_budget; 4: the differences, their squares and the sum that form r^2.  g = the largest over the
        W cells of max |node coordinate| / len(cell).  A node coordinate c + (len / 2) node_i is formed on the device from
        the double node (one rounding of the long-double node), one product and one sum (or one fused step): its absolute
        error is at most u (len + |coordinate|) <= u len (1 + g).  A W cell is a descendant of a colleague of the leaf that
        does not touch the leaf, so every target is at least len(cell) away from every node of it: the relative change of
        r^2 is at most 2 sqrt(d) u (1 + g) <= 3.47 u (1 + g), which is <= 8 u g, the term p2l carries, as soon as g >= 0.77.
        Every cell lies in the positive orthant (up to the root's margin of 1e-3), where max |coordinate| >= (len / 2) (1 +
        cos(pi / 4)) = 0.85 len: m2p asserts g >= 0.8.
        A gradient component sum_j w_j f_tj (x_t - x_j)_a takes the form tests/test_gpu_pair_kernels.py uses for pair
        gradients, u [(N + a_f + 4) s_f + (b_f + 4 + 8 g) s_xf] with s_f = sum |w| |f| |dx_a|, s_xf = sum |w| |r^2 f'| |dx_a| and
        (a_f, b_f) the budget of the factor path, PLUS u s_pos, s_pos = sum_j |w_j| |f_tj| (len + max |coordinate|) of j's cell:
        the absolute error of the node position enters dx_a itself, which may be far smaller than len (a pair sum has
        exact differences on the grid; this one does not).  The values of a gradient call use the value_g budget.
"""
import numpy as np

from kernel_reference import LD, U  # noqa: F401  (U re-exported for the tests)
from oracle import bbfmm_oracle as O

PI = LD(4) * np.arctan(LD(1))
C0_M2L = 25


def e_S(p):
    return (7.0 / 3.0) * (p - 1) * (2 * p - 1) + 2 * p + 6


def e_dS(p):
    return 2.1 * p ** 4 + (2.0 / 3.0) * (p + 2) * p * p


# ------------------------------------------------------------------ Chebyshev pieces
def nodes(p):
    i = np.arange(p - 1, -1, -1).astype(LD)
    return np.cos(PI * (i + LD(0.5)) / LD(p))


def cheb_T(p, x):
    """T_k(x) and T'_k(x), k < p, for a long-double vector x: two (len(x), p) arrays."""
    x = np.asarray(x, dtype=LD)
    T, dT = np.ones((len(x), p), dtype=LD), np.zeros((len(x), p), dtype=LD)
    if p > 1:
        T[:, 1], dT[:, 1] = x, 1
    for j in range(2, p):
        T[:, j] = 2 * x * T[:, j - 1] - T[:, j - 2]
        dT[:, j] = 2 * T[:, j - 1] + 2 * x * dT[:, j - 1] - dT[:, j - 2]
    return T, dT


def cheb_S(p, x):
    """S_j(x) and dS_j/dx: two (len(x), p) arrays."""
    T, dT = cheb_T(p, x)
    Tn = cheb_T(p, nodes(p))[0]                       # [node j, k]
    return (2 * (T @ Tn.T) - 1) / LD(p), (LD(2) / LD(p)) * (dT @ Tn.T)


def transfer_1d(p):
    """X[side][a, i] = S_i of the parent at the child's node a, the child on the low (0) or high (1) side."""
    x = nodes(p)
    return [cheb_S(p, (x - 1) / 2)[0], cheb_S(p, (x + 1) / 2)[0]]


def dense_transfer(p, d, child_index):
    """The n x n matrix [parent node, child node] of one child, multiplied out (bit a of the index <-> axis a)."""
    X = transfer_1d(p)
    acc = None
    for a in range(d):
        m = X[(child_index >> a) & 1]
        acc = m if acc is None else np.kron(acc, m)
    return acc.T


# ------------------------------------------------------------------ the tree as the handle exposes it
class Geometry:
    def __init__(self, t):
        s = t.stats()
        self.d, self.p, self.n, self.depth = int(s.d), int(s.order), int(s.n_nodes), int(s.depth)
        self.P = [self.p if a < self.d else 1 for a in range(3)]
        keys, leaf = t.cells()
        self.keys = [int(k) for k in keys]
        self.C = len(self.keys)
        self.is_leaf = leaf.astype(bool)
        centre, radius = [float(s.center[a]) for a in range(self.d)], float(s.radius)
        cl = [O.get_center_length(k, centre, radius, self.d) for k in self.keys]
        self.centres = np.array([c for c, _ in cl], dtype=np.float64).reshape(self.C, self.d)
        self.lengths = np.array([l for _, l in cl], dtype=np.float64)
        self.level = np.array([k & O.LEVEL_MASK for k in self.keys])
        self.octant = np.array([O.get_child_index(k, self.d) for k in self.keys])
        index = {k: i for i, k in enumerate(self.keys)}
        self.parent = np.array([index.get(O.get_parent(k, self.d), -1) if k & O.LEVEL_MASK else -1 for k in self.keys])
        self.children = [[] for _ in range(self.C)]
        for c, q in enumerate(self.parent):
            if q >= 0:
                self.children[q].append(c)
        self.src_ptr, self.src_idx = t.leaf_sources()
        self.lists = {w: t.interaction_list(w) for w in "UVWX"}
        self.anchor = np.array([O.decode_key(k, self.d)[0] for k in self.keys])
        # transfer index of every V pair (target anchor - source anchor, same level) and its lookups
        all_vecs, ref_vecs = O.get_m2l_vectors(self.d)
        self.perm, self.invperm, self.perm_lookup, self.ref_lookup = O.get_permutation_lookups(self.d, self.p, all_vecs, ref_vecs)
        vp, vi = self.lists["V"]
        tgt = np.repeat(np.arange(self.C), np.diff(vp))
        diff = self.anchor[tgt] - self.anchor[vi]
        assert (np.abs(diff) <= 3).all() and (self.level[tgt] == self.level[vi]).all()
        self.v_tgt, self.v_src = tgt, vi.astype(np.int64)
        self.v_tidx = ((diff + 3) * (7 ** np.arange(self.d - 1, -1, -1))).sum(axis=1)

    def points_x(self, c, pts):
        """The Chebyshev arguments of points in cell c, formed in long double from the double inputs: (m, d)."""
        return (np.asarray(pts, dtype=np.float64).astype(LD) - self.centres[c].astype(LD)) / (LD(self.lengths[c]) / 2)

    def factors(self, c, pts, deriv=False):
        """Per axis (3 of them, ones beyond the tree's) the (m, P_a) factor rows S and, with deriv, dS/dcoord."""
        x = self.points_x(c, pts)
        one = np.ones((x.shape[0], 1), dtype=LD)
        S, D = [], []
        for a in range(3):
            if a < self.d:
                s, ds = cheb_S(self.p, x[:, a])
                S.append(s)
                D.append(ds * (LD(2) / LD(self.lengths[c])))
            else:
                S.append(one)
                D.append(None)
        return (S, D) if deriv else S


def _anterpolate(F, w):
    """sum_m w[m, k] F0[m, a] F1[m, b] F2[m, c] -> (K, n)."""
    m, K = w.shape
    A = (F[0][:, :, None] * w[:, None, :]).reshape(m, -1)                    # (m, P0 K)
    B = (F[1][:, :, None] * F[2][:, None, :]).reshape(m, -1)                 # (m, P1 P2)
    out = (A.T @ B).reshape(F[0].shape[1], K, -1)
    return out.transpose(1, 0, 2).reshape(K, -1)


def _interpolate(F, Lc, P):
    """sum_j Lc[k, j] F0[m, a] F1[m, b] F2[m, c] -> (m, K)."""
    A = Lc.reshape(Lc.shape[0], *P)
    v = np.einsum("kabc,mc->mkab", A, F[2])
    v = np.einsum("mkab,mb->mka", v, F[1])
    return np.einsum("mka,ma->mk", v, F[0])


def _one_at_a_time(F, d, fn):
    """sum over the tree's axes of fn with that axis' factor replaced by ones: the s_fac of the module docstring."""
    tot = 0
    for a in range(d):
        G = list(F)
        G[a] = np.ones_like(F[a])
        tot = tot + fn(G)
    return tot


# ------------------------------------------------------------------ P2M
def p2m(geo, pts, w, cells=None):
    """{c: (M (K, n), s_abs (K, n), s_fac (K, n), n_pts)} for the leaves that hold points."""
    w = np.asarray(w, dtype=np.float64)
    w = (w[:, None] if w.ndim == 1 else w).astype(LD)
    out = {}
    for c in (np.nonzero(np.diff(geo.src_ptr) > 0)[0] if cells is None else cells):
        idx = geo.src_idx[geo.src_ptr[c]:geo.src_ptr[c + 1]]
        F = geo.factors(c, pts[idx])
        A = [np.abs(f) for f in F]
        aw = np.abs(w[idx])
        out[int(c)] = (_anterpolate(F, w[idx]), _anterpolate(A, aw), _one_at_a_time(A, geo.d, lambda G: _anterpolate(G, aw)), len(idx))
    return out


def p2m_bound(geo, s_abs, s_fac, n_pts):
    return LD(U) * ((n_pts + 3) * s_abs + e_S(geo.p) * s_fac).max(axis=-1)


# ------------------------------------------------------------------ M2M / L2L
def _transfer(vec, mats, P, forward):
    """vec (B, n) through the three 1-D transfers.  forward (M2M): out[i] = sum_a X[a, i] in[a]; else (L2L) the transpose."""
    B = vec.shape[0]
    m = [x.T if forward else x for x in mats]                     # [out index, in index]
    A = np.matmul(m[0], vec.reshape(B, P[0], P[1] * P[2]))
    A = np.matmul(m[1], A.reshape(B * m[0].shape[0], P[1], P[2]))
    A = np.matmul(A.reshape(-1, P[2]), m[2].T)
    return A.reshape(B, -1)


class Transfers:
    def __init__(self, geo):
        self.geo = geo
        X = transfer_1d(geo.p)
        self.X, self.A = X, [np.abs(x) for x in X]
        self.one = np.ones((1, 1), dtype=LD)

    def mats(self, octant, absolute):
        X = self.A if absolute else self.X
        return [X[(octant >> a) & 1] if a < self.geo.d else self.one for a in range(3)]

    def apply(self, vec, octant, forward):
        """(value, s_abs, s_fac) of one cell's (K, n) vector through the transfer of `octant`."""
        g = self.geo
        v = np.asarray(vec, dtype=np.float64).astype(LD)
        A = self.mats(octant, True)
        av = np.abs(v)
        return (_transfer(v, self.mats(octant, False), g.P, forward), _transfer(av, A, g.P, forward),
                _one_at_a_time(A, g.d, lambda G: _transfer(av, G, g.P, forward)))


def m2m(geo, xf, M_dev, parent, terms=None):
    """(M (K, n), bound (K,)) of one parent from its children's device M (K, C, n).  terms: the summation count of the
    code under test where it is not the device's 3p + 3 (the oracle multiplies by the dense matrix: n + 3)."""
    tot = [0, 0, 0]
    for ch in geo.children[parent]:
        for i, v in enumerate(xf.apply(M_dev[:, ch], geo.octant[ch], True)):
            tot[i] = tot[i] + v
    nch = len(geo.children[parent])
    terms = 3 * geo.p + 3 if terms is None else terms
    return tot[0], LD(U) * ((terms + nch) * tot[1] + e_S(geo.p) * tot[2]).max(axis=-1)


def l2l(geo, xf, L_dev, child, terms=None):
    """(term (K, n), bound (K,)) of L2L into one child from the device's parent L (terms as in m2m)."""
    v, s_abs, s_fac = xf.apply(L_dev[:, geo.parent[child]], geo.octant[child], False)
    terms = 3 * geo.p + 3 if terms is None else terms
    return v, LD(U) * (terms * s_abs + e_S(geo.p) * s_fac).max(axis=-1)


# ------------------------------------------------------------------ M2L
def sym_abs(geo, M):
    """|M| symmetrised over the x and y reflections of the nodes: (..., n)."""
    A = np.abs(M).reshape(*M.shape[:-1], *geo.P)
    A = np.maximum(A, A[..., ::-1, :, :])
    if geo.d > 1:
        A = np.maximum(A, A[..., :, ::-1, :])
    return A.reshape(M.shape)


class M2L:
    """L_c += U_v (V_v^T (perm M_s)) per V-list pair, batched by transfer vector over all cells of a level, with the
    factors exactly as the handle returns them."""

    def __init__(self, geo, t):
        self.geo = geo
        self.ranks = t.m2l_ranks()
        self.f = {}
        for level in range(2, geo.depth + 1):
            for ref in range(self.ranks.shape[1]):
                u, vt = t.m2l_factors(level, ref)
                self.f[level, ref] = (u.astype(LD), None if vt is None else vt.astype(LD))

    def pairs_of(self, cells=None, skip=None):
        g = self.geo
        keep = np.ones(len(g.v_tgt), dtype=bool)
        if cells is not None:
            keep &= np.isin(g.v_tgt, cells)
        if skip is not None:                       # (target, source) pairs left out: the altered-data test
            for tc, sc in skip:
                keep &= ~((g.v_tgt == tc) & (g.v_src == sc))
        return keep

    def apply(self, M, cells=None, skip=None):
        """(L (K, C, n), s (K, C, n), R (C,)) of M2L alone for the double M (K, C, n): long double, zero where no pair lands."""
        g = self.geo
        M = np.asarray(M, dtype=np.float64)
        K = M.shape[0]
        Ml, Ms = M.astype(LD), sym_abs(g, M).astype(LD)
        L, S = np.zeros((K, g.C, g.n), dtype=LD), np.zeros((K, g.C, g.n), dtype=LD)
        R = np.zeros(g.C, dtype=np.int64)
        keep = self.pairs_of(cells, skip) & (M != 0).any(axis=(0, 2))[g.v_src]   # (a source of zeros contributes exact zeros)
        lev = g.level[g.v_tgt]
        for level in np.unique(lev[keep]):
            for tv in np.unique(g.v_tidx[keep & (lev == level)]):
                sel = keep & (lev == level) & (g.v_tidx == tv)
                tg, sc = g.v_tgt[sel], g.v_src[sel]
                ref, pl = int(g.ref_lookup[tv]), int(g.perm_lookup[tv])
                u, vt = self.f[int(level), ref]
                perm, inv = g.perm[pl], g.invperm[pl]
                kk = np.nonzero((M[:, sc] != 0).any(axis=(1, 2)))[0]                     # right-hand sides with a live source
                X, Xs = Ml[kk][:, sc][:, :, perm], Ms[kk][:, sc][:, :, perm]             # (K', cells, n)
                if vt is not None:
                    Y, Ys = (X @ vt.T) @ u.T, (Xs @ np.abs(vt).T) @ np.abs(u).T
                else:
                    Y, Ys = X @ u.T, Xs @ np.abs(u).T
                L[kk[:, None], tg[None, :]] += Y[:, :, inv]
                S[kk[:, None], tg[None, :]] += Ys[:, :, inv]
                R[tg] += u.shape[1]
        return L, S, R

    def bound(self, S, R):
        """(K, C): u 4 (n + R_c + c0) max_j s_j."""
        return LD(U) * 4 * (self.geo.n + R + C0_M2L)[None, :] * S.max(axis=-1)


# ------------------------------------------------------------------ P2L
def p2l(geo, kernel, pts, w, cell, where=1):
    """(term (K, n), bound (K,)) of the X-list term of one cell; kernel = (id, base_range, total_sill); where = 1 the
    device's kernel functions, 0 the host's (the budgets of kernel_pointwise)."""
    import kernel_pointwise as KP
    import kernel_reference as KR
    xp, xi = geo.lists["X"]
    srcs = np.concatenate([geo.src_idx[geo.src_ptr[x]:geo.src_ptr[x + 1]] for x in xi[xp[cell]:xp[cell + 1]]])
    nd = np.stack(np.meshgrid(*[nodes(geo.p)] * geo.d, indexing="ij"), -1).reshape(-1, geo.d)
    pos = (geo.centres[cell].astype(LD) + (LD(geo.lengths[cell]) / 2) * nd).astype(np.float64)
    D = KR.Dense(kernel[0], kernel[1], kernel[2], pos, pts[srcs])
    y, s_phi, s_arg = D.sums(np.asarray(w, dtype=np.float64).reshape(len(pts), -1)[srcs])
    a, b = KP.sum_budget(where, kernel[0], "value")
    # a node coordinate centre + (len / 2) node carries up to two roundings of size u |coordinate| per axis; a source of
    # the X list lies in a leaf that is not adjacent to the cell, so r >= len, and the relative change of r^2 is at most
    # 2 sqrt(d) (2 u |coord|) / len <= 8 u |coord| / len
    g = float(np.abs(pos).max() / geo.lengths[cell])
    return y.T, LD(U) * ((len(srcs) + a + 4) * s_phi + (b + 4 + 8 * g) * s_arg).T.max(axis=-1)


# ------------------------------------------------------------------ M2P
def cell_nodes(geo, cell):
    """The Chebyshev nodes of a cell, (n, d) doubles in node-index order: centre + (len / 2) node formed in long double
    from the doubles the handle exposes and rounded to double (as p2l forms its targets)."""
    nd = np.stack(np.meshgrid(*[nodes(geo.p)] * geo.d, indexing="ij"), -1).reshape(-1, geo.d)
    return (geo.centres[cell].astype(LD) + (LD(geo.lengths[cell]) / 2) * nd).astype(np.float64)


class M2PMatrices:
    """The kernel matrices of (targets in `leaf`) x (nodes of the cells of its W list), computed once: the sums for any
    multipoles come from them.  Without gradients only the three matrices of the value path are kept."""

    def __init__(self, geo, kernel, leaf, targets, where=1, gradients=False):
        import kernel_pointwise as KP
        import kernel_reference as KR
        wp, wi = geo.lists["W"]
        self.n, self.cells = geo.n, [int(c) for c in wi[wp[leaf]:wp[leaf + 1]]]
        assert self.cells, "the leaf has no W list"
        pos = [cell_nodes(geo, c) for c in self.cells]
        self.g = max(float(np.abs(q).max() / geo.lengths[c]) for q, c in zip(pos, self.cells))
        assert self.g >= 0.8                                          # the premise of the 8 g term (module docstring)
        self.N = sum(len(q) for q in pos)
        self.budget = {path: KP.sum_budget(where, kernel[0], path) for path in ("value", "value_g", "factor")}
        D = KR.Dense(kernel[0], kernel[1], kernel[2], targets, np.concatenate(pos))
        self.value, self.abs_value, self.abs_x_dvalue = D.value, D.abs_value, D.abs_x_dvalue
        self.D = D if gradients else None
        self.delta = np.concatenate([np.full(len(q), geo.lengths[c] + np.abs(q).max()) for q, c in zip(pos, self.cells)]).astype(LD)

    def weights(self, M_dev):
        return np.concatenate([np.asarray(M_dev[:, c, :self.n], dtype=np.float64).T for c in self.cells]).astype(LD)   # (N, K)

    def _bound(self, path, s_main, s_arg):
        a, b = self.budget[path]
        return LD(U) * ((self.N + a + 4) * s_main + (b + 4 + 8 * self.g) * s_arg)

    def values(self, M_dev, rows=slice(None)):
        """y (m, K) and its bound at the targets `rows`."""
        w = self.weights(M_dev)
        aw = np.abs(w)
        return self.value[rows] @ w, self._bound("value", self.abs_value[rows] @ aw, self.abs_x_dvalue[rows] @ aw)

    def gradients(self, M_dev):
        """(values, their bound under the value_g budget, gradients (m, K, d), their bound)."""
        w = self.weights(M_dev)
        y, gr, s_phi, s_arg, s_f, s_xf = self.D.grad_sums(w)
        s_pos = np.abs(self.D.factor) @ (np.abs(w) * self.delta[:, None])
        return y, self._bound("value_g", s_phi, s_arg), gr, self._bound("factor", s_f, s_xf) + LD(U) * s_pos[:, :, None]


def m2p(geo, kernel, M_dev, leaf, targets, with_grads=False, where=1):
    """y (m, K) and its bound (m, K) of the W-list term at targets in `leaf`, from the device's M (K, C, n); with_grads
    the values of a gradient call (the value_g budget) and their bound, then the gradients (m, K, d) and their bound.
    kernel = (id, base_range, total_sill); where as in p2l."""
    mats = M2PMatrices(geo, kernel, leaf, targets, where, gradients=with_grads)
    return mats.gradients(M_dev) if with_grads else mats.values(M_dev)


# ------------------------------------------------------------------ L2P
def l2p(geo, L_dev, cell, targets, with_grads=False):
    """y (m, K) and its bound (m, K) for targets in leaf `cell` from the device's L (K, C, n); with_grads also the
    gradients (m, K, d) and their bounds.  The contraction over the last axis (the expensive one) is formed once per
    distinct (factor, coefficients) pair and shared by the sums that need it."""
    Lc = np.asarray(L_dev[:, cell], dtype=np.float64).astype(LD)
    aL = np.abs(Lc)
    K, P, d, p = Lc.shape[0], geo.P, geo.d, geo.p
    S, D = geo.factors(cell, targets, deriv=True)
    A = [np.abs(s) for s in S]
    ONE = [np.ones_like(s) for s in S]
    m = S[0].shape[0]
    stage = {}

    def contract(F, coef, tag):
        """sum_j coef[k, j] F0[m, a] F1[m, b] F2[m, c]; tag names (F2, coef) for the shared first step."""
        if tag not in stage:
            stage[tag] = (F[2] @ coef.reshape(K * P[0] * P[1], P[2]).T).reshape(m, K, P[0], P[1])
        v = (stage[tag] * F[1][:, None, None, :]).sum(axis=3)
        return (v * F[0][:, None, :]).sum(axis=2)

    def mag(F, tag):
        return contract(F, aL, tag)

    def one_at_a_time(F, tags, skip=None):
        """F with one value factor at a time replaced by ones (tags[a]: the name of F2 when axis a is replaced)."""
        tot = 0
        for a in range(d):
            if a != skip:
                G = list(F)
                G[a] = ONE[a]
                tot = tot + mag(G, tags[a])
        return tot

    y = contract(S, Lc, "S")
    yb = LD(U) * ((3 * p + 4) * mag(A, "A") + e_S(p) * one_at_a_time(A, ["A", "A", "1"]))
    if not with_grads:
        return y, yb
    scale = LD(2) / LD(geo.lengths[cell])
    g, gb = [], []
    for a in range(d):
        F, Fa, Fo = list(S), list(A), list(A)
        F[a], Fa[a], Fo[a] = D[a], np.abs(D[a]), ONE[a]
        last = "D" if a == 2 else "S"
        alast = "|D|" if a == 2 else "A"
        g.append(contract(F, Lc, last))
        tags = [alast, alast, "1"]
        gb.append(LD(U) * ((3 * p + 6) * mag(Fa, alast) + e_S(p) * one_at_a_time(Fa, tags, skip=a)
                           + e_dS(p) * scale * mag(Fo, "1" if a == 2 else "A")))
    return y, yb, np.stack(g, axis=2), np.stack(gb, axis=2)


# ------------------------------------------------------------------ the per-cell check
def check_cells(name, got, ref, bound, cells, what="", describe=None):
    """max_j |got - ref| of every listed cell and right-hand side against its own bound.  got (K, C, n) double, ref and bound
    dicts or arrays indexed by cell: ref[c] (K, n), bound[c] (K,).  Prints and returns the largest ratio; asserts <= 1."""
    worst, at = 0.0, None
    for c in cells:
        err = np.abs(np.asarray(got[:, c], dtype=np.float64).astype(LD) - ref[c]).max(axis=-1)
        b = np.asarray(bound[c], dtype=LD)
        with np.errstate(all="ignore"):
            r = np.where(err == 0, LD(0), err / np.where(b > 0, b, LD(1)) + np.where(b > 0, LD(0), LD(np.inf)))
        k = int(np.argmax(r))
        if float(r[k]) > worst:
            worst, at = float(r[k]), (int(c), k, float(err[k]), float(b[k]))
    where = f" [{describe(at[0])}]" if describe is not None and at is not None else ""
    print(f"{name} {what}: largest error / bound {worst:.3g} at (cell, rhs, error, bound) {at}{where}")
    assert np.isfinite(np.asarray(got[:, list(cells)])).all(), (name, what)
    assert worst <= 1.0, (name, what, worst, at, where)
    return worst


def l2l_many(geo, xf, L_dev, cells, terms=None):
    """L2L into many cells at once, batched by octant: (term (K, len(cells), n), bound (K, len(cells)))."""
    cells = np.asarray(cells, dtype=np.int64)
    K = L_dev.shape[0]
    val, bnd = np.zeros((K, len(cells), geo.n), dtype=LD), np.zeros((K, len(cells)), dtype=LD)
    terms = 3 * geo.p + 3 if terms is None else terms
    for o in np.unique(geo.octant[cells]):
        at = np.nonzero((geo.octant[cells] == o) & (geo.parent[cells] >= 0))[0]
        if len(at) == 0:
            continue
        vec = L_dev[:, geo.parent[cells[at]]].reshape(K * len(at), geo.n)
        v, s_abs, s_fac = xf.apply(vec, int(o), False)
        val[:, at] = v.reshape(K, len(at), geo.n)
        bnd[:, at] = (LD(U) * (terms * s_abs + e_S(geo.p) * s_fac).max(axis=-1)).reshape(K, len(at))
    return val, bnd


def downward(geo, m2l, xf, M_dev, L_dev, cells, p2l_args=None, terms=None, skip=None, m2l_result=None, p2l_cache=None):
    """What L holds in the listed cells after the downward pass, one step from its inputs: M2L of M_dev, plus L2L of the
    parent's L_dev, plus (p2l_args = (kernel, pts, w, where)) the X-list term.  Two dicts: ref[c] (K, n), bound[c] (K,).
    m2l_result: m2l.apply(M_dev) computed before (it depends on M_dev alone).  p2l_cache: a dict that keeps the X-list terms
    of the cells (they depend on the weights alone, column by column): w may then hold more columns than L_dev has
    right-hand sides, every column is restated once and later calls take the first K."""
    cells = [int(c) for c in cells]
    Lm, S, R = m2l.apply(M_dev, cells=np.asarray(cells), skip=skip) if m2l_result is None else m2l_result
    bm = m2l.bound(S, R)
    xp = geo.lists["X"][0]
    lv, lb = l2l_many(geo, xf, L_dev, cells, terms)
    ref, bound = {}, {}
    for i, c in enumerate(cells):
        parts, b = [Lm[:, c]], bm[:, c]
        if geo.parent[c] >= 0:
            parts.append(lv[:, i])
            b = b + lb[:, i]
        if p2l_args is not None and xp[c + 1] > xp[c]:
            kernel, pts, w, where = p2l_args
            if p2l_cache is None:
                v, bp = p2l(geo, kernel, pts, w, c, where)
            else:
                if c not in p2l_cache:
                    p2l_cache[c] = p2l(geo, kernel, pts, w, c, where)
                v, bp = (a[:L_dev.shape[0]] for a in p2l_cache[c])
            parts.append(v)
            b = b + bp
        ref[c] = sum(parts)
        bound[c] = b + LD(U) * len(parts) * sum(np.abs(v).max(axis=-1) for v in parts)   # the additions of the terms
    return ref, bound
