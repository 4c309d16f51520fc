"""The checks of tests/schwarz_sweep_reference.py rehearsed without a GPU: a float64 numpy stand-in for the device's sweep
(dense kernel products, numpy solves of the same domains) produces a trace of the same shape.  It passes every check; each
mutation of it -- the errors a five-digit end-to-end tolerance would let through -- fails the check named for it; and a
stand-in whose vector steps are rounded from long double stays inside the bounds (the reference does not exceed its own)."""
import numpy as np
import pytest
import scipy.linalg as sla

import kernel_reference as KR
import schwarz_sweep_reference as W
from ferreus_rbf_rs_amd.ddm import DDMParams, DDMTree, InterpolantSettings
from kernel_reference import LD

PARAMS = (48, 0.5, 0.25, 64)


def kernel_matrix(st, xa, xb, dtype=np.float64):
    return KR.Dense(st.kernel_type, st.base_range, st.total_sill, W.R._pad3(xa), W.R._pad3(xb)).value.astype(dtype)


class HostLevel:
    """The local solvers of one level by numpy: per domain the saddle-point system [[A, P], [P^T, 0]], special points first."""

    def __init__(self, points, domains, st, solve_for_poly=False, scaling=None):
        self.indices, self.internal, self.k, self.m, self._lu, self._a = [], [], [], [], [], []
        for idx, mask in domains:
            idx, mask = np.asarray(idx), np.asarray(mask, dtype=bool)
            x = points[idx]
            a = kernel_matrix(st, x, x) + st.nugget * np.eye(idx.size)
            k = st.basis_size
            if k:
                mono = W.monomials(x, st.polynomial_degree, *(scaling or W.extents_scaling(x)))
                piv = sla.qr(mono.T, pivoting=True, mode="r")[1]
                special = np.sort(piv[:k])
                order = np.concatenate([special, np.setdiff1d(np.arange(idx.size), special)])
                idx, mask, mono = idx[order], mask[order], mono[order]
                a = np.block([[a[np.ix_(order, order)], mono], [mono.T, np.zeros((k, k))]])
            self.indices.append(idx)
            self.internal.append(mask)
            self.k.append(k)
            self.m.append(idx.size - k)
            self._lu.append(sla.lu_factor(a))
            self._a.append(a)

    def forward(self, values, i=0):
        """(coefficients of domain i in long double, their forward bound) for values in the domain's order: the LU solve
        refined twice with long-double residuals, and the normwise bound of a pivoted LU with the constant of
        ddm_local_reference section 4, 8 n u kappa ||x||."""
        a, lu, n = self._a[i], self._lu[i], self.indices[i].size
        rhs = np.concatenate([np.asarray(values, dtype=np.float64), np.zeros(self.k[i])]).astype(LD)
        x = sla.lu_solve(lu, rhs.astype(np.float64)).astype(LD)
        for _ in range(2):
            x = x + sla.lu_solve(lu, (rhs - a.astype(LD) @ x).astype(np.float64)).astype(LD)
        bound = 8 * a.shape[0] * W.U * np.linalg.cond(a) * float(np.abs(x).max())
        return x[:n], np.full(n, bound)

    def solve(self, values, out, all_points=False):
        o = np.array(out, dtype=np.float64)
        for idx, mask, k, lu in zip(self.indices, self.internal, self.k, self._lu):
            lam = sla.lu_solve(lu, np.concatenate([values[idx], np.zeros(k)]))[:idx.size]
            keep = np.ones(idx.size, dtype=bool) if all_points else mask
            o[idx[keep]] = lam[keep]
        return o


class HostSweep:
    """level_step() and the loop of the apply in float64 numpy.  mutate: a set of the defects named in the tests below.
    precise: the vector steps and the tail's right-hand side are formed in long double and rounded once."""

    def __init__(self, points, st, params=PARAMS, global_scaling=False, mutate=(), precise=False):
        self.points, self.st, self.mutate, self.precise = points, st, set(mutate), precise
        self.n, self.basis = points.shape[0], st.basis_size
        self.ddm = DDMTree(points, DDMParams(*params)).levels
        self.num_levels = len(self.ddm)
        self.kmat = kernel_matrix(st, points, points)
        self.ortho = None
        own = W.extents_scaling(points[self.ddm[-1].point_indices])
        self.scaling = W.extents_scaling(points) if global_scaling else own
        other = own if global_scaling else W.extents_scaling(points)
        if self.basis:
            self.mono = W.monomials(points, st.polynomial_degree, *W.extents_scaling(points))
            self.ortho = W.mgs_twice(self.mono, LD if precise else np.float64).astype(np.float64)
        self.levels = [HostLevel(points, W.level_domains(lv), st, li + 1 == self.num_levels and self.basis > 0,
                                 self.scaling if (li + 1 == self.num_levels and global_scaling) else None)
                       for li, lv in enumerate(self.ddm)]
        self.special = self.levels[-1].indices[0][:self.basis]
        self.tail_scaling = other if "tail_other_scaling" in self.mutate else self.scaling
        self.res = np.full(self.n, 7.0)                       # (the device's d_res starts uninitialised)
        self.out = np.zeros(self.n)

    def _step(self, li, have_sl, coarse, add_poly, rg, sl):
        st, n, mut = self.st, self.n, self.mutate
        wt = LD if self.precise else np.float64
        rows = np.asarray(self.ddm[li].point_indices)
        y, src = None, rg[:n]
        if have_sl:
            y = self.kmat[rows] @ sl
            ypad = np.zeros(n)
            ypad[:rows.size] = y
            yj = ypad[rows] if "y_by_row" in mut else y
            nug = 0.0 if "no_nugget" in mut else st.nugget
            new = ((rg[:n][rows].astype(wt) - yj.astype(wt)) - wt(nug) * sl[rows].astype(wt)).astype(np.float64)
            if "res_all_rows" in mut:
                self.res = rg[:n] - self.kmat @ sl - nug * sl
            self.res = self.res.copy()
            self.res[rows] = new
            src = self.res
        self.out = self.levels[li].solve(src, self.out, coarse)
        sl = sl.copy()
        proj = None
        if not coarse and self.basis:
            prow = np.arange(n) if "proj_all_rows" in mut else rows
            per = -(-prow.size // W.PROJECT_BLOCKS)
            part = [self.ortho[prow[lo:lo + per]].astype(wt).T @ self.out[prow[lo:lo + per]].astype(wt)
                    for lo in range(0, prow.size, per)]
            if "proj_lost_block" in mut:
                part.pop(len(part) // 2)
            proj = np.sum(part, axis=0).astype(np.float64)
        sl[rows] = sl[rows] + self.out[rows]
        if proj is not None:
            sub = rows if "subtract_level_rows" in mut else np.arange(n)
            sl[sub] = (sl[sub].astype(wt) - self.ortho[sub].astype(wt) @ proj.astype(wt)).astype(np.float64)
        tail = None
        if coarse and self.basis and (add_poly or "tail_every_visit" in mut):
            sp = self.special
            a = kernel_matrix(st, self.points[sp], self.points[rows], wt)
            if "no_nugget_diagonal" not in mut:
                a = a + wt(st.nugget) * (sp[:, None] == rows[None, :])
            r = src[sp].astype(wt) - a @ self.out[rows].astype(wt)
            spm = W.monomials(self.points[sp], st.polynomial_degree, *self.tail_scaling)
            tail = np.linalg.solve(spm, r.astype(np.float64))
            if self.precise:                                  # one step of refinement with a long-double residual
                tail = tail + np.linalg.solve(spm, (r - spm.astype(LD) @ tail.astype(LD)).astype(np.float64))
        rec = {"level": li, "coarse": coarse, "have_sl": have_sl, "add_poly": add_poly, "y": y, "res": self.res.copy(),
               "out": self.out.copy(), "sl": sl.copy(), "proj": proj, "tail": tail}
        return rec, sl

    def debug_apply_trace(self, rg):
        rg = np.asarray(rg, dtype=np.float64)
        initial = {"res": self.res.copy(), "out": self.out.copy()}
        sl, steps, coarse = np.zeros(self.n), [], self.num_levels - 1
        if coarse == 0:
            rec, sl = self._step(0, False, True, True, rg, sl)
            steps.append(rec)
        for i in range(coarse):
            rec, sl = self._step(i, i > 0, False, False, rg, sl)
            steps.append(rec)
            if "skip_coarse" in self.mutate and i == 0 and coarse > 1:
                continue
            rec, sl = self._step(coarse, True, True, i == coarse - 1, rg, sl)
            steps.append(rec)
        z = np.zeros(self.n + self.basis)
        z[:self.n] = sl
        if steps[-1]["tail"] is not None:
            z[self.n:] = steps[-1]["tail"]
        return z, steps, initial


CASES = {"3d_linear": (700, 3, 1, 3, 0.05), "3d_no_drift": (500, 3, -1, 3, 0.05), "2d_kernel0": (500, 2, 0, 0, 0.0),
         "1d_quadratic": (400, 1, 2, 3, 0.05)}
_cache = {}


def setup(name, **kw):
    key = (name, tuple(sorted((k, tuple(v) if isinstance(v, (set, tuple, list)) else v) for k, v in kw.items())))
    if key not in _cache:
        n, dim, drift, kid, nugget = CASES[name]
        pts = W.cloud(n, dim, 40 + n)
        st = InterpolantSettings(kid, dim, drift=drift, nugget=nugget, base_range=0.3 if kid == 3 else 1.0, total_sill=1.0)
        hs = HostSweep(pts, st, **kw)
        rg = np.random.default_rng(n).standard_normal(n + st.basis_size)
        rg[n:] = 0.0
        hs.debug_apply_trace(rg)                              # (a first apply leaves stale rows in d_out, as on the device)
        _cache[key] = (hs, rg, hs.debug_apply_trace(rg))
    return _cache[key]


def run_checks(hs, rg, trace, **kw):
    z, steps, initial = trace
    return W.check_trace(hs.points, hs.st, hs.ddm, hs.levels, hs.ortho, rg, z, steps, initial, special=hs.special,
                         scaling=hs.scaling, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("precise", [False, True])
def test_the_stand_in_passes_every_check(name, precise):
    hs, rg, trace = setup(name, precise=precise)
    assert hs.num_levels >= 3
    stats = run_checks(hs, rg, trace)
    print(name, "precise" if precise else "float64", stats)
    assert stats["residual"] > 0 and stats["solve_rows"] > 0 and stats["writeback_rows"] > 0
    if hs.basis:
        assert stats["projection"] > 0 and stats["writeback"] > 0 and stats["tail"] > 0 and stats["stale"] > 0
        worst, measured = W.check_ortho(hs.ortho, hs.mono)
        print("ortho", worst, measured)
    else:
        assert stats["projection"] is None and stats["tail"] is None and trace[0].size == hs.n


def test_global_scaling_stand_in_and_the_same_polynomial():
    hs, rg, trace = setup("3d_linear")
    hg, _, trace_g = setup("3d_linear", global_scaling=True)
    assert run_checks(hg, rg, trace_g)["tail"] > 0
    assert np.array_equal(hs.special, hg.special)
    assert not np.array_equal(trace[1][-1]["tail"], trace_g[1][-1]["tail"])
    lv = hs.levels[-1]
    same = W.check_tails_agree(lv.forward, lv.indices[0], hs.points, hs.st, hs.special,
                               [(t[1][-1], t[1][-2], rg, h.scaling) for h, t in ((hs, trace), (hg, trace_g))])
    print("the two tails at the special points:", same)
    assert same["ratio"] > 0
    # a tail that belongs to another right-hand side is outside the bound
    other = setup("3d_linear", global_scaling=True, mutate=("no_nugget_diagonal",))[2]
    with pytest.raises(AssertionError, match="^tail:|one polynomial"):
        W.check_tails_agree(lv.forward, lv.indices[0], hs.points, hs.st, hs.special,
                            [(t[1][-1], t[1][-2], rg, h.scaling) for h, t in ((hs, trace), (hg, other))])


def test_one_level_gives_a_single_record():
    pts = W.cloud(60, 3, 9)
    st = InterpolantSettings(3, 3, drift=1, nugget=0.05, base_range=0.3, total_sill=1.0)
    hs = HostSweep(pts, st)
    rg = np.concatenate([np.random.default_rng(1).standard_normal(60), np.zeros(4)])
    trace = hs.debug_apply_trace(rg)
    assert hs.num_levels == 1 and len(trace[1]) == 1 and not trace[1][0]["have_sl"]
    assert run_checks(hs, rg, trace)["tail"] > 0


MUTATIONS = [("no_nugget", "residual of level"), ("y_by_row", "residual of level"), ("res_all_rows", "a row outside the level"),
             ("proj_all_rows", "projection of level"), ("proj_lost_block", "projection of level"),
             ("subtract_level_rows", "write-back of level"), ("tail_every_visit", "not the last"),
             ("skip_coarse", "order of the sweep"), ("no_nugget_diagonal", "^tail:"), ("tail_other_scaling", "^tail:")]


@pytest.mark.parametrize("mutation,names", MUTATIONS)
def test_each_mutation_fails_the_check_named_for_it(mutation, names):
    hs, rg, trace = setup("3d_linear", mutate=(mutation,))
    with pytest.raises(AssertionError, match=names):
        run_checks(hs, rg, trace)
    # ... and no other check: with the named one left out the trace passes
    z, steps, initial = trace
    n = hs.n
    for i, step in enumerate(steps):
        before = W.state_before(steps, initial, i)
        rows = np.asarray(hs.ddm[step["level"]].point_indices)
        if mutation not in ("no_nugget", "y_by_row", "res_all_rows"):
            W.check_residual(step, before, rg, rows, hs.st.nugget)
        W.check_local_solves(hs.levels[step["level"]], step, before, rg)
        if step["proj"] is not None and mutation not in ("proj_all_rows", "proj_lost_block"):
            W.check_projection(step, hs.ortho, rows)
        if mutation != "subtract_level_rows":
            W.check_writeback(step, before, hs.ortho, rows)
    assert z.size == n + hs.basis
