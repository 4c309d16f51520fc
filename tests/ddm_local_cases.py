"""The inputs of tests/test_gpu_ddm_local.py and scripts/ddm_local_accuracy.py: levels of prescribed domains for the debug hook
(ferreus_rbf_rs_amd.ddm.DebugLevel) and the per-domain checks against tests/ddm_local_reference.py.  A plain helper module.

Points lie on the 2^-30 grid (ddm_local_reference.on_grid).  The matrices are those of the bounds' calibration unless a case
says otherwise: uniform points in the unit cube, Spheroidal (order 3), range 0.3, sill 1, nugget 0.05."""
import numpy as np

import ddm_local_reference as R
from ferreus_rbf_rs_amd.ddm import DebugLevel, InterpolantSettings

# every block edge of the per-domain kernels: the 32-wide solve panels, the 16-row MFMA groups, the 64-column blocks with a
# short last block, the four-wave turn of 256 rows (first wrap at 321), a second wrap plus a short block
M_ALL = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320, 321, 383, 384, 385, 577, 641)
M_FEW = (1, 2, 17, 33, 64, 65, 129, 257, 321)
M_KERNELS = (33, 65, 257)
# one large domain: h1 >= m and end >= m exits, one-column second halves, one-row trailing parts, tiles4 rounding, a third and
# a fourth 1024-block of 1 and 1023 columns
BIG_CASES = tuple(zip((2049, 2111, 2112, 2113, 2175, 2176, 2177, 3071, 3072, 3073), (0, 4, 10, 0, 4, 10, 0, 4, 10, 4)))
DEGREE_OF_K3 = {0: -1, 1: 0, 4: 1, 10: 2}
SENTINEL = np.float64(-1.2345678901234567e+300)

make_level = DebugLevel        # (a host stand-in can be put here to rehearse the checks without a GPU)


def settings(kid=3, dim=3, drift=-1, nugget=0.05, base_range=0.3, total_sill=1.0):
    return InterpolantSettings(kid, dim, drift=drift, nugget=nugget, base_range=base_range, total_sill=total_sill)


def disjoint_domains(rng, dim, sizes, box=1.0, internal=0.6):
    """One fresh uniform cloud per domain (`sizes` points each), a random internal mask with at least one point set."""
    pts, doms, off = [], [], 0
    for n in sizes:
        pts.append(R.on_grid(rng.random((n, dim)) * box))
        mask = rng.random(n) < internal
        mask[rng.integers(n)] = True
        doms.append((np.arange(off, off + n), mask))
        off += n
    return np.vstack(pts), doms


def add_domain(pts, doms, x, rng, internal=0.6):
    mask = rng.random(x.shape[0]) < internal
    mask[0] = True
    doms.append((np.arange(pts.shape[0], pts.shape[0] + x.shape[0]), mask))
    return np.vstack([pts, R.on_grid(x)]), doms


def flagship(seed=11):
    """All sizes of M_ALL with a linear drift in 3-D (k = 4), a coplanar domain (k = 3 < basis) and one with duplicated
    points.  Returns (points, domains, settings, expected k per domain)."""
    rng = np.random.default_rng(seed)
    pts, doms = disjoint_domains(rng, 3, [m + 4 for m in M_ALL])
    flat = rng.random((43, 3))
    flat[:, 2] = 0.5
    pts, doms = add_domain(pts, doms, flat, rng)
    dup = rng.random((54, 3))
    dup[10:14] = dup[0:4]
    pts, doms = add_domain(pts, doms, dup, rng)
    return pts, doms, settings(drift=1), [4] * len(M_ALL) + [3, 4]


def sized(seed, dim, drift, sizes, k, kid=3, nugget=0.05, base_range=0.3, total_sill=1.0):
    rng = np.random.default_rng(seed)
    pts, doms = disjoint_domains(rng, dim, [m + k for m in sizes])
    return pts, doms, settings(kid, dim, drift, nugget, base_range, total_sill), [k] * len(sizes)


def many_small(seed=5, count=511):
    """512 domains (the assembly launch splits the columns four ways instead of sixty-four from 512 domains on)."""
    rng = np.random.default_rng(seed)
    sizes = [int(v) for v in rng.integers(4, 11, count)] + [131]
    pts, doms = disjoint_domains(rng, 3, sizes)
    return pts, doms, settings(drift=0), [1] * len(sizes)


def overlapping(seed=21):
    """Three domains whose internal sets are disjoint and whose overlaps reach into each other, 40 points that no domain
    holds as internal and 25 that no domain holds at all."""
    rng = np.random.default_rng(seed)
    pts = R.on_grid(rng.random((3 * 150 + 40 + 25, 3)))
    doms = []
    for i in range(3):
        own = np.arange(150 * i, 150 * (i + 1))
        others = np.setdiff1d(np.arange(450 + 40), own)
        extra = rng.choice(others, 70, replace=False)
        idx = np.concatenate([own, extra])
        perm = rng.permutation(idx.size)
        doms.append((idx[perm], (np.arange(idx.size) < 150)[perm]))
    return pts, doms, settings(drift=1)


def two_clusters(rng, n, side):
    """Two clusters of n / 2 points, far apart and each so tight that n slope r stays below the nugget's 0.05: the kernel
    matrix is then [[J, eps J], [eps J, J]] (J all ones) up to less than that, two large positive eigenvalues, and a negative
    nugget puts all the others near -0.05 -- indefinite with a wide gap around zero."""
    x = side * rng.random((n, 3))
    x[: n // 2] += 0.05
    x[n // 2:] += 0.95
    return R.on_grid(x)


def fallback(seed=31):
    """A negative nugget: tightly clustered domains are indefinite, domains whose points lie further apart than the range stay
    positive definite.  Constant drift (k = 1)."""
    rng = np.random.default_rng(seed)
    pts, doms = np.zeros((0, 3)), []
    kinds = []
    for n, tight in ((21, True), (28, False), (34, True), (65, False), (66, True), (71, True), (101, False), (130, True)):
        if tight:
            x = two_clusters(rng, n, 2e-5)
        else:       # a jittered lattice of spacing 0.6 = twice the range
            side = int(np.ceil(n ** (1 / 3)))
            g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n]
            x = 0.6 * g + 0.05 * rng.random((n, 3))
        pts, doms = add_domain(pts, doms, x, rng)
        kinds.append(tight)
    return pts, doms, settings(drift=0, nugget=-0.05), kinds


def big(m, k, seed=0, nugget=0.05, box=1.0):
    rng = np.random.default_rng(3000 + m + seed)
    n = m + k
    pts = R.on_grid(rng.random((n + 30, 3)) * box)           # (30 points the domain does not hold)
    idx = rng.permutation(n + 30)[:n]
    mask = rng.random(n) < 0.5
    return pts, [(idx, mask)], settings(drift=DEGREE_OF_K3[k], nugget=nugget)


# ------------------------------------------------------------------ per-domain checks
def domain_points(level, pts, i):
    return pts[level.indices[i]]


def check_assembly(level, pts, st, assembled, i, rows=None):
    a_ref, bound = R.assembly_reference(st.kernel_type, st.base_range, st.total_sill, st.nugget, domain_points(level, pts, i),
                                        level.k[i], level.q[i], rows=rows)
    return R.assembly_check(assembled[i], level.m[i], a_ref, bound, rows=rows)


def check_factor(level, assembled, factor, i, rows=None):
    return R.factor_check(assembled[i], factor[i], level.m[i], big=level.is_big, rows=rows)


def check_solve(level, factor, values, out, i):
    idx = level.indices[i]
    return R.solve_check(factor[i], level.m[i], level.k[i], level.q[i], values[idx], out[idx], big=level.is_big)


def reference_matrix(level, pts, st, i):
    """Q^T A Q of domain i in long double, symmetric."""
    a_ref, _ = R.assembly_reference(st.kernel_type, st.base_range, st.total_sill, st.nugget, domain_points(level, pts, i),
                                    level.k[i], level.q[i])
    lo = np.tril(a_ref)
    return lo + np.tril(lo, -1).T


def rows_written(level, n, all_points):
    w = np.zeros(n, dtype=bool)
    for idx, internal in zip(level.indices, level.internal):
        w[idx[internal | bool(all_points)]] = True
    return w


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))
