"""FGMRES and the Schwarz iteration with their vectors on the device (solvers.fgmres / schwarz_ddm_solver,
vectors="device"; DESIGN.md, "Device-resident solvers"): the vector kernels against numpy.longdouble, the drivers
against the host drivers on dense operators, the device operators against their host twins, and the fit."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ferreus_rbf_rs_amd as F
from ferreus_rbf_rs_amd import _lib as L
from ferreus_rbf_rs_amd import rbf as R
from ferreus_rbf_rs_amd import solvers as S
from ferreus_rbf_rs_amd.ddm import DDMParams, InterpolantSettings, SchwarzPreconditioner

U = 2.0 ** -53
LD = np.longdouble
REL, ABS = S.FittingAccuracyType.Relative, S.FittingAccuracyType.Absolute


# ------------------------------------------------------------------------------------------------ 1. vector kernels
SIZES = [1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 200003]   # wave, block and chunk edges, two and a bit chunks


def vector_op(op, a, b=None, c=None, alpha=0.0, mode=3, coeffs=None, offset=0):
    """bbfmm_debug_solver_vector_op -> (the vector the op writes, scalars[2])"""
    a = np.asfortranarray(a, dtype=np.float64)
    n = a.shape[0]
    out, sc = np.zeros(n), np.zeros(2)
    b, c, coeffs = (None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (b, c, coeffs))
    data = lambda v: None if v is None else v.ctypes.data  # noqa: E731
    rc = L.load().bbfmm_debug_solver_vector_op(op, mode, n, a.ctypes.data, data(b), data(c), float(alpha),
                                               0 if coeffs is None else len(coeffs), data(coeffs), offset, out.ctypes.data,
                                               sc.ctypes.data)
    assert rc == L.OK, rc
    return out, sc


@functools.lru_cache(maxsize=None)
def vectors(n):
    """mixed signs, magnitudes over 1e-3 .. 1e3; shared and left unchanged"""
    rng = np.random.default_rng(1000 + n)
    out = []
    for _ in range(3):
        v = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)
        v.setflags(write=False)
        out.append(v)
    return out


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_reductions_against_long_double(n, offset):
    a, b, _ = vectors(n)
    exact = float(np.abs(a.astype(LD) * b.astype(LD)).sum())
    _, sc = vector_op(3, a, b, offset=offset)
    print(n, "dot error / bound", abs(LD(sc[0]) - (a.astype(LD) * b.astype(LD)).sum()) / (n * U * exact))
    assert abs(LD(sc[0]) - (a.astype(LD) * b.astype(LD)).sum()) <= n * U * exact
    _, again = vector_op(3, a, b, offset=offset)
    assert again[0].tobytes() == sc[0].tobytes()                   # the same bits run to run
    s2 = (a.astype(LD) ** 2).sum()
    _, sq = vector_op(3, a, a, offset=offset)                      # ||a||_2^2
    assert abs(LD(sq[0]) - s2) <= n * U * float(s2)
    _, nrm = vector_op(4, a, offset=offset)
    _, nrm2 = vector_op(4, a, offset=offset)
    assert nrm[0].tobytes() == nrm2[0].tobytes()
    # sqrt(s (1 + d)), |d| <= n u, then the square root's own rounding (one ulp allowed)
    assert abs(LD(nrm[0]) - np.sqrt(s2)) <= (n * U / 2 + 2 * U) * float(np.sqrt(s2))
    _, mx = vector_op(5, a, offset=offset)
    _, mx2 = vector_op(5, a, offset=offset)
    assert mx[0] == np.abs(a).max() and mx2[0].tobytes() == mx[0].tobytes()     # exact


def test_reductions_do_not_depend_on_the_alignment():
    a, b, _ = vectors(200003)
    assert vector_op(3, a, b, offset=0)[1][0].tobytes() == vector_op(3, a, b, offset=1)[1][0].tobytes()
    assert vector_op(4, a, offset=0)[1][0].tobytes() == vector_op(4, a, offset=1)[1][0].tobytes()


def test_the_partials_are_added_in_chunk_order_like_the_host():
    """exactly representable data: chunk sums 2^60, 1, -2^60 give 0 added in index order and 1 in any other"""
    n = 3 * 65536
    a = np.zeros(n)
    a[0], a[65536], a[2 * 65536] = 2.0 ** 60, 1.0, -2.0 ** 60
    assert vector_op(3, a, np.ones(n))[1][0] == 0.0


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_elementwise_kernels_against_long_double(n, offset):
    a, b, c = vectors(n)
    out, sc = vector_op(0, a, b, offset=offset)                    # a - b: one rounding, with the fused norms of the result
    assert np.array_equal(out, a - b)
    s2 = (out.astype(LD) ** 2).sum()
    assert abs(LD(sc[0]) - s2) <= n * U * float(s2) and sc[1] == np.abs(out).max()
    alpha = -3.7e-2
    for mode, eff in ((0, alpha), (1, -alpha), (2, 1.0 / alpha), (3, alpha)):
        out, _ = vector_op(1, a, alpha=alpha, mode=mode, offset=offset)          # alpha' a: one rounding
        assert np.array_equal(out, eff * a), mode
        out, sc = vector_op(2, a, b, c, alpha=alpha, mode=mode, offset=offset)   # b + alpha' a, then <c, result>
        ax = LD(eff) * a.astype(LD)
        assert np.all(np.abs(out.astype(LD) - (b.astype(LD) + ax)) <= 2 * U * (np.abs(b) + np.abs(ax).astype(np.float64))), mode
        assert np.array_equal(out, b + eff * a), mode              # and the host loop's arithmetic: a product, then a sum
        prod = c.astype(LD) * out.astype(LD)
        assert abs(LD(sc[0]) - prod.sum()) <= n * U * float(np.abs(prod).sum()), mode
        _, sc_self = vector_op(2, a, b, None, alpha=alpha, mode=mode, offset=offset)   # the norm of the result, squared
        s2 = (out.astype(LD) ** 2).sum()
        assert abs(LD(sc_self[0]) - s2) <= n * U * float(s2), mode
    out, _ = vector_op(1, a, alpha=0.0, mode=2, offset=offset)     # a zero norm yields a zero vector
    assert not out.any()


@pytest.mark.parametrize("n", [1, 257, 65537, 200003])
@pytest.mark.parametrize("offset", [0, 1])
def test_solution_update(n, offset):
    rng = np.random.default_rng(n)
    z = np.asfortranarray(rng.standard_normal((n, 5)))
    x, _, _ = vectors(n)
    y = rng.standard_normal(5)
    for count in (1, 5):
        out, _ = vector_op(6, z[:, :count], x, coeffs=y[:count], offset=offset)
        want = x.copy()
        for c in range(count):
            want = want + y[c] * z[:, c]                           # the host's axpys in turn
        assert np.array_equal(out, want)


# ------------------------------------------------------------------------------------------------ 2. driver logic
def dense_system(n, seed=0):
    """A = I + 0.5 R / ||R||_2: cond(A) <= 3 by construction"""
    rng = np.random.default_rng(seed + n)
    Rm = rng.standard_normal((n, n))
    A = np.eye(n) + 0.5 * Rm / np.linalg.norm(Rm, 2)
    return A, rng.standard_normal(n), rng.standard_normal(n)


def on_device(M):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(M)).cuda()
    return (lambda v: t @ v) if M.ndim == 2 else (lambda v: t * v)


def on_host(M):
    return (lambda v: M @ v) if M.ndim == 2 else (lambda v: M * v)


def compare(run, absolute, beta):
    xh, hh = run("host", on_host)
    xd, hd = run("device", on_device)
    assert [i for i, _ in hh] == [i for i, _ in hd], (hh, hd)                  # equal iteration counts
    scale = beta if absolute else 1.0                                          # relative histories are already over beta
    diffs = [abs(a - b) for (_, a), (_, b) in zip(hh, hd)]
    dx = float(np.abs(xh - xd).max())
    print("largest history difference / bound", max(diffs, default=0.0) / (1e-10 * scale),
          "x", dx / (1e-10 * max(np.abs(xh).max(), 1e-300)))
    assert all(d <= 1e-10 * scale for d in diffs), (hh, hd)
    assert dx <= 1e-10 * np.abs(xh).max()
    return xh, hh


@pytest.mark.parametrize("n", [1, 7, 300])
@pytest.mark.parametrize("ttype", [REL, ABS])
@pytest.mark.parametrize("with_x0", [False, True])
@pytest.mark.parametrize("outer,inner", [(20, 5), (3, 2)])
@pytest.mark.parametrize("precon", ["jacobi", None])
def test_fgmres_device_follows_the_host_driver(n, ttype, with_x0, outer, inner, precon):
    A, b, x0 = dense_system(n)
    M = None if precon is None else 1.0 / np.diag(A)
    r0 = b - A @ (x0 if with_x0 else 0 * x0)
    beta = np.abs(r0).max() if ttype is ABS else np.linalg.norm(r0)

    def run(vec, wrap):
        return S.fgmres(wrap(A), b, None if M is None else wrap(M), x0 if with_x0 else None, outer, inner,
                        S.FittingAccuracy(1e-9, ttype), vectors=vec)

    x, hist = compare(run, ttype is ABS, beta)
    if (outer, inner) == (3, 2) and n > 1:
        assert len(hist) == 6 and hist[-1][1] > 1e-9               # ran out of outer iterations
    else:
        assert hist[-1][1] < 1e-9 and (n == 1 or len(hist) > inner)   # converged, after a restart
        assert np.abs(A @ x - b).max() < 1e-7 * np.abs(b).max()


@pytest.mark.parametrize("ttype", [REL, ABS])
def test_fgmres_device_zero_residual_return(ttype):
    A, _, _ = dense_system(7)
    x0 = np.zeros(7)
    x0[3] = 1.0
    b = A[:, 3].copy()                                             # b = A x0 exactly, in any order of summation
    for vec, wrap in (("host", on_host), ("device", on_device)):
        x, hist = S.fgmres(wrap(A), b, None, x0, 20, 5, S.FittingAccuracy(1e-9, ttype), vectors=vec)
        assert hist == [] and np.array_equal(x, x0), vec


@pytest.mark.parametrize("n", [1, 7, 300])
@pytest.mark.parametrize("ttype", [REL, ABS])
@pytest.mark.parametrize("precon,max_iterations", [("inverse", 100), ("jacobi", 100), ("jacobi", 5), (None, 100)])
def test_schwarz_ddm_solver_device_follows_the_host_driver(n, ttype, precon, max_iterations):
    A, b, _ = dense_system(n, seed=5)
    M = {"inverse": np.linalg.inv(A), "jacobi": 0.8 / np.diag(A), None: None}[precon]      # (damped Jacobi)
    beta = np.abs(b).max() if ttype is ABS else np.linalg.norm(b)

    def run(vec, wrap):
        return S.schwarz_ddm_solver(wrap(A), b, None if M is None else wrap(M), max_iterations, S.FittingAccuracy(1e-9, ttype),
                                    vectors=vec)

    x, hist = compare(run, ttype is ABS, beta)
    if precon is None:
        assert hist == [] and not x.any()                          # the reference returns the zero vector
    elif max_iterations == 5:
        assert len(hist) == 5 and hist[-1][1] > 1e-9               # ran out of iterations
    else:
        assert hist[-1][1] <= 1e-9 and np.abs(A @ x - b).max() < 1e-7 * np.abs(b).max()


# ------------------------------------------------------------------------------------------------ 3. device operators
OPERATOR_CASES = {"linear_drift_nugget": (0, 1, 0.1, 1.0), "spheroidal_no_drift": (3, None, 0.0, 0.3)}


@functools.lru_cache(maxsize=None)
def operators(name):
    kid, drift, nugget, br = OPERATOR_CASES[name]
    rng = np.random.default_rng(31)
    pts = rng.random((5000, 3))
    st = InterpolantSettings(kid, 3, drift=drift, nugget=nugget, base_range=br, total_sill=br)
    tree = F.FmmTree(pts, 6, F.KernelParams(F.KernelType(kid), base_range=br, total_sill=br), True, True, deterministic=True)
    pre = SchwarzPreconditioner(tree, pts, st, DDMParams(128, 0.5, 0.125, 512))
    op = S.RbfSystemOperator(tree, st.basis_size, pre.monomial_matrix, nugget)
    return pts, st, tree, pre, op


@pytest.mark.parametrize("name", list(OPERATOR_CASES))
def test_system_operator_device_apply_equals_the_host_apply(name):
    import torch
    pts, st, tree, pre, op = operators(name)
    n, m = len(pts), st.basis_size
    assert m == (4 if name == "linear_drift_nugget" else 0)
    x = np.random.default_rng(32).standard_normal(n + m)
    xt = torch.from_numpy(x).cuda()
    y = op(x)
    yd = op.apply_device(xt).cpu().numpy()
    print(name, "system operator difference / max|y|", np.abs(yd[:n] - y[:n]).max() / np.abs(y).max())
    assert np.abs(yd[:n] - y[:n]).max() <= 1e-12 * np.abs(y).max()
    assert yd.shape == (n + m,) and not yd[n:].any() and not y[n:].any()       # the last basis_size rows are exactly 0
    again = op.apply_device(xt).cpu().numpy()                      # the same input vector reused across calls
    assert np.array_equal(again, yd) and np.array_equal(xt.cpu().numpy(), x)


@pytest.mark.parametrize("name", list(OPERATOR_CASES))
def test_schwarz_device_apply_equals_the_host_apply(name):
    import torch
    pts, st, tree, pre, op = operators(name)
    n, m = len(pts), st.basis_size
    r = np.random.default_rng(33).standard_normal(n + m)
    r[n:] = 0.0
    rt = torch.from_numpy(r).cuda()
    z = pre(r)
    zd = pre.apply_device(rt).cpu().numpy()
    print(name, "schwarz apply difference / max|z|", np.abs(zd - z).max() / np.abs(z).max(), "tail", z[n:], zd[n:])
    assert np.abs(zd - z).max() <= 1e-13 * np.abs(z).max()        # the same sweep on the same device buffers, tail included
    if m:
        assert z[n:].any()                                         # the case has a polynomial tail to carry
    again = pre.apply_device(rt).cpu().numpy()
    assert np.array_equal(again, zd) and np.array_equal(rt.cpu().numpy(), r)


def test_native_operators_of_different_trees_or_streams_are_refused():
    import torch
    pts, st, tree, pre, op = operators("spheroidal_no_drift")
    other = F.FmmTree(pts, 6, F.KernelParams(F.KernelType(3), base_range=0.3, total_sill=0.3), True, True, deterministic=True)
    op2 = S.RbfSystemOperator(other, 0, None, 0.0)
    with pytest.raises(RuntimeError, match="different trees"):
        S.fgmres(op2, np.ones(len(pts)), pre, vectors="device")
    lib = L.load()
    x = torch.zeros(len(pts), dtype=torch.float64, device="cuda")
    y = torch.zeros_like(x)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert side.cuda_stream != tree.stream()
    for dop in (op._dop, pre._dop):
        fn = ctypes.cast(dop.fn_ptr, L.APPLY_DEVICE_FN)
        assert fn(dop.user_ptr, x.data_ptr(), y.data_ptr(), x.numel(), side.cuda_stream) == L.BAD_ARGUMENT
    it, res = ctypes.c_int64(0), ctypes.c_double(0.0)
    rc = lib.bbfmm_fgmres_device(x.numel(), op._dop.fn_ptr, op._dop.user_ptr, x.data_ptr(), None, None, None, 2, 2, 1, 1e-6, None, None,
                                 y.data_ptr(), ctypes.byref(it), ctypes.byref(res), side.cuda_stream)
    assert rc == L.BAD_ARGUMENT and b"stream" in lib.bbfmm_last_error(tree._h)


# ------------------------------------------------------------------------------------------------ 4. the fit
TOL = 1e-6
# seeds at which the HOST solver crosses the tolerance clear of it (first residual below < 0.95 tol, the one before
# > 1.05 tol) for both value columns: the iteration counts of the two routes then cannot legitimately differ
FIT_SEEDS = {(3, "FGMRES"): 0, (3, "DDM"): 0, (2, "FGMRES"): 0}


def fit_data(dim, seed):
    rng = np.random.default_rng(seed)
    n = 6000 if dim == 3 else 5000
    pts = rng.random((n, dim))
    smooth = np.sin(4 * pts[:, 0]) * np.cos(3 * pts[:, -1])
    vals = np.stack([smooth + pts[:, 0] - 0.5 * pts[:, 1], np.cos(5 * pts[:, 1]) * pts[:, 0] + 2.0 * pts[:, -1]], axis=1)
    return pts, vals


@functools.lru_cache(maxsize=None)
def fit(dim, solver, vectors_, repeat=0):
    pts, vals = fit_data(dim, FIT_SEEDS[(dim, solver)])
    kernel = R.RBFKernelType.Linear if dim == 3 else R.RBFKernelType.ThinPlateSpline
    settings = R.InterpolantSettings(kernel, fitting_accuracy=R.FittingAccuracy(TOL, R.FittingAccuracyType.Relative))
    params = R.Params(kernel, solver_type=R.Solvers[solver], deterministic=True, solver_vectors=vectors_)
    return R.RBFInterpolator(pts, vals, settings, params), pts, vals


def crosses_clear_of_the_tolerance(history):
    res = [r for _, r in history]
    k = next(i for i, r in enumerate(res) if r < TOL)
    return res[k] < 0.95 * TOL and (k == 0 or res[k - 1] > 1.05 * TOL)


@pytest.mark.parametrize("dim,solver", list(FIT_SEEDS))
def test_device_fit_equals_the_host_fit(dim, solver):
    host, pts, vals = fit(dim, solver, "host")
    dev, _, _ = fit(dim, solver, "device")
    assert len(host.residual_histories) == len(dev.residual_histories) == 2    # the operators are reused across the columns
    for c in range(2):
        hh, hd = host.residual_histories[c], dev.residual_histories[c]
        assert crosses_clear_of_the_tolerance(hh), hh                           # the precondition, on the host run alone
        assert len(hh) == len(hd), (hh, hd)
        diff = max(abs(a - b) / b for (_, b), (_, a) in zip(hh, hd))
        print(dim, solver, "column", c, "iterations", len(hh), "largest relative history difference", diff)
        assert diff < 1e-8, (hh, hd)
    ch, cd = host.coefficients, dev.coefficients
    rel = np.abs(cd.point_coefficients - ch.point_coefficients).max(axis=0) / np.abs(ch.point_coefficients).max(axis=0)
    print(dim, solver, "coefficients", rel)
    assert np.all(rel < 1e-6)
    assert np.abs(cd.poly_coefficients - ch.poly_coefficients).max() < 1e-6 * np.abs(ch.poly_coefficients).max()
    fitted = dev.evaluate_at_source()
    assert np.abs(fitted - vals).max() < 1e-4 * np.abs(vals).max()


def test_two_device_fits_give_the_same_bits():
    a, _, _ = fit(3, "FGMRES", "device")
    b, _, _ = fit(3, "FGMRES", "device", repeat=1)
    assert a is not b and a.residual_histories == b.residual_histories
    assert np.array_equal(a.coefficients.point_coefficients, b.coefficients.point_coefficients)
    assert np.array_equal(a.coefficients.poly_coefficients, b.coefficients.poly_coefficients)


# ------------------------------------------------------------------------------------------------ 5. device in, device out
def test_tensors_in_tensor_out_equals_the_numpy_route():
    import torch
    pts, st, tree, pre, op = operators("linear_drift_nugget")
    n, m = len(pts), st.basis_size
    rhs = np.concatenate([np.sin(4 * pts[:, 0]) + pts[:, 1], np.zeros(m)])
    x_np, h_np = S.fgmres(op, rhs, pre, None, 20, 5, S.FittingAccuracy(1e-6), vectors="device")
    assert isinstance(x_np, np.ndarray) and h_np[-1][1] < 1e-6
    rhs_t = torch.from_numpy(rhs).to(torch.device("cuda", tree.device()))
    x_t, h_t = S.fgmres(op, rhs_t, pre, None, 20, 5, S.FittingAccuracy(1e-6), vectors="device")
    assert isinstance(x_t, torch.Tensor) and x_t.device == rhs_t.device and x_t.dtype == torch.float64
    assert h_t == h_np and np.array_equal(x_t.cpu().numpy(), x_np)
    x_s, h_s = S.schwarz_ddm_solver(op, rhs_t, pre, 100, S.FittingAccuracy(1e-6), vectors="device")
    x_sn, h_sn = S.schwarz_ddm_solver(op, rhs, pre, 100, S.FittingAccuracy(1e-6), vectors="device")
    assert isinstance(x_s, torch.Tensor) and h_s == h_sn and np.array_equal(x_s.cpu().numpy(), x_sn)


# ------------------------------------------------------------------------------------------------ 6. lifecycle
class OperatorFailure(Exception):
    pass


def test_thirty_solves_leave_no_memory_behind_and_errors_are_the_callers():
    import torch
    pts, st, tree, pre, op = operators("linear_drift_nugget")
    n, m = len(pts), st.basis_size
    rhs = np.concatenate([np.cos(3 * pts[:, 2]), np.zeros(m)])
    dev = torch.device("cuda", tree.device())
    rhs_t = torch.from_numpy(rhs).to(dev)
    granule = 2 << 20     # the 2 MiB segments torch's allocator takes small blocks in; the runtime's own granule is no larger

    def failing_operator():
        calls = [0]

        def apply(v):
            calls[0] += 1
            if calls[0] == 3:
                raise OperatorFailure("third call")
            return op.apply_device(v)
        return apply

    free_after_first = None
    for i in range(30):
        if i % 10 == 5:                                            # through the error path: the workspace is freed there too
            with pytest.raises(OperatorFailure, match="third call"):
                S.fgmres(failing_operator(), rhs_t, pre, None, 20, 5, S.FittingAccuracy(1e-6), vectors="device")
        elif i % 2:
            S.schwarz_ddm_solver(op, rhs_t, pre, 100, S.FittingAccuracy(1e-4), vectors="device")
        else:
            S.fgmres(op, rhs_t, pre, None, 20, 5, S.FittingAccuracy(1e-6), vectors="device")
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()                                   # (torch's own cached blocks are not the solver's)
        if i == 0:
            free_after_first = torch.cuda.mem_get_info(dev)[0]
    assert abs(torch.cuda.mem_get_info(dev)[0] - free_after_first) <= granule
