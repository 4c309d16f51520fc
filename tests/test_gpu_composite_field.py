"""Composite fields on the device (bbfmm_isosurfaces_from_fields_opts), on deterministic handles: one MODEL operand is the
tree's own extraction bit for bit; one HEIGHT operand over a 2-D tree is x[axis] - g; maximum(model - c, height) is the
restatement of the program on the two single-operand fields bit for bit; a box of six affines needs no tree and is a
closed mesh; and what the entry refuses."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import composite_cases as CC
import field_program_restatement as FR
import interpolant_restatement as IR
import isosurface_restatement as R
import ferreus_rbf_rs_amd as F
from ferreus_rbf_rs_amd import _lib as L
from ferreus_rbf_rs_amd import rmt

EXT, RES, same_mesh = CC.EXT, CC.RES, CC.same_mesh
MODEL, HEIGHT, AFFINE = L.FIELD_MODEL, L.FIELD_HEIGHT, L.FIELD_AFFINE
C_OFFSET = 0.2                                        # the model's level: a sphere of radius 2.0, cut by the topography near z = 3.4


@pytest.fixture(scope="module")
def lattice():
    lat = R.Lattice(EXT, RES)
    nodes = lat.e_nodes()
    return lat, nodes, lat.world(nodes), tuple((nodes - lat.lo)[:, ::-1].T)


def on_e(field, lat):
    assert field.shape == lat.shape and np.array_equal(np.isnan(field), ~lat.inE)
    return field[lat.inE]


def same_field(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a).view(np.uint64),
                                                                                             np.nan_to_num(b).view(np.uint64))


# ---- 1. one MODEL operand is the tree's own extraction
@pytest.mark.parametrize("cluster", ["none", "curvature"])
@pytest.mark.parametrize("follow", ["dense", "surface"])
@pytest.mark.parametrize("with_terms", [False, True])
def test_one_model_operand_is_the_tree_extraction_bit_for_bit(with_terms, follow, cluster):
    if with_terms:                                                   # a quadratic drift and a global trend
        fit, tree = CC.model()
        terms, seeds, iso = fit.terms(1), fit.source_points, [0.0, -0.3]
    else:                                                            # the tree's kernel sum alone
        seeds, tree, level = CC.plain()
        terms, iso = None, [level]
    kw = dict(cluster=cluster, follow=follow, seeds=seeds if follow == "surface" else None, return_field=True)
    want, wfield = tree.build_isosurfaces(EXT, RES, iso, drift=terms, **kw)
    got, gfield = rmt.isosurfaces_from_fields([rmt.BoundOperand(MODEL, tree, terms)], [0], EXT, RES, iso, **kw)
    assert same_field(wfield, gfield)
    assert len(want) == len(got) == len(iso)
    for w, g in zip(want, got):
        assert len(w[1]) > 200 and same_mesh(w, g)


# ---- 2. one HEIGHT operand over a 2-D tree
def height_reference(axis, with_terms, world):
    fit, tree = CC.topo()
    uv = np.asfortranarray(world[:, [a for a in range(3) if a != axis]])
    g = tree.evaluate_leaves(None, uv)[:, 0]
    if with_terms:
        g = g + IR.polynomial(uv, 1, fit.coefficients.poly_coefficients, fit.translation_factor, fit.scale_factor)[0][:, 0]
    return world[:, axis] - g, g


@pytest.mark.parametrize("axis, with_terms", [(2, False), (0, False), (2, True), (0, True)])
def test_one_height_operand_is_the_axis_minus_the_2d_interpolant(lattice, axis, with_terms):
    lat, nodes, world, sel = lattice
    fit, tree = CC.topo()
    terms = fit.terms(1) if with_terms else None
    assert terms is None or (terms.d == 2 and terms.degree == 1)
    (mesh,), field = rmt.isosurfaces_from_fields([rmt.BoundOperand(HEIGHT, tree, terms, axis=axis)], [0], EXT, RES, [0.0],
                                                 return_field=True)
    want, g = height_reference(axis, with_terms, world)
    err, bound = float(np.abs(on_e(field, lat) - want).max()), 1e-12 * float(np.abs(g).max())
    CC.record(f"height_axis{axis}_{'drift' if with_terms else 'kernel_sum'}_max_abs_error", err, bound)
    assert err <= bound
    assert same_mesh(mesh, F.isosurface_from_values(field, EXT, RES, 0.0))
    if with_terms:                                                   # the fitted topography: the sheet x[axis] = g(u, v)
        assert len(mesh[1]) > 500
        uv = mesh[0][:, [a for a in range(3) if a != axis]]
        inside = (np.abs(uv - 3.0) < 2.4).all(axis=1)
        assert float(np.abs(mesh[0][inside, axis] - CC.topography(uv[inside])).max()) < 0.1


def interpolant_reference(fit, axes, x):
    """values (m,) and gradients (m, d) of a fitted interpolant at the world points x: RBFInterpolator's own Leaves-mode
    evaluation (trend map, host-target evaluate_leaves_with_gradients, trend_gradients, polynomial) on the evaluator tree
    that CC.evaluator builds"""
    fit.build_evaluator(CC.evaluator_extents(fit, axes))
    v, g = fit.evaluate_targets_with_gradients(np.ascontiguousarray(x))
    return np.asarray(v)[:, 0], np.asarray(g).reshape(len(x), len(axes))


@pytest.mark.parametrize("case", ["drift", "trend"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_height_operand_values_and_gradients_at_points(axis, case):
    """The operand column and its three gradient columns, as the seed projection gets them: x[axis] - g and e_axis minus
    grad g on the other two axes in ascending order, times the operand's scale (offset added to the value alone).  g and
    grad g come from the interpolator's host-target Leaves evaluation of the same tree; the bounds are the standing one of
    two batchings of one leaf pass, 1e-12 of the largest |g| for values and of the largest |grad g| for gradients (the same
    sums with the kernel's derivative in place of its value)."""
    fit, tree = CC.topo() if case == "drift" else CC.topo_trend()
    x = np.random.default_rng(21 + axis).uniform(0.2, 5.8, (700, 3))
    uv_axes = [a for a in range(3) if a != axis]
    g, gg = interpolant_reference(fit, (0, 1), x[:, uv_axes])
    scale, offset = -0.5, 0.3
    v, grad = rmt.evaluate_fields([rmt.BoundOperand(HEIGHT, tree, fit.terms(1), axis=axis, scale=scale, offset=offset)], [0], x, True)
    want_v = scale * (x[:, axis] - g) + offset
    want_g = np.zeros((len(x), 3))
    want_g[:, axis] = scale
    want_g[:, uv_axes[0]], want_g[:, uv_axes[1]] = -scale * gg[:, 0], -scale * gg[:, 1]
    err_v, bound_v = float(np.abs(v - want_v).max()), 1e-12 * float(np.abs(g).max())
    err_g, bound_g = float(np.abs(grad - want_g).max()), 1e-12 * float(np.abs(gg).max())
    CC.record(f"height_points_axis{axis}_{case}_max_value_error", err_v, bound_v)
    CC.record(f"height_points_axis{axis}_{case}_max_gradient_error", err_g, bound_g)
    assert err_v <= bound_v and err_g <= bound_g
    # the two slopes differ, so a swap of u and v or a wrong sign is far outside the bound
    assert float(np.abs(gg[:, 0] - gg[:, 1]).max()) > 0.05 and float(np.abs(gg).max()) > 0.05
    # central differences of the operand's own values agree with its gradient columns (to 1e-2: the Linear kernel |r| has
    # a kink at every data point, and a wrong sign or a swap of columns is 0.05 or more)
    h = 1e-5
    for a in range(3):
        step = np.zeros(3)
        step[a] = h
        ops = [rmt.BoundOperand(HEIGHT, tree, fit.terms(1), axis=axis, scale=scale, offset=offset)]
        diff = (rmt.evaluate_fields(ops, [0], x + step) - rmt.evaluate_fields(ops, [0], x - step)) / (2 * h)
        assert float(np.abs(diff - grad[:, a]).max()) < 1e-2


def test_model_operand_and_max_gradients_at_points():
    """a MODEL operand's gradient is the interpolator's; under MAX the gradient travels with the value chosen"""
    (fit3, tree3), (fit2, tree2) = CC.model(), CC.topo()
    x = np.random.default_rng(31).uniform(0.6, 5.4, (700, 3))
    f, fg = interpolant_reference(fit3, (0, 1, 2), x)
    m_op = rmt.BoundOperand(MODEL, tree3, fit3.terms(1), offset=-C_OFFSET)
    h_op = rmt.BoundOperand(HEIGHT, tree2, fit2.terms(1), axis=2)
    v, grad = rmt.evaluate_fields([m_op], [0], x, True)
    assert float(np.abs(v - (f - C_OFFSET)).max()) <= 1e-12 * float(np.abs(f).max())
    assert float(np.abs(grad - fg).max()) <= 1e-12 * float(np.abs(fg).max())
    hv, hgrad = rmt.evaluate_fields([h_op], [0], x, True)
    bv, bgrad = rmt.evaluate_fields([m_op, h_op], [0, 1, L.FIELD_OP_MAX], x, True)
    first = v >= hv
    assert first.any() and (~first).any()
    assert np.array_equal(bv.view(np.uint64), np.where(first, v, hv).view(np.uint64))
    assert np.array_equal(bgrad.view(np.uint64), np.where(first[:, None], grad, hgrad).view(np.uint64))
    with pytest.raises(F.PointOutsideTree, match="operand 0"):
        rmt.evaluate_fields([m_op], [0], np.array([[3.0, 3.0, 400.0]]))


def test_height_operand_with_a_2d_trend_on_the_lattice(lattice):
    """the d = 2 trend path: the map of (u, v) on the device, the 4 transformed corners of the pre-flight test"""
    lat, nodes, world, sel = lattice
    fit, tree = CC.topo_trend()
    op = [rmt.BoundOperand(HEIGHT, tree, fit.terms(1), axis=2)]
    (mesh,), field = rmt.isosurfaces_from_fields(op, [0], EXT, RES, [0.0], return_field=True)
    g, _ = interpolant_reference(fit, (0, 1), world[:, :2])
    err, bound = float(np.abs(on_e(field, lat) - (world[:, 2] - g)).max()), 1e-12 * float(np.abs(g).max())
    CC.record("height_axis2_trend_max_abs_error", err, bound)
    assert err <= bound and len(mesh[1]) > 500
    uv = fit.source_points[::7]
    seeds = np.column_stack([uv, CC.topography(uv) + 0.35])
    (followed,) = rmt.isosurfaces_from_fields(op, [0], EXT, RES, [0.0], follow="surface", seeds=seeds)
    assert same_mesh(mesh, followed)
    with pytest.raises(F.PointOutsideTree, match="operand 0"):          # the transformed corners are tested
        rmt.isosurfaces_from_fields(op, [0], [-40.0, 0.0, 0.0, 6.0, 6.0, 6.0], RES, [0.0])


def test_height_along_x_followed_from_seeds_displaced_sideways(monkeypatch):
    """axis = 0: the sheet x = g(y, z), seeds displaced along y and z as well, with the composite GradFn and with central
    differences; both reach the dense mesh"""
    fit, tree = CC.topo()
    op = [rmt.BoundOperand(HEIGHT, tree, fit.terms(1), axis=0)]
    (dense,) = rmt.isosurfaces_from_fields(op, [0], EXT, RES, [0.0])
    yz = fit.source_points[::7]
    seeds = np.column_stack([CC.topography(yz) + 0.3, yz[:, 0] + 0.25, yz[:, 1] - 0.25])
    for gradients in ("leaf_pass", "differences"):
        monkeypatch.setenv("BBFMM_ISO_SEED_GRADIENTS", gradients)
        (followed,) = rmt.isosurfaces_from_fields(op, [0], EXT, RES, [0.0], follow="surface", seeds=seeds, return_stats=True)
        assert followed[2]["follow"]["newton_steps"] >= 1 and len(dense[1]) > 500
        assert same_mesh(dense, followed[:2])


@pytest.mark.parametrize("gradients", ["leaf_pass", "differences"])
def test_height_gradients_follow_the_surface_to_the_dense_mesh(monkeypatch, gradients):
    """The seed projection with the composite GradFn (e_axis minus grad g through the 2-D leaf pass, its trend and
    polynomial gradient) and with central differences of the composite value: both reach the one sheet, and on a
    deterministic handle with terms every node's value is the same double in both passes."""
    fit, tree = CC.topo()
    op = [rmt.BoundOperand(HEIGHT, tree, fit.terms(1), axis=2)]
    (dense,) = rmt.isosurfaces_from_fields(op, [0], EXT, RES, [0.0])
    uv = fit.source_points[::7]
    seeds = np.column_stack([uv, CC.topography(uv) + 0.35])          # off the sheet: the projection has to move them
    monkeypatch.setenv("BBFMM_ISO_SEED_GRADIENTS", gradients)
    (followed,) = rmt.isosurfaces_from_fields(op, [0], EXT, RES, [0.0], follow="surface", seeds=seeds, return_stats=True)
    st = followed[2]["follow"]
    assert st["newton_steps"] >= 1 and 0 < st["nodes_evaluated"] < st["nodes"]
    assert same_mesh(dense, followed[:2])


# ---- 3. the model cut off at the topography
@pytest.fixture(scope="module")
def clipped(lattice):
    lat = lattice[0]
    (fit3, tree3), (fit2, tree2) = CC.model(), CC.topo()
    m_op = rmt.BoundOperand(MODEL, tree3, fit3.terms(1))
    h_op = rmt.BoundOperand(HEIGHT, tree2, fit2.terms(1), axis=2)
    (_,), f_model = rmt.isosurfaces_from_fields([m_op], [0], EXT, RES, [0.0], return_field=True)
    (_,), f_height = rmt.isosurfaces_from_fields([h_op], [0], EXT, RES, [0.0], return_field=True)
    ops = [rmt.BoundOperand(MODEL, tree3, fit3.terms(1), offset=-C_OFFSET), h_op]
    (mesh,), f_both = rmt.isosurfaces_from_fields(ops, [0, 1, L.FIELD_OP_MAX], EXT, RES, [0.0], return_field=True)
    return ops, mesh, f_both, f_model, f_height


def test_clipped_model_is_the_program_on_the_two_fields_bit_for_bit(lattice, clipped):
    lat = lattice[0]
    ops, mesh, f_both, f_model, f_height = clipped
    V = np.stack([on_e(f_model, lat), on_e(f_height, lat)], axis=1)
    want = FR.program([1.0, 1.0], [-C_OFFSET, 0.0], [0, 1, FR.OP_MAX], V)[0]
    assert np.array_equal(on_e(f_both, lat).view(np.uint64), want.view(np.uint64))
    assert len(mesh[1]) > 500 and same_mesh(mesh, F.isosurface_from_values(f_both, EXT, RES, 0.0))
    # both branches of the max own part of the surface: lattice edges (the 7 owned deltas) with their ends on opposite sides
    # of 0 and the same branch at both ends
    first = (f_model - C_OFFSET) >= f_height
    by_model = by_height = 0
    for delta in R.ED[:7]:
        near, far = [], []
        for axis, step in enumerate(int(s) for s in delta[::-1]):    # arrays are (nk, nj, ni)
            n = f_both.shape[axis]
            near.append(slice(0, n - step) if step >= 0 else slice(-step, n))
            far.append(slice(step, n) if step >= 0 else slice(0, n + step))
        near, far = tuple(near), tuple(far)
        crossing = ((f_both[near] < 0.0) != (f_both[far] < 0.0)) & np.isfinite(f_both[near]) & np.isfinite(f_both[far])
        by_model += int((crossing & first[near] & first[far]).sum())
        by_height += int((crossing & ~first[near] & ~first[far]).sum())
    print("lattice edges crossed on the model's branch:", by_model, "on the height's branch:", by_height)
    assert by_model > 100 and by_height > 100
    # it is not the unclipped model's surface
    (unclipped,) = rmt.isosurfaces_from_fields(ops[:1], [0], EXT, RES, [0.0])
    assert not same_mesh(mesh, unclipped) and float(mesh[0][:, 2].max()) < float(unclipped[0][:, 2].max()) - 0.5
    assert R.directed_edges_once(mesh[1]) and R.euler_characteristic(*mesh) == 2       # closed at the topography


def test_clipped_model_followed_from_seeds_is_the_dense_mesh(clipped):
    ops, mesh = clipped[0], clipped[1]
    fit3 = CC.model()[0]
    (followed,) = rmt.isosurfaces_from_fields(ops, [0, 1, L.FIELD_OP_MAX], EXT, RES, [0.0], follow="surface", seeds=fit3.source_points,
                                              return_stats=True)
    st = followed[2]["follow"]
    assert 0 < st["nodes_evaluated"] < st["nodes"] and st["newton_steps"] >= 1
    assert same_mesh(mesh, followed[:2])


def test_field_expression_of_interpolators_through_build_isosurface():
    """the reference's isosurface_linear_topo through the public surface: evaluator trees built inside the call"""
    (fit3, _), (fit2, _) = CC.model(), CC.topo()
    expr = rmt.maximum(rmt.field(fit3) - C_OFFSET, rmt.height_field(fit2, axis=2))
    events = []
    mesh, field = rmt.build_isosurface(fit3.source_points, np.array(EXT), RES, 0.0, expr, cluster_method=rmt.ClusterMethod.None_,
                                       follow="dense", finish="raw", self_intersections="ignore", return_field=True,
                                       progress_callback=rmt.Progress(events.append))
    assert isinstance(mesh, rmt.Mesh) and [e.stage for e in events] == ["started", "finished"]
    assert same_mesh((mesh.vertices, mesh.facets), F.isosurface_from_values(field, EXT, RES, 0.0))
    default = rmt.build_isosurface(fit3.source_points, EXT, RES, 0.0, expr)             # curvature clusters, followed, clipped, rollback
    assert 0 < len(default.facets) < len(mesh.facets)
    top = default.vertices[:, 2] > 3.0
    assert float(np.abs(default.vertices[top, 2] - CC.topography(default.vertices[top, :2])).min()) < 0.05


# ---- 4. affine operands alone
def test_box_of_six_affines_needs_no_tree_and_is_closed(lattice):
    lat, nodes, world, sel = lattice
    box = [1.3, 1.1, 1.7, 4.9, 4.4, 4.6]                             # strictly inside the extents
    operands, program = rmt.compile_expr(rmt.box(box))
    bound = [rmt.BoundOperand(AFFINE, coefficients=o.coefficients) for o in operands]
    (mesh,), field = rmt.isosurfaces_from_fields(bound, program, EXT, RES, [0.0], return_field=True)
    V = np.stack([FR.affine(c, world) for c in FR.box_planes(box)], axis=1)
    want = FR.program([1.0] * 6, [0.0] * 6, program, V)[0]
    assert np.array_equal(on_e(field, lat).view(np.uint64), want.view(np.uint64))
    assert same_mesh(mesh, F.isosurface_from_values(field, EXT, RES, 0.0))
    assert len(mesh[1]) > 500 and R.directed_edges_once(mesh[1]) and R.euler_characteristic(*mesh) == 2
    lo, hi = mesh[0].min(0), mesh[0].max(0)
    assert (np.abs(lo - box[:3]) < 1e-9).all() and (np.abs(hi - box[3:]) < 1e-9).all()
    # with a scale, an offset and NEG: the same restatement
    bound[0] = rmt.BoundOperand(AFFINE, coefficients=operands[0].coefficients, scale=-0.5, offset=0.25)
    prog2 = [0, L.FIELD_OP_NEG] + program[1:]
    (_,), field2 = rmt.isosurfaces_from_fields(bound, prog2, EXT, RES, [0.0], return_field=True)
    want2 = FR.program([-0.5] + [1.0] * 5, [0.25] + [0.0] * 5, prog2, V)[0]
    assert np.array_equal(on_e(field2, lat).view(np.uint64), want2.view(np.uint64))


# ---- 5. refusals
def test_refusals():
    (fit3, tree3), (fit2, tree2) = CC.model(), CC.topo()
    with pytest.raises(F.PointOutsideTree, match="operand 1"):                          # a lattice outside the height operand's square
        rmt.isosurfaces_from_fields([rmt.BoundOperand(AFFINE, coefficients=[0, 0, 0, 1]), rmt.BoundOperand(HEIGHT, tree2, axis=2)],
                                    [0, 1, L.FIELD_OP_MAX], [0.0, -40.0, 0.0, 6.0, 6.0, 6.0], RES, [0.0])
    with pytest.raises(F.PointOutsideTree, match="operand 0"):
        rmt.isosurfaces_from_fields([rmt.BoundOperand(MODEL, tree3, fit3.terms(1))], [0], [-40.0, 0.0, 0.0, 6.0, 6.0, 6.0], RES, [0.0])
    with pytest.raises(F.FmmError, match="operand 0.*d = 2"):                           # a d = 3 handle as HEIGHT
        rmt.isosurfaces_from_fields([rmt.BoundOperand(HEIGHT, tree3)], [0], EXT, RES, [0.0])
    with pytest.raises(F.FmmError, match="operand 0.*terms"):                           # 3-D terms on a 2-D handle
        rmt.isosurfaces_from_fields([rmt.BoundOperand(HEIGHT, tree2, fit3.terms(1))], [0], EXT, RES, [0.0])
    bare = F.FmmTree(fit2._tpoints, 7, fit2.settings.kernel_params(), True, False, deterministic=True)
    with pytest.raises(F.FmmError, match="operand 0.*set_local_coefficients"):          # no local coefficients
        rmt.isosurfaces_from_fields([rmt.BoundOperand(HEIGHT, bare)], [0], EXT, RES, [0.0])
    bare.set_weights(np.asfortranarray(fit2.coefficients.point_coefficients))
    with pytest.raises(F.FmmError, match="operand 0.*set_local_coefficients"):
        rmt.isosurfaces_from_fields([rmt.BoundOperand(HEIGHT, bare)], [0], EXT, RES, [0.0])
    # a handle on a device group (two logical parts on one device), ready for Leaves mode, cannot be an operand
    pts, _, _ = CC.plain()
    group = F.FmmTree(pts, 7, F.KernelParams(F.FmmKernelType.LinearRbf), True, False, deterministic=True, devices=[0, 0])
    assert group.device_count() == 2
    w = np.asfortranarray(np.ones((len(pts), 1)))
    group.set_weights(w)
    group.set_local_coefficients(w)
    with pytest.raises(F.FmmError, match="operand 0.*device group") as refused:
        rmt.isosurfaces_from_fields([rmt.BoundOperand(MODEL, group)], [0], EXT, RES, [0.0])
    assert not isinstance(refused.value, F.PointOutsideTree)                            # BBFMM_BAD_ARGUMENT
    with pytest.raises(ValueError):
        rmt.isosurfaces_from_fields([rmt.BoundOperand(MODEL, tree3)], [0], EXT, RES, [0.0], follow="surface")       # no seeds
    # options->terms belongs to the operands
    lib = L.load()
    terms = fit3.terms(1)._c()
    opts = L.IsosurfaceOptions(ctypes.sizeof(L.IsosurfaceOptions))
    opts.terms = ctypes.addressof(terms)
    arr, keep, _ = rmt._c_operands([rmt.BoundOperand(MODEL, tree3)])
    prog, ext, iso, res = np.zeros(1, np.int32), np.array(EXT), np.array([0.0]), ctypes.c_void_p()
    rc = lib.bbfmm_isosurfaces_from_fields_opts(arr, 1, prog.ctypes.data, 1, ext.ctypes.data, RES, iso.ctypes.data, 1, None,
                                                ctypes.addressof(opts), ctypes.byref(res))
    assert rc == L.BAD_ARGUMENT and b"terms" in lib.bbfmm_isosurface_error(res)
    lib.bbfmm_isosurface_destroy(res)
    # the handles stay usable
    (mesh,) = rmt.isosurfaces_from_fields([rmt.BoundOperand(MODEL, tree3, fit3.terms(1))], [0], EXT, RES, [0.0])
    assert len(mesh[1]) > 200
