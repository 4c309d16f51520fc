"""Boundary closure on the device (finish="close_positive" / "close_negative", close_mesh) against the contract of
DESIGN.md "Boundary closure": invariants of a closed mesh, the numpy restatement (tests/isosurface_closure_restatement.py)
and exact volumes.  Small boxes throughout: about 10 cap cells a side."""
import numpy as np
import pytest

import isosurface_restatement as R
import isosurface_finish_restatement as FR
import isosurface_closure_restatement as CR
from test_gpu_isosurface import _tree, fit  # noqa: F401  (fit: a fixture)

pytestmark = pytest.mark.gpu

EXT, RES = FR.EXT, 0.7                       # 9 x 9 x 9 cap cells on the extents of the finish tests
BOX = float(np.prod(np.asarray(EXT[3:]) - np.asarray(EXT[:3])))
UNIT = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
MODES = ("close_positive", "close_negative")


def _reversed(f):
    return f[:, [0, 2, 1]]


def _on_face(v, f, face, ext):
    """The facets with all three vertices on `face`."""
    c = ext[(face >> 1) + 3 * (face & 1)]
    return (v[f][:, :, face >> 1] == c).all(1)


# ---- a caller's own meshes: the situations of the reference's unit tests
def _sheet(z):
    return np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]], float), np.array([[0, 1, 2], [0, 2, 3]])   # normal +z


@pytest.mark.parametrize("z,res", [(0.5, 0.25), (0.37, 0.5)])
def test_a_horizontal_sheet_through_the_unit_box(z, res):
    import ferreus_rbf_rs_amd as F
    v, f = _sheet(z)
    out = {}
    for mode in MODES:
        cv, cf, st = F.close_mesh(v, f, UNIT, res, mode, return_stats=True)
        print(mode, len(cv), len(cf), st)
        CR.check_closed(cv, cf, 2, UNIT)
        assert np.array_equal(cv[:4], v) and np.array_equal(cf[:2], f if mode == "close_positive" else _reversed(f))
        assert st["open_edges"] == [1, 1, 1, 1, 0, 0] and st["conflicts"] == 0 and st["dropped"] == 0
        out[mode] = (cv, cf)
    (pv, pf), (nv, nf) = out["close_positive"], out["close_negative"]
    assert _on_face(pv, pf[2:], 4, UNIT).sum() == 2 * round(1 / res) ** 2     # positive reaches the bottom, which has no open edge
    assert _on_face(nv, nf[2:], 4, UNIT).sum() == 0 and _on_face(pv, pf[2:], 5, UNIT).sum() == 0
    assert _on_face(nv, nf[2:], 5, UNIT).sum() == 2 * round(1 / res) ** 2
    assert abs(R.enclosed_volume(pv, pf) - z) <= 1e-12 and abs(R.enclosed_volume(nv, nf) - (1 - z)) <= 1e-12
    if z == 0.37:                                                             # off-grid vertices on the box edges
        assert not np.isin(0.37, np.arange(0, 1.01, res)) and (pv[:, 2] == 0.37).sum() >= 4


def test_one_triangle_lying_in_a_face():
    import ferreus_rbf_rs_amd as F
    v, f = np.array([[0.2, 0.2, 0], [0.7, 0.3, 0], [0.4, 0.8, 0]], float), np.array([[0, 1, 2]])
    pv, pf = F.close_mesh(v, f, UNIT, 0.25, "close_positive")
    CR.check_closed(pv, pf, 1, UNIT)
    cap = pv[pf[1:]]                                                          # the triangle's mirror image, over the grid points in it
    area = 0.5 * np.linalg.norm(np.cross(cap[:, 1] - cap[:, 0], cap[:, 2] - cap[:, 0]), axis=1).sum()
    assert abs(area - 0.14) <= 1e-14 and abs(R.enclosed_volume(pv, pf)) <= 1e-15 and (pv[:, 2] == 0).all()
    nv, nf = F.close_mesh(v, f, UNIT, 0.25, "close_negative")
    CR.check_closed(nv, nf, 1, UNIT)
    assert abs(R.enclosed_volume(nv, nf) - 1.0) <= 1e-12


def test_a_closed_mesh_inside_the_box_is_returned_unchanged():
    import ferreus_rbf_rs_amd as F
    v = np.array([[0.2, 0.2, 0.2], [0.8, 0.2, 0.2], [0.2, 0.8, 0.2], [0.2, 0.2, 0.8]])
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])
    for mode in MODES:
        cv, cf, st = F.close_mesh(v, f, UNIT, 0.25, mode, return_stats=True)
        assert np.array_equal(cv, v) and np.array_equal(cf, f) and st["open_edges"] == [0] * 6 and st["vertices_added"] == 0
    ev, ef = F.close_mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int64), UNIT, 0.25, "close_positive")
    assert ev.shape == (0, 3) and ef.shape == (0, 3)


def test_a_rectangle_in_a_face_of_a_box_whose_sides_are_no_multiples_of_the_resolution():
    import ferreus_rbf_rs_amd as F
    ext = [0.0, 0.0, 0.0, 1.1, 0.9, 1.3]
    v = np.array([[1.1, 0.2, 0.3], [1.1, 0.6, 0.3], [1.1, 0.6, 1.0], [1.1, 0.2, 1.0]])
    f = np.array([[0, 1, 2], [0, 2, 3]])
    nv, nf, st = F.close_mesh(v, f, ext, 0.25, "close_negative", return_stats=True)
    CR.check_closed(nv, nf, 2, ext)
    assert np.array_equal(nf[:2], _reversed(f)) and st["open_edges"] == [0, 4, 0, 0, 0, 0]
    pv, pf = F.close_mesh(v, f, ext, 0.25, "close_positive")
    CR.check_closed(pv, pf, 2, ext)
    vols = sorted([abs(R.enclosed_volume(nv, nf)), abs(R.enclosed_volume(pv, pf))])
    assert vols[0] <= 1e-12 and abs(vols[1] - 1.1 * 0.9 * 1.3) <= 1e-12
    assert nv.max(0).tolist() == [1.1, 0.9, 1.3] or pv.max(0).tolist() == [1.1, 0.9, 1.3]   # the last grid coordinate is max


def test_an_open_edge_inside_the_box_is_refused():
    import ferreus_rbf_rs_amd as F
    v, f = np.array([[0.2, 0.2, 0.5], [0.7, 0.3, 0.5], [0.4, 0.8, 0.5]]), np.array([[0, 1, 2]])
    with pytest.raises(F.FmmError, match="3 open edge"):
        F.close_mesh(v, f, UNIT, 0.25, "close_positive")
    with pytest.raises(ValueError):
        F.close_mesh(v, f, UNIT, 0.25, "clipped")


# ---- exact volumes
def _halfspace_volume(ext, n, c):
    """The volume of {x in the box: n . x <= c}: the box's faces clipped by the plane, and the cut polygon."""
    lo, hi = np.asarray(ext[:3], float), np.asarray(ext[3:], float)
    n = np.asarray(n, float)
    polys, cutpts = [], []
    for a in range(3):
        b, d = (a + 1) % 3, (a + 2) % 3
        for side, x in ((0, lo[a]), (1, hi[a])):
            q = np.zeros((4, 3))
            q[:, a] = x
            q[:, b] = [lo[b], hi[b], hi[b], lo[b]]
            q[:, d] = [lo[d], lo[d], hi[d], hi[d]]               # counter-clockwise seen from +a
            if not side:
                q = q[::-1]
            out = []
            for k in range(4):
                p0, p1 = q[k], q[(k + 1) % 4]
                s0, s1 = n @ p0 - c, n @ p1 - c
                if s0 <= 0:
                    out.append(p0)
                if (s0 < 0) != (s1 < 0) and s0 != 0 and s1 != 0:
                    x_ = p0 + (s0 / (s0 - s1)) * (p1 - p0)
                    out.append(x_)
                    cutpts.append(x_)
            if len(out) >= 3:
                polys.append(np.array(out))
    if len(cutpts) >= 3:
        cp = np.unique(np.round(np.array(cutpts), 12), axis=0)
        m = cp.mean(0)
        e0 = np.cross(n, [1.0, 0.3, 0.2])
        e1 = np.cross(n, e0)
        ang = np.arctan2((cp - m) @ e1, (cp - m) @ e0)
        polys.append(cp[np.argsort(ang)])                        # e0 x e1 is along +n: counter-clockwise seen from +n
    vol = 0.0
    for p in polys:
        for k in range(1, len(p) - 1):
            vol += p[0] @ np.cross(p[k], p[k + 1]) / 6.0
    return vol


@pytest.mark.parametrize("cluster", ["none", "average", "curvature"])
def test_an_affine_field_gives_the_volume_of_the_clipped_box(cluster):
    import ferreus_rbf_rs_amd as F
    n, c = np.array([0.31, 0.52, 0.79]), 8.0                     # cuts off the corner region at (hi, hi, hi): three faces
    lat = R.Lattice(EXT, RES)
    field = lat.world(lat.node_ijk()) @ n - c
    want = _halfspace_volume(EXT, n, c)
    assert 0.8 * BOX < want < 0.99 * BOX
    vols = {}
    for mode in MODES:
        v, f, st = F.isosurface_from_values(field, EXT, RES, 0.0, cluster=cluster, finish=mode, return_stats=True)
        CR.check_closed(v, f)
        assert sum(1 for x in st["closure"]["open_edges"] if x) == 3 and st["closure"]["conflicts"] == 0
        vols[mode] = R.enclosed_volume(v, f)
    print(cluster, "volumes", vols, "polytope", want, BOX - want)
    assert abs(vols["close_positive"] - want) <= 1e-9 * want
    assert abs(vols["close_negative"] - (BOX - want)) <= 1e-9 * (BOX - want)


def _field(name, w):
    if name in FR.FIELDS:
        return FR.field(name, w)
    if name == "sphere_through_a_face":
        return np.linalg.norm(w - [1.0, 3.0, 3.2], axis=-1) - 1.6
    if name == "sphere_about_a_corner":
        return np.linalg.norm(w - np.asarray(EXT[3:]), axis=-1) - 2.0
    return np.abs(np.linalg.norm(w - [3.1, 2.9, 0.8], axis=-1) - 2.2) - 0.5      # a shell: annuli on the faces it cuts


ANALYTIC = {"sphere_through_a_face": (4 / 3 * np.pi * 1.6 ** 3 - np.pi * 0.7 ** 2 * (3 * 1.6 - 0.7) / 3, 4 * np.pi * 1.6 ** 2),
            "sphere_about_a_corner": (np.pi * 2.0 ** 3 / 6, 4 * np.pi * 2.0 ** 2)}
ALL_FIELDS = FR.FIELDS + ("sphere_through_a_face", "sphere_about_a_corner", "shell")


@pytest.fixture(scope="module")
def closed():
    """Per field: the lattice field and the clipped, positive and negative meshes with their stats, computed once."""
    import ferreus_rbf_rs_amd as F
    lat = R.Lattice(EXT, RES)
    w = lat.world(lat.node_ijk())
    out = {}
    for name in ALL_FIELDS:
        field = _field(name, w)
        out[name] = {"field": field}
        for fin in ("clipped",) + MODES:
            out[name][fin] = F.isosurface_from_values(field, EXT, RES, 0.0, finish=fin, return_stats=True)
    return out


@pytest.mark.parametrize("name", ALL_FIELDS)
def test_both_modes_are_closed_and_their_volumes_tile_the_box(closed, name):
    m = closed[name]["clipped"]
    vols = {}
    for mode in MODES:
        v, f, st = closed[name][mode]
        print(name, mode, len(v), len(f), st["closure"])
        CR.check_closed(v, f, len(m[1]), EXT)
        assert st["closure"]["conflicts"] == 0 and st["closure"]["dropped"] == 0
        vols[mode] = R.enclosed_volume(v, f)
    print(name, vols, BOX)
    assert abs(vols["close_positive"] + vols["close_negative"] - BOX) <= 1e-10 * BOX
    if name in ANALYTIC:
        want, area = ANALYTIC[name]
        assert abs(vols["close_positive"] - want) <= area * RES
        v, f, _ = closed[name]["close_positive"]
        assert R.euler_characteristic(v, f) == 2                 # one component


@pytest.mark.parametrize("name", ALL_FIELDS)
def test_structure_and_counts_against_the_restatement(closed, name):
    mv, mf, _ = closed[name]["clipped"]
    cut, edges, em = CR.cut_cells(mv, mf, EXT, RES)
    lab, n, off, n_regions = CR.regions(cut)
    assert len(edges) > 0 and em.any(1).all()
    band, whole = {}, {}
    for mode in MODES:
        v, f, st = closed[name][mode]
        # the mesh first, bit for bit the clipped one (reversed for negative); new vertices behind it, in order of first use
        assert np.array_equal(v[:len(mv)].view(np.uint64), mv.view(np.uint64))
        assert np.array_equal(f[:len(mf)], mf if mode == "close_positive" else _reversed(mf))
        cap = f[len(mf):]
        new = cap[cap >= len(mv)]
        _, first = np.unique(new, return_index=True)
        assert np.array_equal(new[np.sort(first)], np.arange(len(mv), len(v))) and st["closure"]["vertices_added"] == len(v) - len(mv)
        c = st["closure"]
        assert c["open_edges"] == em.sum(0).tolist() and c["open_edges_off_box"] == 0
        assert c["cut_cells"] == [int(x.sum()) for x in cut] and c["regions"] == n_regions
        kind = CR.whole_cell_triangles(v, cap, cut, EXT, RES)
        is_whole = kind[:, 1] >= 0
        assert c["band_triangles"] == int((~is_whole).sum()) and 2 * sum(c["whole_cells_kept"]) == int(is_whole.sum())
        # per face: the kept whole cells in cell order, two triangles each, then the band
        faces = kind[:, 0]
        assert (np.diff(faces) >= 0).all()
        for face in range(6):
            k = kind[faces == face]
            nw = c["whole_cells_kept"][face]
            assert (k[:2 * nw, 1] >= 0).all() and (k[2 * nw:, 1] < 0).all()
            assert np.array_equal(k[:2 * nw:2, 1], k[1:2 * nw:2, 1]) and (np.diff(k[:2 * nw:2, 1]) > 0).all()
        band[mode] = np.concatenate([faces[~is_whole, None], cap[~is_whole]], 1)
        whole[mode] = [set(kind[(faces == face) & is_whole, 1].tolist()) for face in range(6)]
    # the selection, restated over the band triangles of both modes (their new vertices renumbered into one list)
    pv, nv = closed[name]["close_positive"][0], closed[name]["close_negative"][0]
    allv = np.concatenate([pv, nv[len(mv):]])
    nb = band["close_negative"].copy()
    nb[:, 1:][nb[:, 1:] >= len(mv)] += len(pv) - len(mv)
    uniq, inv = np.unique(allv, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    inv[:len(mv)] = np.arange(len(mv))                           # mesh vertices keep their ids
    remap = np.concatenate([np.arange(len(mv)), len(mv) + inv[len(mv):]])
    vv = np.concatenate([mv, uniq])
    both = np.concatenate([band["close_positive"], nb])
    both[:, 1:] = remap[both[:, 1:]]
    seeded, regions_seeded = CR.select(vv, both, edges, em, cut, lab, n, off, EXT, RES)
    assert seeded[:len(band["close_positive"])].all() and not seeded[len(band["close_positive"]):].any()
    for face in range(6):
        labels = lab[off[face]:off[face + 1]]
        want = {q for q in range(len(labels)) if labels[q] in regions_seeded}
        assert whole["close_positive"][face] == want
        assert whole["close_negative"][face] == {q for q in range(len(labels)) if labels[q] >= 0} - want


# ---- invariance
def test_the_mesh_does_not_depend_on_runs_batches_or_the_number_of_isovalues(closed):
    import ferreus_rbf_rs_amd as F
    field = closed["torus_cut"]["field"]
    v, f, _ = closed["torus_cut"]["close_positive"]
    again = F.isosurface_from_values(field, EXT, RES, 0.0, finish="close_positive")
    tiny = F.isosurface_from_values(field, EXT, RES, 0.0, finish="close_positive", batch_bytes=1)
    three = F.isosurfaces_from_values(field, EXT, RES, [-0.2, 0.0, 0.15], finish="close_positive")
    for got in (again, tiny, three[1]):
        assert np.array_equal(got[0].view(np.uint64), v.view(np.uint64)) and np.array_equal(got[1], f)
    for got in (three[0], three[2]):
        CR.check_closed(got[0], got[1])


def test_following_the_surface_of_an_fmm_field_gives_the_dense_closed_mesh(fit):
    """On a deterministic handle the field with terms is the same double at a node in every batching (DESIGN.md
    "Batching"; without terms the dense and the followed fields differ in their last bits before any closure runs), so the
    closed mesh of the followed surface is the dense one bit for bit."""
    from ferreus_rbf_rs_amd import rbf as RBF
    pts, coef = fit
    r = 0.5
    ext = [0.4, 0.4, 0.4, 3.4, 5.6, 5.6]                         # x = 3.4 cuts the fitted sphere (centre 3, radius 1.8)
    t = _tree(pts, coef, r, deterministic=True)
    terms = RBF.FieldTerms(3, 1, np.array([0.01, 0.001, -0.002, 0.003])[:, None])
    for cluster in ("none", "curvature"):
        opts = dict(drift=terms, cluster=cluster, self_intersections="rollback")
        dense = t.build_isosurface(ext, r, 0.0, finish="close_negative", **opts)
        follow = t.build_isosurface(ext, r, 0.0, finish="close_negative", follow="surface", seeds=pts, **opts)
        CR.check_closed(dense[0], dense[1])
        print(cluster, "closed: vertices", dense[0].shape, follow[0].shape, "facets equal", np.array_equal(dense[1], follow[1]),
              "max vertex difference", float(np.abs(dense[0] - follow[0]).max()) if dense[0].shape == follow[0].shape else None)
        assert len(dense[1]) > 1000
        assert np.array_equal(dense[0].view(np.uint64), follow[0].view(np.uint64)) and np.array_equal(dense[1], follow[1])


# ---- wiring
def test_the_interpolator_and_rmt_take_the_new_finish_values():
    import composite_cases as CC
    from ferreus_rbf_rs_amd import rbf as RBF, rmt
    model = CC.model()[0]
    ext, res = [2.0, 0.6, 0.6, 5.4, 5.4, 5.4], 0.6                 # x = 2 cuts the model's sphere (centre 3, radius 1.8)
    want = 4 / 3 * np.pi * 1.8 ** 3 - np.pi * 0.8 ** 2 * (3 * 1.8 - 0.8) / 3
    quiet = dict(follow="dense", self_intersections="ignore")
    mesh = model.build_isosurface(ext, res, 0.0, finish="close_positive", cluster="none", return_stats=True, **quiet)
    CR.check_closed(mesh.vertices, mesh.facets)
    assert mesh.stats["closure"]["open_edges"][0] > 0 and abs(R.enclosed_volume(mesh.vertices, mesh.facets) - want) <= 4 * np.pi * 1.8 ** 2 * res
    expr = rmt.build_isosurface(None, ext, res, 0.0, rmt.field(model), finish="close_positive", cluster_method=rmt.ClusterMethod.None_, **quiet)
    CR.check_closed(expr.vertices, expr.facets)
    assert np.array_equal(expr.facets, mesh.facets)

    def sphere(x):
        return np.linalg.norm(x - CC.CENTRE, axis=1) - CC.RADIUS

    call = rmt.build_isosurface(None, ext, res, 0.0, sphere, finish="close_negative", cluster_method=rmt.ClusterMethod.None_, **quiet)
    CR.check_closed(call.vertices, call.facets)
    box = float(np.prod(np.asarray(ext[3:]) - np.asarray(ext[:3])))
    assert abs(box - R.enclosed_volume(call.vertices, call.facets) - want) <= 4 * np.pi * 1.8 ** 2 * res
    with pytest.raises(NotImplementedError, match="close_positive"):
        rmt.build_isosurface(None, ext, res, 0.0, sphere, boundary_closure=rmt.BoundaryClosure.ClosePositive, **quiet)
    with pytest.raises(NotImplementedError, match="close_negative"):
        model.build_isosurface(ext, res, 0.0, RBF.BoundaryClosure.CloseNegative)
