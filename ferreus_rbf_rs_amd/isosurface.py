"""Isosurfaces on the regularised-marching-tetrahedra (RMT) sampling lattice, extracted on the device.

The mesh is ferreus_rmt's marching-tetrahedra output (`build_isosurface`, ferreus_rmt/src/isosurface.rs:489-), taken
over every sample point of the extraction domain instead of the sample points a seeded wavefront reaches (DESIGN.md
"Isosurfaces on the RMT lattice").  `finish="raw"` (the default) is that mesh as it is, before `clip_mesh_to_aabb` and
`clean_mesh`: it reaches two lattice cells past the extents.  `finish="clipped"` runs both on the device before the
download (isosurface.rs:1009-1021): the reference's finished mesh for `BoundaryClosure::None`;
`finish="close_positive"` / `"close_negative"` then close that mesh on the six faces of the extents (its
`BoundaryClosure::ClosePositive` / `CloseNegative`, boundary_closure.rs; see below).  Vertex gradients are not
implemented.  `cluster="none"` (the
default) is its `ClusterMethod::None`, one vertex per crossed lattice edge; `cluster="average"` its
`ClusterMethod::Average`: the intersections near a sample point are merged into their mean where the topology tests
allow it (topology.rs:232-314), and clusters that give a mesh edge more than 2 faces are split again
(isosurface.rs:798-930); the reference's later self-intersection rollback (isosurface.rs:932-1007) is run with
`self_intersections="rollback"` and left out with `"ignore"` (the default).  `cluster="curvature"` is its
`ClusterMethod::CurvatureWeighted`, the method its interpolator always uses (rbf.rs:1054-1064): the same clusters and
facets, every cluster placed at the mean of its intersections weighted by the curvature estimate of their lattice edges.

* lattice (lattice.rs:55-96): spacing [r/2, r*sqrt2/2, r/sqrt2], max_ijk = ceil((hi - lo) / spacing), max_ijk[0] += 1,
  world(ijk) = lo + ijk * spacing;
* keys: sample points (even i + j + k) with one of their 8 corners (get_edge_points::<8>, isosurface.rs:87-102) in
  [-2, max_ijk + 2] (extraction_ijk_inbounds, lattice.rs:117-128); E: the corners of the keys, where the field is
  evaluated; inside means f - isovalue < -1e-9 (isosurface.rs:286-289);
* one vertex per lattice edge of E with finite ends on opposite sides, placed from the end that holds it under the
  wavefront's t < 0.5 rule (isosurface.rs:588-610) with lerp_alpha (isosurface.rs:173-181);
* facets: march_tets (isosurface.rs:224-283) over the keys, in key order, tetrahedra 0..5, table rows in order;
* cluster="average": one vertex per cluster, ordered by sample point and lowest edge; triangles that two corners of
  share a vertex are dropped; `return_stats=True` adds the counts of `STATS` per mesh;
* cluster="curvature" (curvature_weighting.rs:48-276): the weight of a crossed edge comes from the field at the 14
  neighbours of the sample point that owns it (1 where one of them is off E, not evaluated or not finite, or the stencil
  is degenerate), computed on the device once per isovalue; every cluster, those of one edge too, is placed at the sum
  of w * p in ascending edge order times 1 / sum of w, or where that sum is 1e-12 or less as "average" places it.
  Facets, vertex order and the counts of `STATS` are those of "average"; the device's trigonometric functions differ
  from a host's in their last bits, so vertices agree with the numpy restatement to about 1e-13 of the resolution and
  not bit for bit.  `return_stats=True` then holds the counts of `CURVATURE_STATS` under "curvature";
* self_intersections="rollback", with cluster="average" or "curvature", after the two passes above and before the clip, one round: the
  triangles on true self-intersections (mesh_intersections.rs:125-208; `triangle_pair` is the predicate) among the
  facets with every corner inside the extents, found on the device through a uniform grid over their bounding boxes;
  their vertices that are clusters of several lattice edges; the sample points that own those go back to one vertex
  per edge and the mesh is marched again.  Nothing found: the mesh is bit for bit the one of "ignore".  With
  cluster="none" nothing is done.  `return_stats=True` then holds the counts of `INTERSECTION_STATS` under
  "self_intersections";
* finish="clipped" (aabb_clipping.rs:55-105, mesh_cleanup.rs:32-96), with eps = 1e-10 * max(|hi - lo|, 1): every facet
  clipped against the six planes of the extents in turn and fanned; vertices within eps welded, the lowest-index
  vertex of a group its representative; collapsed, zero-area (|ab x ac|^2 <= eps^4), repeated and lone facets dropped;
  vertices renumbered in order of first use.  `return_stats=True` then also holds the counts of `FINISH_STATS`;
* finish="close_positive" / "close_negative" (DESIGN.md "Boundary closure"): the clipped mesh first (reversed for
  "close_negative"), then per face of the extents (XMin, XMax, YMin, YMax, ZMin, ZMax) the cap facets, wound outward: the
  kept whole cells of a grid of `resolution` (two triangles each, made on the device) and the triangles of the band of
  cut cells along the open edges (triangulated on the host with exact orientation tests).  "close_positive" keeps the
  part of the faces where the field outside the extents counts as above the isovalue, "close_negative" the rest.  New
  vertices follow the mesh's in order of first use.  A mesh without open edges is returned as it is; an open edge off
  the faces is refused.  `return_stats=True` then holds the counts of `CLOSURE_STATS` under "closure".  `close_mesh`
  runs the closure alone on a caller's clipped mesh.

`follow="dense"` (the default) evaluates the field at every node of E.  `follow="surface"` follows the surface from seed
points as the reference does (seed_projection.rs:29-130, isosurface.rs:551-697; DESIGN.md "Following the surface"): the
box of E is cut into bricks of B x B x B nodes (B = 8; the environment variable BBFMM_ISO_BRICK takes 4, 8 or 16 and is
read per call); `seeds` ((n, 3) world points; None with a tree: its source points) are clamped to the extents, kept one
per lattice cell and, with a tree, moved onto the level set by at most 30 Newton steps (gradients from the leaf pass;
BBFMM_ISO_SEED_GRADIENTS=differences takes the reference's central differences instead); the bricks that hold the 8
corners of their cells are evaluated, and every lattice edge with both ends known and on opposite sides sends the wavefront into every brick
within (4, 2, 2) nodes of its ends, until nothing new is reached.  The mesh is the dense extraction (every option
above) of the field that is NaN outside the bricks visited for that isovalue: every component that passes through a
seed's cell is complete and bit for bit the dense one on the same values, a component no seed reaches is absent,
no seeds give an empty mesh.  `return_stats=True` then holds the counts of `FOLLOW_STATS`, the host times of the three
stages, the brick side and the (nbz, nby, nbx) array of visited bricks under "follow".  Memory stays proportional to the box.

Lattice fields are arrays of shape (nk, nj, ni) over the bounding box of E (`lattice_info(...)["shape"]`, entry
[0, 0, 0] at ijk `lattice_info(...)["lo"]`); entries off E are ignored, and NaN in returned fields.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L


def _ext(extents):
    e = np.ascontiguousarray(np.asarray(extents, dtype=np.float64).reshape(-1))
    if e.shape != (6,):
        raise ValueError("extents must hold 6 values: min x, min y, min z, max x, max y, max z")
    return e


def _isovalues(isovalues):
    v = np.ascontiguousarray(np.atleast_1d(np.asarray(isovalues, dtype=np.float64)).reshape(-1))
    if v.size == 0:
        raise ValueError("at least one isovalue is needed")
    return v


def _field_terms(drift):
    """The rbf.FieldTerms given as `drift` (polynomial of degree -1 .. 2 and / or a global trend), else None."""
    from .rbf import FieldTerms
    if not isinstance(drift, FieldTerms):
        return None
    if drift.d != 3 or drift.k != 1:
        raise ValueError("the field terms of an isosurface need d = 3 and one column")
    return drift


def _drift(drift):
    """None, [a, b0, b1, b2] or (a, [b0, b1, b2]): the affine drift a + b . x."""
    if drift is None:
        return None
    if len(drift) == 2 and np.ndim(drift[1]) == 1:
        d = np.concatenate([[float(drift[0])], np.asarray(drift[1], dtype=np.float64).reshape(-1)])
    else:
        d = np.asarray(drift, dtype=np.float64).reshape(-1)
    if d.shape != (4,):
        raise ValueError("drift must be [a, b0, b1, b2] or (a, [b0, b1, b2])")
    return np.ascontiguousarray(d)


def affine_drift(coefficients, translation=None, scale=None):
    """The drift of a Constant ([c0]) or Linear ([c0, c1, c2, c3] for [1, x0, x1, x2]) polynomial evaluated on (x - translation) / scale,
    as the reference's interpolator evaluates its global trend (polynomials.rs:30-74), folded into (a, b)."""
    c = np.asarray(coefficients, dtype=np.float64).reshape(-1)
    if c.size == 1:
        return (float(c[0]), np.zeros(3))
    if c.size != 4:
        raise ValueError("only Constant (1) and Linear (4 coefficients) drift is supported")
    t = np.broadcast_to(np.asarray(0.0 if translation is None else translation, dtype=np.float64), (3,))
    s = np.broadcast_to(np.asarray(1.0 if scale is None else scale, dtype=np.float64), (3,))
    b = c[1:] / s
    return (float(c[0] - np.dot(b, t)), b)


def lattice_info(extents, resolution, tree=None) -> dict:
    """max_ijk (SampleLattice::new), the number of keys and of nodes of E, and the layout of lattice fields."""
    lib = L.load()
    info = np.zeros(11, dtype=np.int64)
    h = tree._h if tree is not None else None
    rc = lib.bbfmm_isosurface_lattice(h, _ext(extents).ctypes.data, float(resolution), info.ctypes.data)
    if rc != L.OK:
        raise ValueError(lib.bbfmm_last_error(h).decode() if h else "bad isosurface lattice arguments")
    return {"max_ijk": info[0:3].copy(), "n_keys": int(info[3]), "n_nodes": int(info[4]), "lo": info[5:8].copy(),
            "shape": (int(info[10]), int(info[9]), int(info[8]))}


def tables() -> dict:
    """The marching-tetrahedra tables the library holds (ferreus_rmt/src/constants.rs)."""
    lib = L.load()
    ed, rev = np.zeros(42, np.int32), np.zeros(14, np.int32)
    tets, pairs, mt = np.zeros(18, np.int32), np.zeros(12, np.int32), np.zeros(16 * 7, np.int32)
    rc = lib.bbfmm_isosurface_tables(ed.ctypes.data, rev.ctypes.data, tets.ctypes.data, pairs.ctypes.data, mt.ctypes.data)
    assert rc == L.OK
    mt = mt.reshape(16, 7)
    return {"EDGE_DELTAS": ed.reshape(14, 3).tolist(), "REVERSE_EDGE": rev.tolist(),
            "OWNED_TET_EDGES": tets.reshape(6, 3).tolist(), "TET_EDGE_PAIRS": pairs.reshape(6, 2).tolist(),
            "MT_TABLE": [mt[c, 1:1 + 3 * mt[c, 0]].reshape(-1, 3).tolist() for c in range(16)]}


CLUSTER_METHODS = {"none": 0, "average": 1, "curvature": 2}
# return_stats with cluster="curvature" (bbfmm_isosurface_curvature_stats)
CURVATURE_STATS = ("edges", "edge_fallbacks", "clusters", "cluster_fallbacks")
# return_stats: sample points per topology case, then the two rollback passes (bbfmm_isosurface_stats)
STATS = ("closed", "multi_hole", "flat_hole", "multi_surface", "simple", "incomplete")


FINISH = {"raw": 0, "clipped": 1}
# the boundary closure behind the clip and clean: further values of `finish`, and the modes of close_mesh
FINISH_CLOSE = {"close_positive": 2, "close_negative": 3}
# return_stats with finish="close_positive" / "close_negative", and close_mesh (bbfmm_isosurface_closure_stats); the
# per-face entries are lists of 6 (XMin, XMax, YMin, YMax, ZMin, ZMax)
CLOSURE_STATS = ("open_edges", "open_edges_off_box", "cut_cells", "whole_cells_kept", "regions", "band_points",
                 "band_triangles", "dropped", "constraint_flips", "lawson_flips", "vertices_added", "conflicts",
                 "band_host_us")
# return_stats with finish="clipped" (bbfmm_isosurface_finish_stats)
FINISH_STATS = ("facets_in", "straddling", "outside", "vertices_emitted", "welded", "weld_loose", "collapsed", "tiny",
                "duplicate", "lone")


SELF_INTERSECTIONS = {"ignore": 0, "rollback": 1}
# return_stats with self_intersections="rollback", and mesh_self_intersections (bbfmm_isosurface_intersection_stats)
INTERSECTION_STATS = ("inside_facets", "box_pairs", "moller_pairs", "true_pairs", "triangles", "cluster_vertices",
                      "rolled_back")
# triangle_pair: the test that decided
PAIR_STAGES = ("degenerate", "shared_two", "moller", "shared_crossing", "geometric_shared", "near_coplanar", "true")


def _self_intersections(mode):
    if mode not in SELF_INTERSECTIONS:
        raise ValueError(f"self_intersections must be one of {sorted(SELF_INTERSECTIONS)}, got {mode!r}")
    return SELF_INTERSECTIONS[mode]


def _finish(finish):
    if finish in FINISH_CLOSE:
        return FINISH_CLOSE[finish]
    if finish not in FINISH:
        raise ValueError(f"finish must be one of {sorted(FINISH) + sorted(FINISH_CLOSE)}, got {finish!r}")
    return FINISH[finish]


FOLLOW = {"dense": 0, "surface": 1}
# return_stats with follow="surface" (bbfmm_isosurface_follow_stats)
FOLLOW_STATS = ("seeds", "seed_cells", "newton_steps", "seed_bricks", "rounds", "bricks_visited", "nodes_evaluated", "nodes")


def _follow(follow):
    if follow not in FOLLOW:
        raise ValueError(f"follow must be one of {sorted(FOLLOW)}, got {follow!r}")
    return FOLLOW[follow]


def _seeds(seeds):
    """None, or the (n, 3) seed points as a column-major array (kept alive by the caller for the call)."""
    if seeds is None:
        return None
    s = np.asarray(seeds, dtype=np.float64)
    if s.size == 0:
        return np.zeros((1, 3), order="F")[:0]
    if s.ndim != 2 or s.shape[1] != 3:
        raise ValueError(f"seeds must have shape (n, 3), got {s.shape}")
    if not np.all(np.isfinite(s)):
        raise ValueError("seeds must be finite")
    return np.asfortranarray(s)


def _options(method, finish, batch_bytes, self_intersections=0, follow=0, seeds=None):
    o = L.IsosurfaceOptions(ctypes.sizeof(L.IsosurfaceOptions), method, finish, int(batch_bytes), self_intersections)
    o.follow = follow
    if seeds is not None:
        o.seeds = seeds.base.ctypes.data if len(seeds) == 0 else seeds.ctypes.data  # never null: an empty set of seeds is one
        o.n_seeds = len(seeds)
        o.seeds_ld = max(len(seeds), 1)
    return o


def _cluster(cluster):
    if cluster not in CLUSTER_METHODS:
        raise ValueError(f"cluster must be one of {sorted(CLUSTER_METHODS)}, got {cluster!r}")
    return CLUSTER_METHODS[cluster]


def cluster_tables() -> dict:
    """The clustering tables the library holds (ferreus_rmt/src/constants.rs)."""
    lib = L.load()
    nb, fh, all14 = np.zeros(14, np.int32), np.zeros(72, np.int32), ctypes.c_int32()
    rc = lib.bbfmm_isosurface_cluster_tables(nb.ctypes.data, fh.ctypes.data, ctypes.byref(all14))
    assert rc == L.OK
    return {"NEIGHBOUR_MASKS": nb.tolist(), "FLAT_HOLE_MASKS": fh.reshape(36, 2).tolist(), "ALL14_MASK": all14.value}


def curvature_tables() -> dict:
    """The curvature-weighting tables the library holds (ferreus_rmt/src/constants.rs, curvature_weighting.rs): the rows
    of the 7 owned edges, the angles written out as numbers."""
    lib = L.load()
    pairs, phis, c = np.zeros(42, np.int32), np.zeros(42, np.int32), np.zeros(5)
    rc = lib.bbfmm_isosurface_curvature_tables(pairs.ctypes.data, phis.ctypes.data, c.ctypes.data)
    assert rc == L.OK
    pairs, phis = pairs.reshape(7, 3, 2), phis.reshape(7, 3, 2)
    rows = [[p for p in range(3) if pairs[l, p, 0] >= 0] for l in range(7)]
    return {"NEIGHBOUR_EDGE_PLANE_PAIRS": [[pairs[l, p].tolist() for p in rows[l]] for l in range(7)],
            "NEIGHBOUR_EDGE_PLANE_PHIS": [[[float(c[q - 1]) for q in phis[l, p]] for p in rows[l]] for l in range(7)],
            "PHI_1": float(c[0]), "PHI_2": float(c[1]), "EPS": float(c[2]), "MAX_COT_THETA": float(c[3]),
            "MAX_CURVATURE_WEIGHT": float(c[4])}


def curvature_weight(values, owner_ijk, label, lo_world, spacing):
    """(weight, fallback) of one crossed edge by the function the device runs (host only; curvature_weight_for_edge,
    curvature_weighting.rs:48-234): the owned edge `label` (0..6) of the sample point owner_ijk on the lattice
    world(ijk) = lo_world + ijk * spacing.  values: f - isovalue at the owner, then at its 14 neighbours, NaN for a
    missing one.  fallback True: the reference gives None and the weight is 1."""
    lib = L.load()
    v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
    o = np.ascontiguousarray(np.asarray(owner_ijk, dtype=np.int64).reshape(-1))
    lo = np.ascontiguousarray(np.asarray(lo_world, dtype=np.float64).reshape(-1))
    sp = np.ascontiguousarray(np.asarray(spacing, dtype=np.float64).reshape(-1))
    if v.shape != (15,) or o.shape != (3,) or lo.shape != (3,) or sp.shape != (3,):
        raise ValueError("values must hold 15 numbers, owner_ijk, lo_world and spacing 3 each")
    w, back = ctypes.c_double(), ctypes.c_int32()
    rc = lib.bbfmm_isosurface_curvature_weight(v.ctypes.data, o.ctypes.data, int(label), lo.ctypes.data, sp.ctypes.data,
                                               ctypes.byref(w), ctypes.byref(back))
    if rc != L.OK:
        raise ValueError("label must be one of the 7 owned edges, 0..6")
    return w.value, bool(back.value)


def topology(near_mask, neighbour_values=None):
    """(case, cluster_of_edge[14]) of a 14-bit near mask by the function the device runs (test_topology,
    topology.rs:232-314): case 0 closed, 1 multi-hole, 2 flat-hole, 3 multi-surface, 4 simple; cluster_of_edge the lowest
    edge of each edge's cluster, -1 off the mask.  neighbour_values: f - isovalue at the 14 neighbours, None to leave out
    the flat-hole test."""
    lib = L.load()
    case, lab = ctypes.c_int32(), np.zeros(14, np.int32)
    v = None
    if neighbour_values is not None:
        v = np.ascontiguousarray(np.asarray(neighbour_values, dtype=np.float64).reshape(-1))
        if v.shape != (14,):
            raise ValueError("neighbour_values must hold 14 values")
    rc = lib.bbfmm_isosurface_topology(int(near_mask), v.ctypes.data if v is not None else None, ctypes.byref(case),
                                       lab.ctypes.data)
    if rc != L.OK:
        raise ValueError("near_mask must be a 14-bit mask")
    return case.value, lab


def _stats(lib, res, i):
    s = np.zeros(16, dtype=np.int64)
    lib.bbfmm_isosurface_stats(res, i, s.ctypes.data)
    out = {name: int(s[q]) for q, name in enumerate(STATS)}
    out.update(over_used_a=int(s[6]), split_a=int(s[7]), rolled_b=s[8:12].tolist(), over_used_b=s[12:16].tolist())
    return out


def _finish_stats(lib, res, i):
    s = np.zeros(len(FINISH_STATS), dtype=np.int64)
    lib.bbfmm_isosurface_finish_stats(res, i, s.ctypes.data)
    return {name: int(s[q]) for q, name in enumerate(FINISH_STATS)}


def _closure_stats(lib, res, i):
    s = np.zeros(32, dtype=np.int64)
    lib.bbfmm_isosurface_closure_stats(res, i, s.ctypes.data)
    out = dict(open_edges=s[0:6].tolist(), open_edges_off_box=int(s[6]), cut_cells=s[7:13].tolist(),
               whole_cells_kept=s[13:19].tolist())
    out.update({name: int(s[19 + q]) for q, name in enumerate(CLOSURE_STATS[4:])})
    return out


def _follow_stats(lib, res, i):
    s, ms = np.zeros(len(FOLLOW_STATS), dtype=np.int64), np.zeros(3)
    lib.bbfmm_isosurface_follow_stats(res, i, s.ctypes.data)
    lib.bbfmm_isosurface_follow_times(res, i, ms.ctypes.data)
    out = {name: int(s[q]) for q, name in enumerate(FOLLOW_STATS)}
    out.update(seed_ms=float(ms[0]), wavefront_ms=float(ms[1]), extract_ms=float(ms[2]))
    dims = np.zeros(4, dtype=np.int32)
    lib.bbfmm_isosurface_follow_bricks(res, i, dims.ctypes.data, None)
    bricks = np.zeros(int(dims[1]) * int(dims[2]) * int(dims[3]), dtype=np.uint8)
    if bricks.size:
        lib.bbfmm_isosurface_follow_bricks(res, i, dims.ctypes.data, bricks.ctypes.data)
    out.update(brick=int(dims[0]), visited=bricks.reshape(int(dims[3]), int(dims[2]), int(dims[1])).astype(bool))
    return out


def _intersection_stats(lib, res, i):
    s = np.zeros(8, dtype=np.int64)
    lib.bbfmm_isosurface_intersection_stats(res, i, s.ctypes.data)
    return {name: int(s[q]) for q, name in enumerate(INTERSECTION_STATS)}


def _curvature_stats(lib, res, i):
    s = np.zeros(len(CURVATURE_STATS), dtype=np.int64)
    lib.bbfmm_isosurface_curvature_stats(res, i, s.ctypes.data)
    return {name: int(s[q]) for q, name in enumerate(CURVATURE_STATS)}


def _meshes(lib, res, stats=False, finish=0, self_intersections=0, follow=0, method=0):
    out = []
    for i in range(lib.bbfmm_isosurface_count(res)):
        nv, nf = ctypes.c_int64(), ctypes.c_int64()
        lib.bbfmm_isosurface_size(res, i, ctypes.byref(nv), ctypes.byref(nf))
        v = np.empty((nv.value, 3), dtype=np.float64)
        f = np.empty((nf.value, 3), dtype=np.int64)
        lib.bbfmm_isosurface_copy(res, i, v.ctypes.data, f.ctypes.data)
        if stats:
            st = _stats(lib, res, i)
            if finish:
                st["finish"] = _finish_stats(lib, res, i)
            if finish >= FINISH_CLOSE["close_positive"]:
                st["closure"] = _closure_stats(lib, res, i)
            if self_intersections:
                st["self_intersections"] = _intersection_stats(lib, res, i)
            if follow:
                st["follow"] = _follow_stats(lib, res, i)
            if method == CLUSTER_METHODS["curvature"]:
                st["curvature"] = _curvature_stats(lib, res, i)
            out.append((v, f, st))
        else:
            out.append((v, f))
    return out


def _raise(rc, msg, leaf=True):
    from .fmm_tree import CallbackFailed, FmmError, PointOutsideTree
    if rc == L.CALLBACK_FAILED:
        raise CallbackFailed(msg)
    if rc == L.POINT_OUTSIDE_TREE:
        e = PointOutsideTree(-1, leaf)
        e.args = (msg,)
        raise e
    if rc == L.DEVICE_ERROR:
        raise RuntimeError(msg)
    raise FmmError(msg)


def build_isosurfaces(tree, extents, resolution, isovalues, *, drift=None, return_field=False, batch_bytes: int = 0,
                      cluster="none", return_stats=False, finish="raw", self_intersections="ignore", follow="dense",
                      seeds=None):
    """Meshes of the tree's field (set_local_coefficients first, one column) at each isovalue, one field evaluation
    for all of them; see FmmTree.build_isosurfaces."""
    lib = L.load()
    method, fin, isect = _cluster(cluster), _finish(finish), _self_intersections(self_intersections)
    fol, sd = _follow(follow), _seeds(seeds)
    terms = _field_terms(drift)
    cterms = terms._c() if terms is not None else None
    ext, iso, d = _ext(extents), _isovalues(isovalues), _drift(None if terms is not None else drift)
    field_t = None
    if return_field:
        import torch
        info = lattice_info(ext, resolution, tree)
        n = int(np.prod(info["shape"]))
        field_t = torch.full((n,), float("nan"), dtype=torch.float64, device=f"cuda:{tree.device()}")
        torch.cuda.synchronize(field_t.device)
    res = ctypes.c_void_p()
    if fin or isect or fol or cterms is not None:
        opts = _options(method, fin, batch_bytes, isect, fol, sd if fol else None)
        if cterms is not None:
            opts.terms = ctypes.addressof(cterms)
        rc = lib.bbfmm_build_isosurfaces_opts(tree._h, ext.ctypes.data, float(resolution), iso.ctypes.data, len(iso),
                                              d.ctypes.data if d is not None else None,
                                              field_t.data_ptr() if field_t is not None else None, ctypes.addressof(opts),
                                              ctypes.byref(res))
    else:
        rc = lib.bbfmm_build_isosurfaces_ex(tree._h, ext.ctypes.data, float(resolution), iso.ctypes.data, len(iso),
                                            d.ctypes.data if d is not None else None,
                                            field_t.data_ptr() if field_t is not None else None, int(batch_bytes), method,
                                            ctypes.byref(res))
    try:
        if rc != L.OK:
            _raise(rc, lib.bbfmm_last_error(tree._h).decode())
        meshes = _meshes(lib, res, return_stats, fin, isect, fol, method)
    finally:
        if res:
            lib.bbfmm_isosurface_destroy(res)
    if return_field:
        return meshes, field_t.cpu().numpy().reshape(info["shape"])
    return meshes


def isosurfaces_from_values(lattice_values, extents, resolution, isovalues, *, batch_bytes: int = 0, tree=None,
                            cluster="none", return_stats=False, finish="raw", self_intersections="ignore", follow="dense",
                            seeds=None):
    """Meshes of a caller's lattice field (shape lattice_info(extents, resolution)["shape"]) at each isovalue, on the
    current device (or the tree's).  cluster: "none", "average" or "curvature", finish: "raw", "clipped", "close_positive" or
    "close_negative" (then under "closure" the counts of CLOSURE_STATS), self_intersections:
    "ignore" or "rollback" (see the module); return_stats: (vertices, facets, stats) per mesh, stats the clustering
    counts (all 0 with "none"), with cluster="curvature" under "curvature" the counts of CURVATURE_STATS, with
    finish="clipped" under "finish" the counts of FINISH_STATS and with
    self_intersections="rollback" under "self_intersections" those of INTERSECTION_STATS.  follow="surface": only the
    values in the bricks the wavefront reaches from `seeds` ((n, 3), required, used as they are) are looked at."""
    lib = L.load()
    method, fin, isect = _cluster(cluster), _finish(finish), _self_intersections(self_intersections)
    fol, sd = _follow(follow), _seeds(seeds)
    if fol and sd is None:
        raise ValueError("follow='surface' of lattice values needs seeds")
    ext, iso = _ext(extents), _isovalues(isovalues)
    vals = np.ascontiguousarray(np.asarray(lattice_values, dtype=np.float64))
    info = lattice_info(ext, resolution, tree)
    if vals.size != int(np.prod(info["shape"])):
        raise ValueError(f"lattice_values must have shape {info['shape']}, got {vals.shape}")
    res = ctypes.c_void_p()
    h = tree._h if tree is not None else None
    if fin or isect or fol:
        opts = _options(method, fin, batch_bytes, isect, fol, sd if fol else None)
        rc = lib.bbfmm_isosurfaces_from_values_opts(h, vals.ctypes.data, ext.ctypes.data, float(resolution),
                                                    iso.ctypes.data, len(iso), ctypes.addressof(opts), ctypes.byref(res))
    else:
        rc = lib.bbfmm_isosurfaces_from_values_ex(h, vals.ctypes.data, ext.ctypes.data, float(resolution), iso.ctypes.data,
                                                  len(iso), int(batch_bytes), method, ctypes.byref(res))
    try:
        if rc != L.OK:
            _raise(rc, lib.bbfmm_isosurface_error(res).decode() if res else "isosurface extraction failed")
        return _meshes(lib, res, return_stats, fin, isect, fol, method)
    finally:
        if res:
            lib.bbfmm_isosurface_destroy(res)


def isosurface_from_values(lattice_values, extents, resolution, isovalue, *, batch_bytes: int = 0, tree=None,
                           cluster="none", return_stats=False, finish="raw", self_intersections="ignore", follow="dense",
                           seeds=None):
    """(vertices (n, 3) f64, facets (m, 3) int64) of a caller's lattice field at one isovalue, and its stats when
    return_stats."""
    return isosurfaces_from_values(lattice_values, extents, resolution, [isovalue], batch_bytes=batch_bytes, tree=tree,
                                   cluster=cluster, return_stats=return_stats, finish=finish,
                                   self_intersections=self_intersections, follow=follow, seeds=seeds)[0]


def clip_mesh(vertices, facets, extents, return_stats=False, *, tree=None):
    """finish="clipped" of a caller's own mesh on the current device (or the tree's): (vertices (n, 3) f64, facets
    (m, 3) int64) clipped to the extents and cleaned, and the counts of FINISH_STATS when return_stats.  A mesh wholly
    outside the extents gives (0, 3) arrays."""
    lib = L.load()
    ext = _ext(extents)
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float64).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(facets, dtype=np.int64).reshape(-1, 3))
    res = ctypes.c_void_p()
    h = tree._h if tree is not None else None
    rc = lib.bbfmm_isosurface_finish_mesh(h, v.ctypes.data, len(v), f.ctypes.data, len(f), ext.ctypes.data,
                                          ctypes.byref(res))
    try:
        if rc != L.OK:
            _raise(rc, lib.bbfmm_isosurface_error(res).decode() if res else "isosurface finish failed")
        vo, fo = _meshes(lib, res)[0]
        return (vo, fo, _finish_stats(lib, res, 0)) if return_stats else (vo, fo)
    finally:
        if res:
            lib.bbfmm_isosurface_destroy(res)


def close_mesh(vertices, facets, extents, resolution, mode, return_stats=False, *, tree=None):
    """The boundary closure alone of a caller's own clipped and cleaned mesh (clip_mesh gives one) on the current device
    (or the tree's): (vertices, facets) closed on the faces of the extents with a cap grid of `resolution`; mode:
    "close_positive" or "close_negative" (see the module); and the counts of CLOSURE_STATS when return_stats.  A mesh
    without facets or without open edges is returned as it is; one with an open edge off the faces is refused."""
    lib = L.load()
    if mode not in FINISH_CLOSE:
        raise ValueError(f"mode must be one of {sorted(FINISH_CLOSE)}, got {mode!r}")
    ext = _ext(extents)
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float64).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(facets, dtype=np.int64).reshape(-1, 3))
    res = ctypes.c_void_p()
    h = tree._h if tree is not None else None
    rc = lib.bbfmm_isosurface_close_mesh(h, v.ctypes.data, len(v), f.ctypes.data, len(f), ext.ctypes.data,
                                         float(resolution), FINISH_CLOSE[mode], ctypes.byref(res))
    try:
        if rc != L.OK:
            _raise(rc, lib.bbfmm_isosurface_error(res).decode() if res else "isosurface closure failed")
        vo, fo = _meshes(lib, res)[0]
        return (vo, fo, _closure_stats(lib, res, 0)) if return_stats else (vo, fo)
    finally:
        if res:
            lib.bbfmm_isosurface_destroy(res)


def orient2d(a, b, c):
    """The exact signs (-1, 0, 1; 1: counter-clockwise) of the orientation determinants of the triples a, b, c ((n, 2)
    each) by the predicate the closure's triangulator runs (host only)."""
    lib = L.load()
    abc = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in (a, b, c)], axis=1))
    out = np.zeros(len(abc), dtype=np.int32)
    rc = lib.bbfmm_debug_orient2d(abc.ctypes.data, len(abc), out.ctypes.data)
    if rc != L.OK:
        raise ValueError("orient2d: bad arguments")
    return out


def triangulate_band(gu, gv, points, edges, cut, resolution, eps):
    """The closure's band triangulator on one face (host only): gu, gv the grid coordinates, points (n, 2) the mesh
    vertices on the face, edges (m, 2) the open edges as point indices, cut the ascending ids v * nu + u of the cut
    cells.  Returns (band points (p, 2), ids (p,): the index of a mesh point or -1 - (v index * (nu + 1) + u index) of a
    grid point, triangles (t, 3) counter-clockwise, counts); raises FmmError where the constraints cannot be met."""
    lib = L.load()
    gu, gv = (np.ascontiguousarray(np.asarray(g, dtype=np.float64).reshape(-1)) for g in (gu, gv))
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 2))
    ed = np.ascontiguousarray(np.asarray(edges, dtype=np.int64).reshape(-1, 2))
    ct = np.ascontiguousarray(np.asarray(cut, dtype=np.int32).reshape(-1))
    cap_p = len(pts) + 4 * len(ct) + 4
    cap_t = 2 * cap_p + 4
    po, ido, to = np.zeros((cap_p, 2)), np.zeros(cap_p, np.int64), np.zeros((cap_t, 3), np.int64)
    counts, err = np.zeros(8, np.int64), ctypes.create_string_buffer(512)
    rc = lib.bbfmm_debug_closure_triangulate(len(gu) - 1, len(gv) - 1, gu.ctypes.data, gv.ctypes.data, pts.ctypes.data, len(pts),
                                             ed.ctypes.data, len(ed), ct.ctypes.data, len(ct), 1e-9 * float(resolution),
                                             max(float(eps), 1e-12), cap_p, po.ctypes.data, ido.ctypes.data, cap_t,
                                             to.ctypes.data, counts.ctypes.data, err, len(err))
    if rc != L.OK:
        _raise(rc, err.value.decode())
    n, t = int(counts[0]), int(counts[1])
    return po[:n].copy(), ido[:n].copy(), to[:t].copy(), dict(points=n, triangles=t, dropped=int(counts[2]),
                                                               constraint_flips=int(counts[3]), lawson_flips=int(counts[4]))


def clip_triangle(triangle, extents):
    """(points (n, 3), corners (n,)) of one triangle clipped to the extents by the function the device runs (host only):
    n = 0 when it is dropped; corners: the corner a point is a kept copy of, -1 for a point made on a plane."""
    lib = L.load()
    tri = np.ascontiguousarray(np.asarray(triangle, dtype=np.float64).reshape(-1))
    if tri.shape != (9,):
        raise ValueError("triangle must hold 3 points")
    pts, corner, n = np.zeros((12, 3)), np.zeros(12, np.int32), ctypes.c_int32()
    rc = lib.bbfmm_isosurface_clip_triangle(tri.ctypes.data, _ext(extents).ctypes.data, pts.ctypes.data, corner.ctypes.data,
                                            ctypes.byref(n))
    if rc != L.OK:
        raise ValueError("extents must be finite with min <= max")
    return pts[:n.value].copy(), corner[:n.value].copy()


def mesh_self_intersections(vertices, facets, extents=None, return_stats=False, *, tree=None):
    """The ids (ascending, int64) of the triangles of a caller's own mesh on true self-intersections, found on the
    current device (or the tree's): the reference's get_intersecting_triangles (mesh_intersections.rs:163-208).
    extents: only the facets with every corner inside them take part (the filter of the rollback), None: all.
    return_stats: also the counts "inside_facets", "box_pairs", "moller_pairs", "true_pairs" and "triangles" of
    INTERSECTION_STATS.  A mesh whose largest facet makes the grid search quadratic is refused (FmmError)."""
    lib = L.load()
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float64).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(facets, dtype=np.int64).reshape(-1, 3))
    ext = _ext(extents) if extents is not None else None
    res = ctypes.c_void_p()
    h = tree._h if tree is not None else None
    rc = lib.bbfmm_isosurface_self_intersections(h, v.ctypes.data, len(v), f.ctypes.data, len(f),
                                                 ext.ctypes.data if ext is not None else None, ctypes.byref(res))
    try:
        if rc != L.OK:
            _raise(rc, lib.bbfmm_isosurface_error(res).decode() if res else "isosurface self-intersection search failed")
        n = ctypes.c_int64()
        lib.bbfmm_isosurface_intersection_ids(res, 0, ctypes.byref(n), None)
        ids = np.empty(n.value, dtype=np.int64)
        lib.bbfmm_isosurface_intersection_ids(res, 0, None, ids.ctypes.data)
        if not return_stats:
            return ids
        st = _intersection_stats(lib, res, 0)
        return ids, {k: st[k] for k in INTERSECTION_STATS[:5]}
    finally:
        if res:
            lib.bbfmm_isosurface_destroy(res)


def triangle_pair(tri_a, ids_a, tri_b, ids_b):
    """(result, stage) of the pair predicate the device runs (host only; is_true_self_intersection,
    mesh_intersections.rs:125-159): result True for a true self-intersection, stage the index into PAIR_STAGES of the
    test that decided.  tri_a, tri_b: 3 points each, ids_a, ids_b: their vertex ids; a is the facet with the lower index.
    The Moeller test inside compares unnormalised normals with 1e-6, so the answer depends on the scale of the
    triangles, as the reference's does."""
    lib = L.load()
    ta = np.ascontiguousarray(np.asarray(tri_a, dtype=np.float64).reshape(-1))
    tb = np.ascontiguousarray(np.asarray(tri_b, dtype=np.float64).reshape(-1))
    ia = np.ascontiguousarray(np.asarray(ids_a, dtype=np.int64).reshape(-1))
    ib = np.ascontiguousarray(np.asarray(ids_b, dtype=np.int64).reshape(-1))
    if ta.shape != (9,) or tb.shape != (9,) or ia.shape != (3,) or ib.shape != (3,):
        raise ValueError("a triangle holds 3 points and 3 vertex ids")
    result, stage = ctypes.c_int32(), ctypes.c_int32()
    rc = lib.bbfmm_isosurface_triangle_pair(ta.ctypes.data, ia.ctypes.data, tb.ctypes.data, ib.ctypes.data,
                                            ctypes.byref(result), ctypes.byref(stage))
    assert rc == L.OK
    return bool(result.value), stage.value
