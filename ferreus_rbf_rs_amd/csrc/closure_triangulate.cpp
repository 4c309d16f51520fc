// The band triangulator of the boundary closure (closure_triangulate.hpp; DESIGN.md "Boundary closure").  All band
// points go into an incremental triangulation of the face's rectangle (walk, split, Lawson legalisation), the
// constraints are recovered by flips, the triangles off the cut cells are dropped and the rest is relaxed by Lawson flips
// on unconstrained edges.  Every orientation decision is the exact sign; the in-circle test is floating point with a
// certified margin, so that a tie (grid points are cocircular by construction) never flips.
#include "closure_triangulate.hpp"

#include <algorithm>
#include <cmath>
#include <unordered_map>

namespace bbfmm {
namespace iso {
namespace closure {

namespace {

inline void two_sum(double a, double b, double *s, double *e) {
    *s = a + b;
    const double bb = *s - a;
    *e = (a - (*s - bb)) + (b - bb);
}

inline void two_prod(double a, double b, double *p, double *e) {
    *p = a * b;
    *e = std::fma(a, b, -*p);
}

// e (n components, nonoverlapping, increasing magnitude) + b
inline int grow(double *e, int n, double b) {
    double q = b;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        double s, h;
        two_sum(q, e[i], &s, &h);
        if (h != 0.0) e[m++] = h;
        q = s;
    }
    if (q != 0.0 || m == 0) e[m++] = q;
    return m;
}

// d strictly inside the circle of the counter-clockwise a, b, c, beyond the rounding of the determinant (the static
// bound of the adaptive predicates: (10 + 96 u) u times the permanent)
inline bool in_circle_certain(const double *a, const double *b, const double *c, const double *d) {
    const double adx = a[0] - d[0], ady = a[1] - d[1], bdx = b[0] - d[0], bdy = b[1] - d[1], cdx = c[0] - d[0], cdy = c[1] - d[1];
    const double bdxcdy = bdx * cdy, cdxbdy = cdx * bdy, alift = adx * adx + ady * ady;
    const double cdxady = cdx * ady, adxcdy = adx * cdy, blift = bdx * bdx + bdy * bdy;
    const double adxbdy = adx * bdy, bdxady = bdx * ady, clift = cdx * cdx + cdy * cdy;
    const double det = alift * (bdxcdy - cdxbdy) + blift * (cdxady - adxcdy) + clift * (adxbdy - bdxady);
    const double permanent = (std::fabs(bdxcdy) + std::fabs(cdxbdy)) * alift + (std::fabs(cdxady) + std::fabs(adxcdy)) * blift +
                             (std::fabs(adxbdy) + std::fabs(bdxady)) * clift;
    const double u = 1.1102230246251565e-16;
    return det > (10.0 + 96.0 * u) * u * permanent * 4.0; // (4: the differences above are rounded too)
}

struct Mesh2 {
    std::vector<double> x, y;
    std::vector<int> V, N;       // 3 per triangle: vertices (counter-clockwise), neighbour across edge k = (V[k], V[k + 1])
    std::vector<uint8_t> C, dead; // constrained edges; dropped triangles
    std::vector<int> vt;          // a triangle of every vertex

    int ntri() const { return static_cast<int>(dead.size()); }
    int orient(int a, int b, int c) const {
        const double pa[2] = {x[a], y[a]}, pb[2] = {x[b], y[b]}, pc[2] = {x[c], y[c]};
        return orient2d_sign(pa, pb, pc);
    }
    int orient_p(int a, int b, const double *p) const {
        const double pa[2] = {x[a], y[a]}, pb[2] = {x[b], y[b]};
        return orient2d_sign(pa, pb, p);
    }
    int new_tri() {
        V.resize(V.size() + 3, -1);
        N.resize(N.size() + 3, -1);
        C.resize(C.size() + 3, 0);
        dead.push_back(0);
        return ntri() - 1;
    }
    void set_tri(int t, int a, int b, int c, int n0, int n1, int n2, int c0, int c1, int c2) {
        V[3 * t] = a, V[3 * t + 1] = b, V[3 * t + 2] = c;
        N[3 * t] = n0, N[3 * t + 1] = n1, N[3 * t + 2] = n2;
        C[3 * t] = uint8_t(c0), C[3 * t + 1] = uint8_t(c1), C[3 * t + 2] = uint8_t(c2);
        vt[a] = vt[b] = vt[c] = t;
    }
    int index_of(int t, int v) const { return V[3 * t] == v ? 0 : (V[3 * t + 1] == v ? 1 : (V[3 * t + 2] == v ? 2 : -1)); }
    // the neighbour o sees the triangle across its edge starting at `from` as t
    void back(int o, int from, int t) {
        if (o < 0) return;
        const int k = index_of(o, from);
        if (k >= 0) N[3 * o + k] = t;
    }
    bool convex(int a, int b, int c, int d) const { // the quadrilateral a, d, b, c around the diagonal a-b, strictly
        return orient(a, d, c) > 0 && orient(d, b, c) > 0;
    }
    // edge k of t replaced by the other diagonal; t becomes (a, d, c), its neighbour (d, b, c)
    void flip(int t, int k, int *t_out, int *u_out) {
        const int a = V[3 * t + k], b = V[3 * t + (k + 1) % 3], c = V[3 * t + (k + 2) % 3];
        const int u = N[3 * t + k], ku = index_of(u, b), d = V[3 * u + (ku + 2) % 3];
        const int n_bc = N[3 * t + (k + 1) % 3], n_ca = N[3 * t + (k + 2) % 3], n_ad = N[3 * u + (ku + 1) % 3], n_db = N[3 * u + (ku + 2) % 3];
        const int c_bc = C[3 * t + (k + 1) % 3], c_ca = C[3 * t + (k + 2) % 3], c_ad = C[3 * u + (ku + 1) % 3], c_db = C[3 * u + (ku + 2) % 3];
        set_tri(t, a, d, c, n_ad, u, n_ca, c_ad, 0, c_ca);
        set_tri(u, d, b, c, n_db, n_bc, t, c_db, c_bc, 0);
        back(n_ad, d, t);
        back(n_bc, c, u);
        *t_out = t;
        *u_out = u;
    }
    bool delaunay_wants(int t, int k) const { // flip edge k of t: certain in-circle and a strictly convex quadrilateral
        const int u = N[3 * t + k];
        if (u < 0 || C[3 * t + k]) return false;
        const int a = V[3 * t + k], b = V[3 * t + (k + 1) % 3], c = V[3 * t + (k + 2) % 3];
        const int d = V[3 * u + (index_of(u, b) + 2) % 3];
        const double pa[2] = {x[a], y[a]}, pb[2] = {x[b], y[b]}, pc[2] = {x[c], y[c]}, pd[2] = {x[d], y[d]};
        return in_circle_certain(pa, pb, pc, pd) && convex(a, b, c, d);
    }
    void legalize(std::vector<std::pair<int, int>> *stack) { // (triangle, its vertex the new point): the edge opposite it
        while (!stack->empty()) {
            const int t = stack->back().first, p = stack->back().second;
            stack->pop_back();
            const int kp = index_of(t, p);
            if (kp < 0) continue;
            const int k = (kp + 1) % 3;
            if (!delaunay_wants(t, k)) continue;
            int t2, u2;
            flip(t, k, &t2, &u2);
            stack->push_back({t2, p});
            stack->push_back({u2, p});
        }
    }
    // the triangle holding p (closed), from `start`: a visibility walk, with a scan of all triangles behind it
    int locate(const double *p, int start, int o[3]) const {
        int t = start;
        const int cap = 64 + 4 * static_cast<int>(std::sqrt(static_cast<double>(ntri())));
        for (int step = 0; step < cap && t >= 0; ++step) {
            int k = 0;
            for (; k < 3; ++k) {
                o[k] = orient_p(V[3 * t + k], V[3 * t + (k + 1) % 3], p);
                if (o[k] < 0) break;
            }
            if (k == 3) return t;
            t = N[3 * t + k];
        }
        for (t = 0; t < ntri(); ++t) {
            int k = 0;
            for (; k < 3; ++k) {
                o[k] = orient_p(V[3 * t + k], V[3 * t + (k + 1) % 3], p);
                if (o[k] < 0) break;
            }
            if (k == 3) return t;
        }
        return -1;
    }
    // the triangles around p, each with the index of p in it
    template <class F> void around(int p, F &&f) const {
        const int t0 = vt[p];
        int t = t0;
        do {
            const int k = index_of(t, p);
            if (f(t, k)) return;
            t = N[3 * t + (k + 2) % 3];
        } while (t >= 0 && t != t0);
        if (t == t0) return;
        t = N[3 * t0 + index_of(t0, p)];
        while (t >= 0) {
            const int k = index_of(t, p);
            if (f(t, k)) return;
            t = N[3 * t + k];
        }
    }
    // the directed edge p -> q as edge k of triangle t, or its twin q -> p (then *twin); false: no such edge
    bool find_edge(int p, int q, int *t_out, int *k_out) const {
        bool found = false;
        around(p, [&](int t, int k) {
            if (V[3 * t + (k + 1) % 3] == q) {
                *t_out = t, *k_out = k, found = true;
            } else if (V[3 * t + (k + 2) % 3] == q) {
                *t_out = t, *k_out = (k + 2) % 3, found = true;
            }
            return found;
        });
        return found;
    }
    void constrain(int t, int k) {
        C[3 * t + k] = 1;
        const int u = N[3 * t + k];
        if (u >= 0) C[3 * u + index_of(u, V[3 * t + (k + 1) % 3])] = 1;
    }
};

int lower_cell(const double *g, int n, double v) { // the last i in [0, n) with g[i] <= v (0 below the grid)
    int lo = 0, hi = n;                            // g[lo] <= v < g[hi] where both hold
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

} // namespace

int orient2d_sign(const double *a, const double *b, const double *c) {
    const double l = (b[0] - a[0]) * (c[1] - a[1]), r = (b[1] - a[1]) * (c[0] - a[0]);
    const double det = l - r, sum = std::fabs(l) + std::fabs(r);
    if (std::fabs(det) > 3.3306690738754716e-16 * sum * 2.0 && std::isfinite(det)) return det > 0 ? 1 : -1;
    // a0 b1 - a0 c1 + b0 c1 - b0 a1 + c0 a1 - c0 b1, every product exact as a pair
    const double f[6][2] = {{a[0], b[1]}, {-a[0], c[1]}, {b[0], c[1]}, {-b[0], a[1]}, {c[0], a[1]}, {-c[0], b[1]}};
    double e[16];
    int n = 0;
    for (int i = 0; i < 6; ++i) {
        double p, q;
        two_prod(f[i][0], f[i][1], &p, &q);
        n = grow(e, n, q);
        n = grow(e, n, p);
    }
    const double top = e[n - 1];
    return top > 0 ? 1 : (top < 0 ? -1 : 0);
}

bool point_on_segment2(const double *p, const double *a, const double *b, double eps) {
    const double ab[2] = {b[0] - a[0], b[1] - a[1]}, ap[2] = {p[0] - a[0], p[1] - a[1]}, bp[2] = {p[0] - b[0], p[1] - b[1]};
    const double cross = ab[0] * ap[1] - ab[1] * ap[0];
    if (std::fabs(cross) > eps * std::max(std::hypot(ab[0], ab[1]), 1.0)) return false;
    return ap[0] * bp[0] + ap[1] * bp[1] <= eps * eps;
}

bool triangulate_band(Band *B, std::string *err) {
    B->xy.clear();
    B->id.clear();
    B->tri.clear();
    B->dropped = B->constraint_flips = B->lawson_flips = 0;
    if (B->n_cut == 0) {
        if (B->n_edges > 0) {
            *err = "closure: open edges on a face without cut cells";
            return false;
        }
        return true;
    }
    const int nu = B->nu, nv = B->nv;
    const int64_t gw = int64_t(nu) + 1;
    auto is_cut = [&](int i, int j) {
        if (i < 0 || j < 0 || i >= nu || j >= nv) return false;
        const int64_t c = int64_t(j) * nu + i;
        const int32_t *e = B->cut + B->n_cut, *it = std::lower_bound(B->cut, e, c, [](int32_t a, int64_t b) { return int64_t(a) < b; });
        return it != e && *it == c;
    };
    for (int64_t q = 0; q < B->n_cut; ++q)
        if (B->cut[q] < 0 || int64_t(B->cut[q]) >= int64_t(nu) * nv || (q && B->cut[q] <= B->cut[q - 1])) {
            *err = "closure: the cut cells must be ascending ids of the grid";
            return false;
        }
    Mesh2 M;
    const int np = static_cast<int>(B->n_points);
    // ---- the band points: the mesh points, then the corners of the cut cells
    struct KeyHash {
        size_t operator()(const std::pair<int64_t, int64_t> &k) const {
            return std::hash<int64_t>()(k.first * 0x9e3779b97f4a7c15ll ^ (k.second + 0x7f4a7c15ll) * 0xbf58476d1ce4e5b9ll);
        }
    };
    std::unordered_map<std::pair<int64_t, int64_t>, int, KeyHash> by_key;
    auto key_of = [&](double u, double v) {
        return std::make_pair(static_cast<int64_t>(std::round(u / B->key_cell)), static_cast<int64_t>(std::round(v / B->key_cell)));
    };
    for (int p = 0; p < np; ++p) {
        const double u = B->points[2 * p], v = B->points[2 * p + 1];
        if (!(u >= B->gu[0] && u <= B->gu[nu] && v >= B->gv[0] && v <= B->gv[nv])) {
            *err = "closure: mesh vertex " + std::to_string(p) + " of the face lies off it";
            return false;
        }
        M.x.push_back(u);
        M.y.push_back(v);
        B->id.push_back(p);
        if (!by_key.emplace(key_of(u, v), p).second) {
            *err = "closure: two mesh vertices of a face share a weld key";
            return false;
        }
    }
    for (int64_t e = 0; e < B->n_edges; ++e)
        for (int s = 0; s < 2; ++s)
            if (B->edges[2 * e + s] < 0 || B->edges[2 * e + s] >= np) {
                *err = "closure: open edge " + std::to_string(e) + " names a point off the list";
                return false;
            }
    // the open edges by the cells their widened boxes meet
    std::unordered_map<int64_t, std::vector<int64_t>> cell_edges;
    for (int64_t e = 0; e < B->n_edges; ++e) {
        const double *a = B->points + 2 * B->edges[2 * e], *b = B->points + 2 * B->edges[2 * e + 1];
        const double ulo = std::min(a[0], b[0]) - B->tol, uhi = std::max(a[0], b[0]) + B->tol;
        const double vlo = std::min(a[1], b[1]) - B->tol, vhi = std::max(a[1], b[1]) + B->tol;
        int i0 = lower_cell(B->gu, nu, ulo), i1 = lower_cell(B->gu, nu, uhi), j0 = lower_cell(B->gv, nv, vlo), j1 = lower_cell(B->gv, nv, vhi);
        if (i0 > 0 && B->gu[i0] >= ulo) --i0; // closed cells: the one ending at ulo meets the box too
        if (j0 > 0 && B->gv[j0] >= vlo) --j0;
        for (int j = j0; j <= j1; ++j)
            for (int i = i0; i <= i1; ++i) cell_edges[int64_t(j) * nu + i].push_back(e);
    }
    std::unordered_map<int64_t, int> grid_pt; // grid point -> band point, -2: omitted (on an open edge)
    auto grid_point = [&](int gi, int gj) -> int {
        const int64_t g = int64_t(gj) * gw + gi;
        auto it = grid_pt.find(g);
        if (it != grid_pt.end()) return it->second;
        const double p[2] = {B->gu[gi], B->gv[gj]};
        int r;
        auto km = by_key.find(key_of(p[0], p[1]));
        if (km != by_key.end()) {
            r = km->second;
        } else {
            bool on = false;
            for (int dj = -1; dj <= 0 && !on; ++dj)
                for (int di = -1; di <= 0 && !on; ++di) {
                    if (gi + di < 0 || gj + dj < 0 || gi + di >= nu || gj + dj >= nv) continue;
                    auto ce = cell_edges.find(int64_t(gj + dj) * nu + gi + di);
                    if (ce == cell_edges.end()) continue;
                    for (int64_t e : ce->second)
                        if (point_on_segment2(p, B->points + 2 * B->edges[2 * e], B->points + 2 * B->edges[2 * e + 1], B->tol)) {
                            on = true;
                            break;
                        }
                }
            if (on) {
                r = -2;
            } else {
                r = static_cast<int>(M.x.size());
                M.x.push_back(p[0]);
                M.y.push_back(p[1]);
                B->id.push_back(-1 - g);
            }
        }
        grid_pt.emplace(g, r);
        return r;
    };
    for (int64_t q = 0; q < B->n_cut; ++q) {
        const int i = B->cut[q] % nu, j = B->cut[q] / nu;
        grid_point(i, j), grid_point(i + 1, j), grid_point(i, j + 1), grid_point(i + 1, j + 1);
    }
    const int n_band = static_cast<int>(M.x.size());
    // ---- the rectangle of the face: its corners are band points or auxiliary ones that no kept triangle may use
    int rect[4];
    const int rc[4][2] = {{0, 0}, {nu, 0}, {nu, nv}, {0, nv}};
    for (int q = 0; q < 4; ++q) {
        const double cu = B->gu[rc[q][0]], cv = B->gv[rc[q][1]];
        auto it = grid_pt.find(int64_t(rc[q][1]) * gw + rc[q][0]);
        int r = it != grid_pt.end() ? it->second : -1;
        if (r < 0) {
            auto km = by_key.find(key_of(cu, cv));
            if (km != by_key.end()) r = km->second;
        }
        if (r >= 0 && (M.x[r] != cu || M.y[r] != cv)) r = -1;
        if (r < 0) {
            r = static_cast<int>(M.x.size());
            M.x.push_back(cu);
            M.y.push_back(cv);
        }
        rect[q] = r;
    }
    if (M.orient(rect[0], rect[1], rect[2]) <= 0 || M.orient(rect[0], rect[2], rect[3]) <= 0) {
        *err = "closure: a face of the extents has no area";
        return false;
    }
    M.vt.assign(M.x.size(), -1);
    const int ta = M.new_tri(), tb = M.new_tri();
    M.set_tri(ta, rect[0], rect[1], rect[2], -1, -1, tb, 0, 0, 0);
    M.set_tri(tb, rect[0], rect[2], rect[3], ta, -1, -1, 0, 0, 0);
    // ---- insertion, in a snake through the cells so that the walk is short
    std::vector<std::pair<int64_t, int>> order;
    order.reserve(n_band);
    for (int p = 0; p < n_band; ++p) {
        if (p == rect[0] || p == rect[1] || p == rect[2] || p == rect[3]) continue;
        const int i = lower_cell(B->gu, nu, M.x[p]), j = lower_cell(B->gv, nv, M.y[p]);
        order.push_back({int64_t(j) * nu + ((j & 1) ? nu - 1 - i : i), p});
    }
    std::sort(order.begin(), order.end());
    std::vector<std::pair<int, int>> stack;
    int last = ta;
    for (const auto &op : order) {
        const int p = op.second;
        const double pp[2] = {M.x[p], M.y[p]};
        int o[3];
        const int t = M.locate(pp, last, o);
        if (t < 0) {
            *err = "closure: a band point lies outside its face";
            return false;
        }
        const int zeros = (o[0] == 0) + (o[1] == 0) + (o[2] == 0);
        if (zeros >= 2) {
            *err = "closure: two band points coincide";
            return false;
        }
        if (zeros == 0) {
            const int a = M.V[3 * t], b = M.V[3 * t + 1], c = M.V[3 * t + 2];
            const int n0 = M.N[3 * t], n1 = M.N[3 * t + 1], n2 = M.N[3 * t + 2];
            const int t1 = M.new_tri(), t2 = M.new_tri();
            M.set_tri(t, a, b, p, n0, t1, t2, 0, 0, 0);
            M.set_tri(t1, b, c, p, n1, t2, t, 0, 0, 0);
            M.set_tri(t2, c, a, p, n2, t, t1, 0, 0, 0);
            M.back(n1, c, t1);
            M.back(n2, a, t2);
            stack.push_back({t, p});
            stack.push_back({t1, p});
            stack.push_back({t2, p});
        } else {
            const int k = o[0] == 0 ? 0 : (o[1] == 0 ? 1 : 2);
            const int a = M.V[3 * t + k], b = M.V[3 * t + (k + 1) % 3], c = M.V[3 * t + (k + 2) % 3];
            const int u = M.N[3 * t + k], n_bc = M.N[3 * t + (k + 1) % 3], n_ca = M.N[3 * t + (k + 2) % 3];
            const int t1 = M.new_tri();
            int ua = -1, ub = -1;
            if (u >= 0) {
                const int ku = M.index_of(u, b), d = M.V[3 * u + (ku + 2) % 3];
                const int n_ad = M.N[3 * u + (ku + 1) % 3], n_db = M.N[3 * u + (ku + 2) % 3];
                ua = u;
                ub = M.new_tri();
                M.set_tri(ua, b, p, d, t1, ub, n_db, 0, 0, 0);
                M.set_tri(ub, p, a, d, t, n_ad, ua, 0, 0, 0);
                M.back(n_ad, d, ub);
                stack.push_back({ua, p});
                stack.push_back({ub, p});
            }
            M.set_tri(t, a, p, c, ub, t1, n_ca, 0, 0, 0);
            M.set_tri(t1, p, b, c, ua, n_bc, t, 0, 0, 0);
            M.back(n_bc, c, t1);
            stack.push_back({t, p});
            stack.push_back({t1, p});
        }
        M.legalize(&stack);
        last = M.vt[p];
    }
    // ---- the constraints: the open edges, then the rim (grid edges between a cut and a whole cell)
    std::vector<std::pair<int, int>> cons;
    for (int64_t e = 0; e < B->n_edges; ++e)
        if (B->edges[2 * e] != B->edges[2 * e + 1]) cons.push_back({int(B->edges[2 * e]), int(B->edges[2 * e + 1])});
    const int64_t n_open_cons = static_cast<int64_t>(cons.size());
    for (int64_t q = 0; q < B->n_cut; ++q) {
        const int i = B->cut[q] % nu, j = B->cut[q] / nu;
        const int side[4][6] = {{i, j - 1, i, j, i + 1, j}, {i + 1, j, i + 1, j, i + 1, j + 1}, {i, j + 1, i, j + 1, i + 1, j + 1}, {i - 1, j, i, j, i, j + 1}};
        for (int s = 0; s < 4; ++s) {
            const int ci = side[s][0], cj = side[s][1];
            if (ci < 0 || cj < 0 || ci >= nu || cj >= nv || is_cut(ci, cj)) continue;
            const int p = grid_point(side[s][2], side[s][3]), r = grid_point(side[s][4], side[s][5]);
            if (p < 0 || r < 0 || p == r) {
                *err = "closure: an open edge touches the rim of the band (the cut cells do not cover it)";
                return false;
            }
            cons.push_back({p, r});
        }
    }
    if (static_cast<int>(M.x.size()) != static_cast<int>(M.vt.size())) {
        *err = "closure: internal: a band point was made after the triangulation began";
        return false;
    }
    std::vector<std::pair<int, int>> crossed;
    for (int64_t ci = 0; ci < static_cast<int64_t>(cons.size()); ++ci) {
        const int p = cons[ci].first, q = cons[ci].second;
        const std::string what = ci < n_open_cons ? "open edge " + std::to_string(ci) : std::string("a rim edge");
        int t, k;
        if (M.find_edge(p, q, &t, &k)) {
            M.constrain(t, k);
            continue;
        }
        // the triangle at p that the segment leaves through its far edge (r right of p -> q, s left of it)
        int t0 = -1, k0 = -1;
        bool blocked = false;
        M.around(p, [&](int tt, int kk) {
            const int r = M.V[3 * tt + (kk + 1) % 3], s = M.V[3 * tt + (kk + 2) % 3];
            const int o_r = M.orient(p, q, r), o_s = M.orient(p, q, s);
            for (int w : {r, s})
                if ((w == r ? o_r : o_s) == 0 && (M.x[w] - M.x[p]) * (M.x[q] - M.x[p]) + (M.y[w] - M.y[p]) * (M.y[q] - M.y[p]) > 0) blocked = true;
            if (o_r < 0 && o_s > 0) t0 = tt, k0 = (kk + 1) % 3;
            return blocked || t0 >= 0;
        });
        if (blocked || t0 < 0) {
            *err = "closure: " + what + " passes through a vertex of the band: it cannot be kept whole";
            return false;
        }
        crossed.clear();
        for (int guard = 0;; ++guard) {
            if (M.C[3 * t0 + k0]) {
                *err = "closure: " + what + " crosses another constraint: two open edges of the mesh cross on a face of the extents";
                return false;
            }
            const int r = M.V[3 * t0 + k0], s = M.V[3 * t0 + (k0 + 1) % 3]; // edge r -> s of t0, r right and s left
            crossed.push_back({r, s});
            const int u = M.N[3 * t0 + k0];
            if (u < 0 || guard > M.ntri()) {
                *err = "closure: " + what + " leaves the face";
                return false;
            }
            const int ku = M.index_of(u, s), w = M.V[3 * u + (ku + 2) % 3]; // u holds s -> r, w opposite
            if (w == q) break;
            const int o_w = M.orient(p, q, w);
            if (o_w == 0) {
                *err = "closure: " + what + " passes through a vertex of the band: it cannot be kept whole";
                return false;
            }
            t0 = u;
            k0 = o_w > 0 ? (ku + 1) % 3 : (ku + 2) % 3; // left: leave through r -> w; right: through w -> s
        }
        size_t head = 0;
        int64_t budget = 16 + 8 * static_cast<int64_t>(crossed.size()) * static_cast<int64_t>(crossed.size());
        while (head < crossed.size()) {
            if (--budget < 0) {
                *err = "closure: " + what + " could not be recovered by flips";
                return false;
            }
            const int r = crossed[head].first, s = crossed[head].second;
            ++head;
            if (!M.find_edge(r, s, &t, &k)) {
                *err = "closure: internal: a crossed edge vanished";
                return false;
            }
            const int a = M.V[3 * t + k], b = M.V[3 * t + (k + 1) % 3], c = M.V[3 * t + (k + 2) % 3];
            const int u = M.N[3 * t + k];
            if (u < 0) {
                *err = "closure: " + what + " leaves the face";
                return false;
            }
            const int d = M.V[3 * u + (M.index_of(u, b) + 2) % 3];
            if (!M.convex(a, b, c, d)) {
                crossed.push_back({r, s});
                continue;
            }
            int t2, u2;
            M.flip(t, k, &t2, &u2);
            ++B->constraint_flips;
            if ((c == p && d == q) || (c == q && d == p)) continue;
            if (c == p || c == q || d == p || d == q) continue;
            const int oc = M.orient(p, q, c), od = M.orient(p, q, d);
            if (oc * od < 0) crossed.push_back({c, d});
        }
        if (!M.find_edge(p, q, &t, &k)) {
            *err = "closure: " + what + " could not be recovered by flips";
            return false;
        }
        M.constrain(t, k);
    }
    // ---- drop what lies off the cut cells (the rim is constrained: no triangle straddles it)
    const int nt = M.ntri();
    for (int t = 0; t < nt; ++t) {
        const int a = M.V[3 * t], b = M.V[3 * t + 1], c = M.V[3 * t + 2];
        const double cu = (M.x[a] + M.x[b] + M.x[c]) / 3.0, cv = (M.y[a] + M.y[b] + M.y[c]) / 3.0;
        if (!is_cut(lower_cell(B->gu, nu, cu), lower_cell(B->gv, nv, cv))) M.dead[t] = 1;
    }
    for (int t = 0; t < nt; ++t) {
        if (M.dead[t]) continue;
        for (int k = 0; k < 3; ++k) {
            if (M.N[3 * t + k] >= 0 && M.dead[M.N[3 * t + k]]) {
                M.N[3 * t + k] = -1;
                M.C[3 * t + k] = 1;
            }
            if (M.V[3 * t + k] >= n_band) {
                *err = "closure: the band reaches a corner of the face that is none of its points";
                return false;
            }
        }
    }
    // ---- Lawson flips on the unconstrained edges, a fixed number of passes at the most
    for (int pass = 0; pass < 32; ++pass) {
        bool changed = false;
        for (int t = 0; t < nt; ++t) {
            if (M.dead[t]) continue;
            for (int k = 0; k < 3; ++k) {
                if (M.N[3 * t + k] < 0 || !M.delaunay_wants(t, k)) continue;
                int t2, u2;
                M.flip(t, k, &t2, &u2);
                ++B->lawson_flips;
                changed = true;
            }
        }
        if (!changed) break;
    }
    B->xy.resize(2 * static_cast<size_t>(n_band));
    B->id.resize(static_cast<size_t>(n_band));
    for (int p = 0; p < n_band; ++p) B->xy[2 * p] = M.x[p], B->xy[2 * p + 1] = M.y[p];
    for (int t = 0; t < nt; ++t) {
        if (M.dead[t]) continue;
        if (M.orient(M.V[3 * t], M.V[3 * t + 1], M.V[3 * t + 2]) <= 0) {
            ++B->dropped;
            continue;
        }
        for (int k = 0; k < 3; ++k) B->tri.push_back(M.V[3 * t + k]);
    }
    return true;
}

} // namespace closure
} // namespace iso
} // namespace bbfmm
