// delaunay_star.h — the star of one point of the Delaunay triangulation, built from a uniform grid alone
// (DESIGN §5j).  One function for the host and the device, parameterised by a policy W that supplies the
// predicates and the lanes:
//   the device policy (delaunay_dev.hip): 64 lanes, the floating-point filters of delaunay.cpp's orient2d /
//     incircle and nothing behind them — a result inside the filter's bound is kUncertain and marks the star;
//   the host policy: one lane, delaunay.cpp's exact predicates — a zero marks a tie.
// The rules: the nearest neighbour q0 of p is a Delaunay neighbour.  Given a Delaunay edge a -> b, the apex of
// the triangle on its left is, among the points r with orient(a, b, r) > 0, the one that is best under the total
// order "r beats s iff incircle(a, b, s, r) > 0" (r inside the circle through a, b, s); none: a hull edge.  The
// star of p pivots on (p, cur) counter-clockwise from q0 until it is back at q0 or meets the hull, then on
// (cur, p) clockwise from q0 to the other hull edge.
// A pivot searches the grid cells that meet the disc through a, b and the best apex so far — a box of cells that
// holds an inflated bounding box of that disc (pivot_box: the stop rule) — and ends when that box has been
// searched; every loop is bounded by the grid.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DSTAR_HD __host__ __device__
#else
#define DSTAR_HD
#endif

namespace deftri {
namespace dstar {

constexpr int kUncertain = 2;                // a predicate inside its filter bound (device policy only)
enum : int {
    kMarkUncertain = 1,                      // a predicate the filter could not decide: the host rebuilds the star
    kMarkOverflow = 2,                       // more triangles than the policy's store holds: the host rebuilds it
    kMarkDuplicate = 4,                      // another point at distance exactly zero: the whole call falls back
    kMarkTie = 8,                            // an exact predicate was zero: the whole call falls back
};

// cell (cx, cy) = (int)((x - minx) * inv_cw), (int)((y - miny) * inv_ch), clamped; its list is
// items[start[cx * gy + cy] .. start[cx * gy + cy + 1]): the cells of a column are adjacent
struct Grid {
    double minx, miny, cw, ch, inv_cw, inv_ch;
    int gx, gy;
};

DSTAR_HD inline int cell_x(const Grid &G, double x) {
    const double t = (x - G.minx) * G.inv_cw;
    return !(t > 0.0) ? 0 : (t >= (double)G.gx ? G.gx - 1 : (int)t);
}
DSTAR_HD inline int cell_y(const Grid &G, double y) {
    const double t = (y - G.miny) * G.inv_ch;
    return !(t > 0.0) ? 0 : (t >= (double)G.gy ? G.gy - 1 : (int)t);
}

// the grid of n points with the bounding box [minx, maxx] x [miny, maxy]: about n cells, about square
inline Grid make_grid(int n, double minx, double miny, double maxx, double maxy) {
    Grid G;
    const double w = maxx - minx, h = maxy - miny;
    const int cap = 4096;
    G.minx = minx; G.miny = miny;
    if (w > 0.0 && h > 0.0) {
        G.gx = (int)std::fmin((double)cap, std::fmax(1.0, std::ceil(std::sqrt((double)n * (w / h)))));
        G.gy = (int)std::fmin((double)cap, std::fmax(1.0, std::ceil((double)n / G.gx)));
    } else {
        G.gx = w > 0.0 ? (n < cap ? (n > 0 ? n : 1) : cap) : 1;
        G.gy = h > 0.0 ? (n < cap ? (n > 0 ? n : 1) : cap) : 1;
    }
    G.cw = w > 0.0 ? w / G.gx : 1.0;
    G.ch = h > 0.0 ? h / G.gy : 1.0;
    G.inv_cw = 1.0 / G.cw;
    G.inv_ch = 1.0 / G.ch;
    return G;
}

struct Box {
    int x0, x1, y0, y1;                      // inclusive; x1 < x0: empty
    DSTAR_HD bool operator==(const Box &o) const { return x0 == o.x0 && x1 == o.x1 && y0 == o.y0 && y1 == o.y1; }
};
DSTAR_HD inline Box box_around(const Grid &G, int cx, int cy, int k) {
    Box b;
    b.x0 = cx - k > 0 ? cx - k : 0;
    b.x1 = cx + k < G.gx - 1 ? cx + k : G.gx - 1;      // k < 2^30: the callers stop at the whole grid
    b.y0 = cy - k > 0 ? cy - k : 0;
    b.y1 = cy + k < G.gy - 1 ? cy + k : G.gy - 1;
    return b;
}
DSTAR_HD inline bool whole_grid(const Grid &G, const Box &b) {
    return b.x0 == 0 && b.y0 == 0 && b.x1 == G.gx - 1 && b.y1 == G.gy - 1;
}

// f(r) for every point r of the cells of `box` that are not in `done` (a box inside it, or empty), the lanes
// striding over each column's run of the cell lists
template <class W, class F>
DSTAR_HD inline void for_new_points(W &w, const Grid &G, const int *start, const int *items, const Box &box, const Box &done, F f) {
    for (int cx = box.x0; cx <= box.x1; cx++) {
        const bool split = done.x1 >= done.x0 && cx >= done.x0 && cx <= done.x1;
        for (int part = 0; part < 2; part++) {
            int ya, yb;
            if (!split) {
                if (part) break;
                ya = box.y0; yb = box.y1;
            } else if (part == 0) {
                ya = box.y0; yb = done.y0 - 1;
            } else {
                ya = done.y1 + 1; yb = box.y1;
            }
            if (ya > yb) continue;
            const int s = start[cx * G.gy + ya], e = start[cx * G.gy + yb + 1];
            for (int t = s + w.lane(); t < e; t += w.lanes()) f(items[t]);
        }
    }
}

// The stop rule.  The cells a pivot on a -> b with the best apex c so far still has to search: a box of cells
// that holds the disc through a, b, c (its part left of ab is where a better apex can be).  The centre is
// a + (nx, ny) / d, d = 2 det, det = bx cy - by cx the orientation determinant of the differences from a.
// Bounds, with eps = 2^-53 and every difference, product and sum rounded once:
//   |det - true| <= 5e-16 (|bx cy| + |by cx|)     (3 eps per product, 1 eps for the difference: 4.44e-16)
//   |nx  - true| <= 1e-15 (|cy b2| + |by c2|)     (b2, c2: 4 eps; the products 6 eps; the difference 1 eps: 7.8e-16)
// With e = 5e-16 (|bx cy| + |by cx|) / |det| <= 1e-3 the centre's coordinates are off by at most
//   dux = 1.01 (Enx / |d| + |ux| e),   duy likewise,
// so the true disc lies in the computed one with the radius r (1 + 1e-12) + 2 (dux + duy) + 4e-16 (|a| + |u| + r)
// (the centre's shift, the radius' change by the same shift, and the rounding of the box's own corners).
// e > 1e-3 or anything not finite: the whole grid.  Too generous costs time, never a missed point.  The cell of
// a bound is found with the function that put the points into cells, which is monotonic, so no point on the
// inner side of a bound is in a cell outside the box.
DSTAR_HD inline Box pivot_box(const Grid &G, const double *a, const double *b, const double *c) {
    const Box all = {0, G.gx - 1, 0, G.gy - 1};
    const double bx = b[0] - a[0], by = b[1] - a[1], cx = c[0] - a[0], cy = c[1] - a[1];
    const double detl = bx * cy, detr = by * cx, det = detl - detr;
    const double e = 5e-16 * (fabs(detl) + fabs(detr)) / fabs(det);
    if (!(e <= 1e-3)) return all;
    const double b2 = bx * bx + by * by, c2 = cx * cx + cy * cy, d = 2.0 * det;
    const double n1 = cy * b2, n2 = by * c2, n3 = bx * c2, n4 = cx * b2;
    const double ux = (n1 - n2) / d, uy = (n3 - n4) / d;
    const double dux = 1.01 * (1e-15 * (fabs(n1) + fabs(n2)) / fabs(d) + fabs(ux) * e);
    const double duy = 1.01 * (1e-15 * (fabs(n3) + fabs(n4)) / fabs(d) + fabs(uy) * e);
    const double r = sqrt(ux * ux + uy * uy);
    const double rr = r * (1.0 + 1e-12) + 2.0 * (dux + duy) + 4e-16 * (fabs(a[0]) + fabs(a[1]) + fabs(ux) + fabs(uy) + r);
    const double xlo = a[0] + ux - rr, xhi = a[0] + ux + rr, ylo = a[1] + uy - rr, yhi = a[1] + uy + rr;
    if (!(xhi - xlo < INFINITY) || !(yhi - ylo < INFINITY)) return all;        // also NaN
    Box q = {cell_x(G, xlo), cell_x(G, xhi), cell_y(G, ylo), cell_y(G, yhi)};
    return q;
}

DSTAR_HD inline Box box_union(const Box &p, const Box &q) {
    if (p.x1 < p.x0) return q;
    Box u;
    u.x0 = p.x0 < q.x0 ? p.x0 : q.x0; u.x1 = p.x1 > q.x1 ? p.x1 : q.x1;
    u.y0 = p.y0 < q.y0 ? p.y0 : q.y0; u.y1 = p.y1 > q.y1 ? p.y1 : q.y1;
    return u;
}

// the marks of all lanes, on every lane
template <class W>
DSTAR_HD inline int wave_or(W &w, int v) {
    for (int m = 1; m < w.lanes(); m <<= 1) v |= w.xchg(v, m);
    return v;
}

// The nearest neighbour of p (cell pcx, pcy); -1: there is no other point.  The window grows ring by ring: a
// point outside the window of k rings is at least k min(cw, ch) away (p is in its own cell), so the search ends
// when the best squared distance is below (k min(cw, ch))^2 (1 - 1e-9).  An exact policy compares with the exact
// sign behind a filter (two equally near points are both Delaunay neighbours: the lower index is taken); the
// filter policy takes the fp64 order and marks the star when the runner-up is within the rounding of the two
// squared distances, |d - true| <= 4.44e-16 d each: d2 - d1 <= 1e-15 d2.
template <class W>
DSTAR_HD inline int nearest(W &w, const Grid &G, const double *xy, const int *start, const int *items, int p, int pcx, int pcy,
                            int &mark) {
    const double P[2] = {xy[2 * (size_t)p], xy[2 * (size_t)p + 1]};
    const double cmin = G.cw < G.ch ? G.cw : G.ch;
    double d1 = INFINITY, d2 = INFINITY;
    int i1 = -1;
    Box done = {0, -1, 0, -1};
    for (int k = 0;; k = 2 * k + 1) {
        const Box box = box_around(G, pcx, pcy, k);
        for_new_points(w, G, start, items, box, done, [&](int r) {
            if (r == p) return;
            const double dx = xy[2 * (size_t)r] - P[0], dy = xy[2 * (size_t)r + 1] - P[1];
            const double d = dx * dx + dy * dy;
            if (d == 0.0) mark |= kMarkDuplicate;
            if (i1 < 0 || w.nearer(xy, p, r, d, i1, d1)) {
                d2 = d1; d1 = d; i1 = r;
            } else if (d < d2) {
                d2 = d;
            }
        });
        // the wave's best, then the runner-up among the lanes' bests and seconds
        for (int m = 1; m < w.lanes(); m <<= 1) {
            const int oi = w.xchg(i1, m);
            const double od1 = w.xchg(d1, m), od2 = w.xchg(d2, m);
            if (oi >= 0 && oi != i1 && (i1 < 0 || w.nearer(xy, p, oi, od1, i1, d1))) {
                d2 = d1 < od2 ? d1 : od2; d1 = od1; i1 = oi;
            } else if (oi != i1) {
                d2 = od1 < d2 ? od1 : d2;
            } else {
                d2 = od2 < d2 ? od2 : d2;
            }
        }
        i1 = w.bcast0(i1); d1 = w.bcast0(d1); d2 = w.bcast0(d2);
        done = box;
        mark = wave_or(w, mark);                 // every lane leaves with the same marks
        if (mark) return -1;
        const double reach = (double)k * cmin;
        if (whole_grid(G, box) || (i1 >= 0 && d1 < reach * reach * (1.0 - 1e-9))) break;
    }
    // no runner-up in the window (d2 infinite): every other point is beyond the reach, so the best is certain
    if (!W::kExact && i1 >= 0 && d2 < INFINITY && !(d2 - d1 > 1e-15 * d2)) mark |= kMarkUncertain;
    return i1;
}

// The apex of the triangle left of a -> b; -1: none (a hull edge), or a mark was set.  (ccx, ccy): the centre of
// the search windows, the cell of the star's point (a or b).
template <class W>
DSTAR_HD inline int pivot(W &w, const Grid &G, const double *xy, const int *start, const int *items, int ia, int ib, int ccx, int ccy,
                          int &mark) {
    const double A[2] = {xy[2 * (size_t)ia], xy[2 * (size_t)ia + 1]}, B[2] = {xy[2 * (size_t)ib], xy[2 * (size_t)ib + 1]};
    auto better = [&](int mine, int r) {             // does r beat mine (both left of ab)?
        const int c = w.incircle(A, B, xy + 2 * (size_t)mine, xy + 2 * (size_t)r);
        if (c == kUncertain) mark |= kMarkUncertain;
        else if (c == 0) mark |= kMarkTie;
        return c == 1;
    };
    // the first window holds both ends of the edge
    int k = 1;
    {
        const int acx = cell_x(G, A[0]) - ccx, acy = cell_y(G, A[1]) - ccy, bcx = cell_x(G, B[0]) - ccx, bcy = cell_y(G, B[1]) - ccy;
        const int m1 = (acx < 0 ? -acx : acx) > (acy < 0 ? -acy : acy) ? (acx < 0 ? -acx : acx) : (acy < 0 ? -acy : acy);
        const int m2 = (bcx < 0 ? -bcx : bcx) > (bcy < 0 ? -bcy : bcy) ? (bcx < 0 ? -bcx : bcx) : (bcy < 0 ? -bcy : bcy);
        k = (m1 > m2 ? m1 : m2) + 1;
    }
    Box done = {0, -1, 0, -1}, box = box_around(G, ccx, ccy, k);
    int best = -1;
    for (;;) {
        int mine = best;
        for_new_points(w, G, start, items, box, done, [&](int r) {
            if (r == ia || r == ib) return;
            const int o = w.orient(A, B, xy + 2 * (size_t)r);
            if (o == kUncertain) { mark |= kMarkUncertain; return; }
            if (o == 0) { mark |= kMarkTie; return; }
            if (o < 0) return;
            if (mine < 0 || better(mine, r)) mine = r;
        });
        // the tournament: the order is total, so the winner does not depend on how the lanes met
        for (int m = 1; m < w.lanes(); m <<= 1) {
            const int other = w.xchg(mine, m);
            if (other >= 0 && other != mine && (mine < 0 || better(mine, other))) mine = other;
        }
        best = w.bcast0(mine);
        done = box;
        mark = wave_or(w, mark);                 // every lane leaves with the same marks
        if (mark) return -1;
        if (whole_grid(G, box)) break;
        if (best < 0) {
            k = 2 * k + 1;
            box = box_around(G, ccx, ccy, k);
        } else {
            box = box_union(done, pivot_box(G, A, B, xy + 2 * (size_t)best));
            if (box == done) break;
        }
    }
    return best;
}

struct Star {
    int mark = 0;        // kMark*
    int degree = 0;      // neighbours
    int hull = 0;        // 1: p is a hull vertex
    int ntri = 0;        // triangles pushed to the policy's store, (p, second, third) counter-clockwise
};

// The star of p.  Every triangle goes to w.push(second, third) (false: the store is full).  `limit` bounds the
// sweeps (n is enough: a star has fewer than n triangles).
template <class W>
DSTAR_HD inline Star build_star(W &w, const Grid &G, const double *xy, const int *start, const int *items, int p, int limit) {
    Star S;
    const int pcx = cell_x(G, xy[2 * (size_t)p]), pcy = cell_y(G, xy[2 * (size_t)p + 1]);
    const int q0 = nearest(w, G, xy, start, items, p, pcx, pcy, S.mark);
    if (S.mark || q0 < 0) return S;
    S.degree = 1;
    int cur = q0;
    bool closed = false;
    for (int step = 0;; step++) {
        const int r = pivot(w, G, xy, start, items, p, cur, pcx, pcy, S.mark);
        if (S.mark) return S;
        if (r < 0) break;
        if (step >= limit) { S.mark |= kMarkUncertain; return S; }
        if (!w.push(cur, r)) { S.mark |= kMarkOverflow; return S; }
        S.ntri++;
        cur = r;
        if (cur == q0) { closed = true; break; }
        S.degree++;
    }
    if (closed) return S;
    S.hull = 1;
    cur = q0;
    for (int step = 0;; step++) {
        const int r = pivot(w, G, xy, start, items, cur, p, pcx, pcy, S.mark);
        if (S.mark) return S;
        if (r < 0) break;
        if (step >= limit) { S.mark |= kMarkUncertain; return S; }
        if (!w.push(r, cur)) { S.mark |= kMarkOverflow; return S; }
        S.ntri++;
        cur = r;
        S.degree++;
    }
    return S;
}

// delaunay.cpp's two filters, the same expressions and constants, and nothing behind them (compile with
// -ffp-contract=off): +1 / -1 are the exact signs, kUncertain everything within the bound
DSTAR_HD inline int orient_filter(const double *a, const double *b, const double *c) {
    const double detl = (a[0] - c[0]) * (b[1] - c[1]);
    const double detr = (a[1] - c[1]) * (b[0] - c[0]);
    const double det = detl - detr;
    const double bound = 3.3306690738754716e-16 * (fabs(detl) + fabs(detr));
    if (det > bound) return 1;
    if (-det > bound) return -1;
    return kUncertain;
}
DSTAR_HD inline int incircle_filter(const double *a, const double *b, const double *c, const double *d) {
    const double adx = a[0] - d[0], ady = a[1] - d[1], bdx = b[0] - d[0], bdy = b[1] - d[1];
    const double cdx = c[0] - d[0], cdy = c[1] - d[1];
    const double bdxcdy = bdx * cdy, cdxbdy = cdx * bdy, cdxady = cdx * ady, adxcdy = adx * cdy;
    const double adxbdy = adx * bdy, bdxady = bdx * ady;
    const double alift = adx * adx + ady * ady, blift = bdx * bdx + bdy * bdy, clift = cdx * cdx + cdy * cdy;
    const double det = alift * (bdxcdy - cdxbdy) + blift * (cdxady - adxcdy) + clift * (adxbdy - bdxady);
    const double perm = (fabs(bdxcdy) + fabs(cdxbdy)) * alift + (fabs(cdxady) + fabs(adxcdy)) * blift +
                        (fabs(adxbdy) + fabs(bdxady)) * clift;
    const double bound = 1.2e-15 * perm;
    if (det > bound) return 1;
    if (-det > bound) return -1;
    return kUncertain;
}

}  // namespace dstar
}  // namespace deftri
