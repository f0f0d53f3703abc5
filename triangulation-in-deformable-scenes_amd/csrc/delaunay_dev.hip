// delaunay_dev.hip — the Delaunay mesh on the device, one star per wave (the star itself is
// delaunay_star.h, shared with the host).
//   k_dl_cells     the cell of every point and the cells' sizes; the lists come from the matchers' scan / fill /
//                  order kernels (matching.hip), so every cell is in point order
//   k_stars<false> one wave per point builds its star and counts the triangles in which the point is the smallest
//                  vertex; a star with an uncertain predicate or more than 64 triangles is marked and counts none
//   k_excl_scan    the rows' offsets (dev_scan.h)
//   k_stars<true>  the same stars again, each writing its row, sorted by the second vertex, where the scan put it
// Counting first and building twice, not a fixed slab per point: the rows land in the canonical order at their
// exact sizes, no capacity decides which stars are marked, and a point of degree 60 that is the smallest of all
// its neighbours costs nothing extra.  The price is the second run of the star kernel (profiles/delaunay_time.json).
// One upload (xy), one blocking download (marks, offsets, cell lists, triangles).  The host then rebuilds the marked
// stars with the exact predicates from the downloaded cell lists and merges their rows; a tie, a duplicate, too
// many marked stars or n < 3 run delaunay2d instead.  Compile with -ffp-contract=off: the filters' bounds hold for
// one rounding per operation.
#include "delaunay_dev.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "delaunay.h"
#include "delaunay_star.h"
#include "dev_arena.h"
#include "dev_scan.h"
#include "matching_grid.h"

namespace deftri {

using dstar::Grid;
using dstar::Star;

namespace dev {

struct StarWave {                            // the device policy: 64 lanes, the filters alone
    static constexpr bool kExact = false;
    int lane_;
    int (*tri_)[2];                          // the star's triangles (second, third), in LDS
    int nt_;
    __device__ int lanes() const { return 64; }
    __device__ int lane() const { return lane_; }
    __device__ int orient(const double *a, const double *b, const double *c) const { return dstar::orient_filter(a, b, c); }
    __device__ int incircle(const double *a, const double *b, const double *c, const double *d) const {
        return dstar::incircle_filter(a, b, c, d);
    }
    __device__ bool nearer(const double *, int, int r, double d, int i1, double d1) const { return d < d1 || (d == d1 && r < i1); }
    __device__ int xchg(int v, int m) const { return __shfl_xor(v, m, 64); }
    __device__ double xchg(double v, int m) const { return __shfl_xor(v, m, 64); }
    __device__ int bcast0(int v) const { return __shfl(v, 0, 64); }
    __device__ double bcast0(double v) const { return __shfl(v, 0, 64); }
    __device__ bool push(int b, int c) {
        if (nt_ >= 64) return false;
        if (lane_ == 0) { tri_[nt_][0] = b; tri_[nt_][1] = c; }
        nt_++;
        return true;
    }
};

__global__ void k_dl_cells(int n, Grid G, const double *__restrict__ xy, int *__restrict__ cell, int *__restrict__ count) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int id = dstar::cell_x(G, xy[2 * (size_t)i]) * G.gy + dstar::cell_y(G, xy[2 * (size_t)i + 1]);
    cell[i] = id;
    atomicAdd(&count[id], 1);
}

// status [p] = mark | hull << 8 | degree << 16.  tris has room for tri_cap triangles.
template <bool FILL>
__global__ void __launch_bounds__(256) k_stars(int n, Grid G, const double *__restrict__ xy, const int *__restrict__ start,
                                               const int *__restrict__ items, int *__restrict__ status, int *__restrict__ tcount,
                                               const int *__restrict__ toff, int *__restrict__ tris, int tri_cap) {
    __shared__ int lds[4][64][2];
    const int wv = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int p = (int)blockIdx.x * 4 + wv;
    bool active = p < n;                                     // uniform over the wave
    if (FILL && active) active = (status[p] & 0xff) == 0;
    Star S;
    if (active) {
        StarWave w{lane, lds[wv], 0};
        S = dstar::build_star(w, G, xy, start, items, p, 64);
    }
    __syncthreads();                                         // lane 0's triangles, read by every lane below
    const bool good = active && S.mark == 0;
    int b = -1, c = -1;
    if (good && lane < S.ntri) { b = lds[wv][lane][0]; c = lds[wv][lane][1]; }
    const bool emit = p < b && p < c;
    if (!FILL) {
        const int cnt = __popcll(__ballot(emit ? 1 : 0));
        if (active && lane == 0) {
            tcount[p] = good ? cnt : 0;
            status[p] = S.mark | S.hull << 8 | S.degree << 16;
        }
    } else if (emit) {
        int rank = 0;                                        // a neighbour is the second vertex of one triangle
        for (int t = 0; t < S.ntri; t++) {
            const int bb = lds[wv][t][0], cc = lds[wv][t][1];
            rank += (p < bb && p < cc && bb < b) ? 1 : 0;
        }
        const int at = toff[p] + rank;
        if (at < toff[p + 1] && at < tri_cap) {
            tris[3 * (size_t)at] = p;
            tris[3 * (size_t)at + 1] = b;
            tris[3 * (size_t)at + 2] = c;
        }
    }
}

}  // namespace dev

namespace {

struct HostWave {                            // the host policy: one lane, the exact predicates
    static constexpr bool kExact = true;
    std::vector<int32_t> tri;                // (second, third) per triangle
    int lanes() const { return 1; }
    int lane() const { return 0; }
    int orient(const double *a, const double *b, const double *c) const { return orient2d_sign(a, b, c); }
    int incircle(const double *a, const double *b, const double *c, const double *d) const { return incircle_sign(a, b, c, d); }
    bool nearer(const double *xy, int p, int r, double d, int i1, double d1) const {
        if (std::fabs(d - d1) > 1e-15 * std::fmax(d, d1)) return d < d1;
        const int s = dist2_cmp_sign(xy + 2 * (size_t)p, xy + 2 * (size_t)r, xy + 2 * (size_t)i1);
        return s < 0 || (s == 0 && r < i1);
    }
    int xchg(int v, int) const { return v; }
    double xchg(double v, int) const { return v; }
    int bcast0(int v) const { return v; }
    double bcast0(double v) const { return v; }
    bool push(int b, int c) { tri.push_back(b); tri.push_back(c); return true; }
};

// the star of p with the exact predicates; its row (the triangles in which p is the smallest vertex, sorted by
// the second) is appended to rows
Star host_star(const Grid &G, const double *xy, const int *start, const int *items, int p, int n, HostWave &w,
               std::vector<int32_t> &rows) {
    w.tri.clear();
    const Star S = dstar::build_star(w, G, xy, start, items, p, n);
    if (S.mark) return S;
    const size_t at = rows.size();
    for (size_t t = 0; t + 1 < w.tri.size(); t += 2)
        if (p < w.tri[t] && p < w.tri[t + 1]) { rows.push_back(p); rows.push_back(w.tri[t]); rows.push_back(w.tri[t + 1]); }
    const size_t k = (rows.size() - at) / 3;
    for (size_t i = 1; i < k; i++)           // insertion sort by the second vertex (a point starts ~2 triangles)
        for (size_t j = i; j > 0 && rows[at + 3 * (j - 1) + 1] > rows[at + 3 * j + 1]; j--)
            for (int c = 1; c < 3; c++) std::swap(rows[at + 3 * (j - 1) + c], rows[at + 3 * j + c]);
    return S;
}

// the whole-call fallback: delaunay2d's triangles, hull_size, skipped and return value
int sweep(int why, int32_t n, const double *xy, std::vector<int32_t> &tris, deftri_delaunay_report &rep) {
    int hull = 0, skipped = 0;
    const bool ok = delaunay2d(xy, n, tris, hull, skipped);
    rep.path = 0;
    rep.fallback = why;
    rep.max_degree = 0;
    rep.n_tris = ok ? (int32_t)(tris.size() / 3) : 0;
    rep.hull_size = ok ? hull : 0;
    rep.skipped = skipped;
    if (!ok) tris.clear();
    return ok || n < 3 ? 0 : DEFTRI_E_GRAPH;
}

size_t pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

DelaunayDevice::~DelaunayDevice() {
    if (!buf_ && !pin_ && !ev_[0]) return;
    hipSetDevice(dev_);
    if (buf_) hipFree(buf_);
    if (pin_) hipHostFree(pin_);
    for (hipEvent_t e : ev_) if (e) hipEventDestroy(e);
}

bool DelaunayDevice::reserve(size_t dev_bytes, size_t pin_bytes) {
    if (!ev_[0])
        for (hipEvent_t &e : ev_) if (hipEventCreate(&e) != hipSuccess) return false;
    if (dev_bytes > cap_) {
        if (buf_) hipFree(buf_);
        buf_ = nullptr; cap_ = 0;
        const size_t want = dev_bytes + dev_bytes / 4;
        if (hipMalloc((void **)&buf_, want) != hipSuccess) return false;
        cap_ = want;
    }
    if (pin_bytes > pin_cap_) {
        if (pin_) hipHostFree(pin_);
        pin_ = nullptr; pin_cap_ = 0;
        const size_t want = pin_bytes + pin_bytes / 4;
        if (hipHostMalloc((void **)&pin_, want, hipHostMallocDefault) != hipSuccess) return false;
        pin_cap_ = want;
    }
    return true;
}

int delaunay_stars(DelaunayDevice *dd, int32_t n, const double *xy, std::vector<int32_t> &tris, deftri_delaunay_report &rep,
                   std::string &err) {
    const auto t_call = std::chrono::steady_clock::now();
    std::memset(&rep, 0, sizeof(rep));
    tris.clear();
    auto done = [&](int rc) { rep.ms_total = ms_since(t_call); return rc; };
    if (n < 3) return done(sweep(4, n, xy, tris, rep));
    double minx = xy[0], maxx = xy[0], miny = xy[1], maxy = xy[1];
    for (int32_t i = 1; i < n; i++) {
        minx = std::fmin(minx, xy[2 * (size_t)i]); maxx = std::fmax(maxx, xy[2 * (size_t)i]);
        miny = std::fmin(miny, xy[2 * (size_t)i + 1]); maxy = std::fmax(maxy, xy[2 * (size_t)i + 1]);
    }
    const Grid G = dstar::make_grid(n, minx, miny, maxx, maxy);
    const size_t ncell = (size_t)G.gx * G.gy, N = (size_t)n;
    HostWave hw;

    if (!dd) {
        // the same stars, every one with the exact predicates, in a sequential loop
        rep.path = 1;
        std::vector<int32_t> start(ncell + 1, 0), items(N), cell(N);
        for (size_t i = 0; i < N; i++) {
            cell[i] = dstar::cell_x(G, xy[2 * i]) * G.gy + dstar::cell_y(G, xy[2 * i + 1]);
            start[cell[i] + 1]++;
        }
        for (size_t c = 0; c < ncell; c++) start[c + 1] += start[c];
        {
            std::vector<int32_t> cur(start.begin(), start.end() - 1);
            for (size_t i = 0; i < N; i++) items[cur[cell[i]]++] = (int32_t)i;
        }
        int marks = 0, hull = 0, maxdeg = 0;
        for (int32_t p = 0; p < n; p++) {
            const Star S = host_star(G, xy, start.data(), items.data(), p, n, hw, tris);
            marks |= S.mark;
            if (S.mark) break;
            hull += S.hull;
            maxdeg = std::max(maxdeg, S.degree);
        }
        rep.ms_host = ms_since(t_call);
        if (marks & dstar::kMarkDuplicate) return done(sweep(2, n, xy, tris, rep));
        if (marks & dstar::kMarkTie) {
            // a duplicate comes first: one further on would also have been met as a tie of its neighbours
            for (size_t c = 0; c < ncell; c++)
                for (int32_t k = start[c]; k + 1 < start[c + 1]; k++)
                    for (int32_t m = k + 1; m < start[c + 1]; m++)
                        if (xy[2 * (size_t)items[k]] == xy[2 * (size_t)items[m]] && xy[2 * (size_t)items[k] + 1] == xy[2 * (size_t)items[m] + 1])
                            return done(sweep(2, n, xy, tris, rep));
            return done(sweep(1, n, xy, tris, rep));
        }
        rep.n_tris = (int32_t)(tris.size() / 3);
        rep.hull_size = hull;
        rep.max_degree = maxdeg;
        rep.host_stars = n;
        return done(0);
    }

    std::lock_guard<std::mutex> lock(dd->mu_);
    hipSetDevice(dd->dev_);
    hipStream_t st = dd->st_;
    const int tri_cap = 2 * n;
    // the device pieces; the last five are one region, downloaded in one copy
    size_t o = 0;
    auto piece = [&](size_t bytes) { const size_t at = o; o += pad(bytes); return at; };
    const size_t o_xy = piece(16 * N), o_cell = piece(4 * N), o_keys = piece(4 * N), o_count = piece(4 * ncell),
                 o_cursor = piece(4 * ncell), o_tcount = piece(4 * N);
    const size_t o_out = o;
    const size_t o_status = piece(4 * N), o_toff = piece(4 * (N + 1)), o_start = piece(4 * (ncell + 1)), o_items = piece(4 * N),
                 o_tris = piece(12 * (size_t)tri_cap);
    const size_t out_bytes = o - o_out;
    if (!dd->reserve(o, out_bytes)) {
        err = "delaunay2d: allocation failed";
        return done(DEFTRI_E_HIP);
    }
    char *D = dd->buf_;
    double *d_xy = (double *)(D + o_xy);
    int *d_cell = (int *)(D + o_cell), *d_keys = (int *)(D + o_keys), *d_count = (int *)(D + o_count), *d_cursor = (int *)(D + o_cursor),
        *d_tcount = (int *)(D + o_tcount), *d_status = (int *)(D + o_status), *d_toff = (int *)(D + o_toff),
        *d_start = (int *)(D + o_start), *d_items = (int *)(D + o_items), *d_tris = (int *)(D + o_tris);
    hipMemcpyAsync(d_xy, xy, 16 * N, hipMemcpyHostToDevice, st);
    hipEventRecord(dd->ev_[0], st);
    hipMemsetAsync(d_count, 0, 4 * ncell, st);
    hipLaunchKernelGGL(dev::k_dl_cells, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, n, G, d_xy, d_cell, d_count);
    launch_grid_lists((int)ncell, n, d_cell, d_count, d_start, d_cursor, d_keys, st);
    launch_grid_order(n, d_cell, d_start, d_keys, d_items, st);
    hipEventRecord(dd->ev_[1], st);
    const dim3 sgrid((unsigned)((N + 3) / 4));
    hipLaunchKernelGGL(dev::k_stars<false>, sgrid, dim3(256), 0, st, n, G, d_xy, d_start, d_items, d_status, d_tcount, d_toff, d_tris,
                       tri_cap);
    dev::launch_excl_scan<int, 1024>(n, d_tcount, d_toff, nullptr, st);
    hipLaunchKernelGGL(dev::k_stars<true>, sgrid, dim3(256), 0, st, n, G, d_xy, d_start, d_items, d_status, d_tcount, d_toff, d_tris,
                       tri_cap);
    hipEventRecord(dd->ev_[2], st);
    hipMemcpyAsync(dd->pin_, D + o_out, out_bytes, hipMemcpyDeviceToHost, st);
    const hipError_t e = hipStreamSynchronize(st);
    rep.round_trips = 1;
    if (e != hipSuccess) {
        err = std::string("delaunay2d: ") + hipGetErrorString(e);
        return done(DEFTRI_E_HIP);
    }
    float ms = 0;
    if (hipEventElapsedTime(&ms, dd->ev_[0], dd->ev_[1]) == hipSuccess) rep.ms_grid = ms;
    if (hipEventElapsedTime(&ms, dd->ev_[1], dd->ev_[2]) == hipSuccess) rep.ms_stars = ms;
    const auto t_host = std::chrono::steady_clock::now();
    const char *H = dd->pin_;
    const int *status = (const int *)(H + (o_status - o_out)), *toff = (const int *)(H + (o_toff - o_out)),
              *start = (const int *)(H + (o_start - o_out)), *items = (const int *)(H + (o_items - o_out)),
              *dtris = (const int *)(H + (o_tris - o_out));
    rep.path = 2;
    std::vector<int32_t> marked;
    int marks = 0, hull = 0, maxdeg = 0;
    for (int32_t p = 0; p < n; p++) {
        const int s = status[p];
        marks |= s & 0xff;
        if (s & 0xff) { marked.push_back(p); continue; }     // its hull flag and degree come from the host's star
        hull += (s >> 8) & 1;
        maxdeg = std::max(maxdeg, s >> 16);
    }
    const int ndev = toff[n];
    if (marks & dstar::kMarkDuplicate) return done(sweep(2, n, xy, tris, rep));
    if ((int)marked.size() > std::max(64, n / 64)) return done(sweep(3, n, xy, tris, rep));
    if (ndev < 0 || ndev > tri_cap) {
        err = "delaunay2d: the device wrote an impossible triangle count";
        return done(DEFTRI_E_INTERNAL);
    }
    rep.host_stars = (int32_t)marked.size();
    if (marked.empty()) {
        tris.assign(dtris, dtris + 3 * (size_t)ndev);
    } else {
        // the marked stars again with the exact predicates, their rows merged in point order
        tris.reserve(3 * (size_t)ndev + 64 * marked.size());
        int32_t from = 0;
        for (int32_t p : marked) {
            tris.insert(tris.end(), dtris + 3 * (size_t)toff[from], dtris + 3 * (size_t)toff[p]);
            const Star S = host_star(G, xy, start, items, p, n, hw, tris);
            if (S.mark & dstar::kMarkDuplicate) return done(sweep(2, n, xy, tris, rep));
            if (S.mark & dstar::kMarkTie) return done(sweep(1, n, xy, tris, rep));
            hull += S.hull;
            maxdeg = std::max(maxdeg, S.degree);
            from = p + 1;
        }
        tris.insert(tris.end(), dtris + 3 * (size_t)toff[from], dtris + 3 * (size_t)ndev);
    }
    rep.n_tris = (int32_t)(tris.size() / 3);
    rep.hull_size = hull;
    rep.max_degree = maxdeg;
    rep.ms_host = ms_since(t_host);
    return done(0);
}

}  // namespace deftri
