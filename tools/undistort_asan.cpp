// undistort_asan.cpp — the host loops of deftri_undistort_points, deftri_image_bounds and
// deftri_distribute_features (csrc/undistort.hip, a host-only context's path) under AddressSanitizer and
// UndefinedBehaviorSanitizer, on keypoints, cell lists and flags held in heap blocks of exactly the documented
// sizes, so that a read or write past an array's end is caught.  CPU only: device = -1, no GPU call is made.
//
// Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/undistort_asan.cpp \
//         triangulation-in-deformable-scenes_amd/csrc/undistort.hip triangulation-in-deformable-scenes_amd/csrc/matching.hip \
//         -o undistort_asan
//   ./undistort_asan
// The edge cases are those of tests/test_undistort.py: n = 0, 1, 63, 64, 65 and 257 slots with a keypoint in the
// last half cell, one that rounds to column -1, a NaN and a zero slot; the in-place calls; 4, 5 and no
// coefficients; all-zero coefficients; k1 = -2 (a negative icdist); a crowded cell; every refused argument.
// Prints one line per case and ends with "clean" unless a sanitizer stopped it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../triangulation-in-deformable-scenes_amd/csrc/undistort.h"

static const float CALIB[4] = {458.654f, 457.296f, 367.215f, 248.375f};
static const float DIST5[5] = {-0.28340811f, 0.07395907f, 0.00019359f, 1.76187114e-05f, 0.01f};
static const int COLS = 752, ROWS = 480, GRID_COLS = 16, GRID_ROWS = 12;

static void die(const char *what, int rc, const std::string &err) {
    std::fprintf(stderr, "%s: %d %s\n", what, rc, err.c_str());
    std::exit(1);
}

// n slots: a fixed pseudo-random sample of the image, and from 4 slots on the special ones at the end
static std::unique_ptr<float[]> slots(int n) {
    std::unique_ptr<float[]> uv(new float[2 * (size_t)n]);
    uint32_t s = 12345u;
    for (int i = 0; i < 2 * n; i++) {
        s = s * 1664525u + 1013904223u;
        uv[i] = (float)(s >> 8) / 16777216.0f * (float)((i & 1) ? ROWS : COLS);
    }
    if (n >= 4) {
        const float special[8] = {745.0f, 10.0f, -40.0f, 240.0f, NAN, 100.0f, 0.0f, 0.0f};
        std::memcpy(uv.get() + 2 * (n - 4), special, sizeof(special));
    }
    return uv;
}

static void points_case(int n, const float *dist, int n_dist, const char *name) {
    const auto in = slots(n);
    std::unique_ptr<float[]> out(new float[2 * (size_t)n]), inplace(new float[2 * (size_t)n]);
    std::memcpy(inplace.get(), in.get(), 8 * (size_t)n);
    std::string err;
    int rc = deftri::undistort_points(-1, nullptr, n, in.get(), CALIB, dist, n_dist, out.get(), err);
    if (!rc) rc = deftri::undistort_points(-1, nullptr, n, inplace.get(), CALIB, dist, n_dist, inplace.get(), err);
    if (rc) die(name, rc, err);
    if (std::memcmp(out.get(), inplace.get(), 8 * (size_t)n)) die(name, 0, "the in-place call differs");
    std::printf("points %s n %d ok\n", name, n);
}

static void distribute_case(int n, const float *dist, int n_dist, bool with_flags, bool in_place) {
    const auto dis = slots(n);
    const size_t ncell = (size_t)GRID_COLS * GRID_ROWS;
    std::unique_ptr<float[]> uv(new float[2 * (size_t)n]);
    std::unique_ptr<int32_t[]> start(new int32_t[ncell + 1]), items(new int32_t[(size_t)n]);
    std::unique_ptr<uint8_t[]> flags(new uint8_t[(size_t)n]);
    deftri_feature_grid g;
    std::string err;
    float *out = in_place ? dis.get() : uv.get();
    const int rc = deftri::distribute_features(-1, nullptr, GRID_COLS, GRID_ROWS, 8, 1.2f, COLS, ROWS, CALIB, dist, n_dist, n, dis.get(),
                                               out, &g, start.get(), items.get(), with_flags ? flags.get() : nullptr, err);
    if (rc) die("distribute_features", rc, err);
    int in_cells = 0;
    for (int k = 0; k < n; k++) in_cells += items[k] >= 0;
    if (start[ncell] != in_cells || start[0] != 0) die("distribute_features", 0, "cell_start does not end at the number of items");
    std::printf("distribute n %d n_dist %d flags %d in_place %d: %d in cells, bounds %.4f %.4f %.4f %.4f\n", n, n_dist, (int)with_flags,
                (int)in_place, in_cells, g.min_col, g.min_row, g.max_col, g.max_row);
}

static void refused(int rc, const std::string &err, const char *what) {
    if (rc != DEFTRI_E_ARG || err.empty()) die(what, rc, "was not refused with a message");
}

int main() {
    const float zeros[5] = {0, 0, 0, 0, 0}, fold[4] = {-2.0f, 0, 0, 0};
    const int sizes[] = {0, 1, 63, 64, 65, 257};
    for (int n : sizes) {
        points_case(n, DIST5, 4, "k1k2p1p2");
        points_case(n, DIST5, 5, "k3");
    }
    points_case(65, zeros, 4, "zeros");
    points_case(65, zeros, 5, "zeros5");
    points_case(257, fold, 4, "negative_icdist");
    for (int n : sizes)
        for (int n_dist : {0, 4, 5}) {
            distribute_case(n, DIST5, n_dist, true, false);
            distribute_case(n, DIST5, n_dist, false, true);
        }
    {   // a crowded cell: 300 zero slots
        std::unique_ptr<float[]> dis(new float[600]()), uv(new float[600]);
        std::unique_ptr<int32_t[]> start(new int32_t[GRID_COLS * GRID_ROWS + 1]), items(new int32_t[300]);
        deftri_feature_grid g;
        std::string err;
        const int rc = deftri::distribute_features(-1, nullptr, GRID_COLS, GRID_ROWS, 8, 1.2f, COLS, ROWS, CALIB, DIST5, 4, 300, dis.get(),
                                                   uv.get(), &g, start.get(), items.get(), nullptr, err);
        if (rc || start[1] != 300 || items[299] != 299) die("crowded", rc, err);
        std::printf("crowded cell ok\n");
    }
    {   // every refused argument: nothing is written
        float b[4], uv[2] = {1, 2}, bad[4] = {0.0f, 457.296f, 367.215f, 248.375f}, nan_cx[4] = {458.654f, 457.296f, NAN, 248.375f};
        int32_t start[2], item[1];
        deftri_feature_grid g;
        std::string err;
        refused(deftri::undistort_points(-1, nullptr, 1, uv, CALIB, DIST5, 3, uv, err), err, "n_dist 3");
        refused(deftri::undistort_points(-1, nullptr, 1, uv, CALIB, DIST5, 0, uv, err), err, "n_dist 0");
        refused(deftri::undistort_points(-1, nullptr, 1, uv, bad, DIST5, 4, uv, err), err, "fx 0");
        refused(deftri::image_bounds(COLS, ROWS, bad, DIST5, 4, b, err), err, "bounds fx 0");
        refused(deftri::image_bounds(COLS, ROWS, nan_cx, DIST5, 4, b, err), err, "bounds cx NaN");
        refused(deftri::image_bounds(0, ROWS, nullptr, nullptr, 0, b, err), err, "bounds cols 0");
        refused(deftri::distribute_features(-1, nullptr, 0, 1, 8, 1.2f, COLS, ROWS, CALIB, DIST5, 4, 1, uv, uv, &g, start, item, nullptr, err),
                err, "grid_cols 0");
        refused(deftri::distribute_features(-1, nullptr, 4097, 4096, 8, 1.2f, COLS, ROWS, CALIB, DIST5, 4, 1, uv, uv, &g, start, item,
                                            nullptr, err), err, "2^24 cells");
        refused(deftri::distribute_features(-1, nullptr, 1, 1, 8, 1.2f, COLS, ROWS, nan_cx, DIST5, 4, 1, uv, uv, &g, start, item, nullptr,
                                            err), err, "cx NaN");
        if (deftri::image_bounds(COLS, ROWS, nullptr, nullptr, 0, b, err) || b[2] != 752.0f || b[3] != 480.0f) die("bounds", 0, err);
        std::printf("refusals ok\n");
    }
    std::printf("clean\n");
    return 0;
}
