// window_search_asan.cpp — the host window search of the descriptor matchers (host_window_best of
// csrc/matching_grid.h, called by match_for_initialization of csrc/matching.hip and by projection_match of
// csrc/projection_matching.hip in its search, guided and fuse modes) under AddressSanitizer and
// UndefinedBehaviorSanitizer, on a scene in heap blocks of exactly the sizes the entries document, so that a read
// past a frame, a cell list or a slot table, or a write past an output, is caught.  CPU only: device = -1, no GPU
// call is made.
//
// Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/window_search_asan.cpp \
//         triangulation-in-deformable-scenes_amd/csrc/projection_matching.hip \
//         triangulation-in-deformable-scenes_amd/csrc/matching.hip -o window_search_asan
//   ./window_search_asan
// The scene: a 16 x 12 grid over 320 x 240 pixels.  The current frame has 120 keypoints within 7 pixels of
// (100, 100) (more than 64 candidates in one window), one at x = 315 (the last half cell: in no cell), a few
// scattered ones and nothing else, so most cells are empty.  The queries sit on the cluster, on the scattered
// keypoints and in empty corners; each matcher runs once with small windows and once with a window wider than the
// image, which leaves the grid on all four sides.  A fifth of the slots is occupied.  It runs the calls with and
// without their optional outputs and the three octave errors, and ends with "clean" unless a sanitizer stopped it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../triangulation-in-deformable-scenes_amd/csrc/matching.h"
#include "../triangulation-in-deformable-scenes_amd/csrc/projection_matching.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

static int fail(const char *what, int rc, const std::string &err) {
    std::fprintf(stderr, "%s: %d %s\n", what, rc, err.c_str());
    return 1;
}

int main() {
    const deftri_feature_grid grid{16, 12, 0.0f, 0.0f, 320.0f, 240.0f, 8, 1.2f};
    const int32_t n_cluster = 120, n2 = n_cluster + 9, n = 24;
    uint32_t seed = 5;
    // ---- the current frame ----
    std::unique_ptr<float[]> uv2(new float[2 * n2]);
    std::unique_ptr<int32_t[]> oct2(new int32_t[n2]), slot(new int32_t[n2]);
    std::unique_ptr<uint8_t[]> d2(new uint8_t[32 * n2]);
    const float scattered[9][2] = {{315.0f, 100.0f}, {5.0f, 5.0f}, {309.0f, 5.0f}, {5.0f, 229.0f}, {309.0f, 229.0f},
                                   {160.0f, 120.0f}, {162.0f, 121.0f}, {220.0f, 60.0f}, {40.0f, 200.0f}};
    for (int32_t j = 0; j < n2; j++) {
        if (j < n_cluster) { uv2[2 * j] = 100.0f + 0.5f * (float)(j % 9); uv2[2 * j + 1] = 100.0f + 0.5f * (float)(j / 9); }
        else { uv2[2 * j] = scattered[j - n_cluster][0]; uv2[2 * j + 1] = scattered[j - n_cluster][1]; }
        oct2[j] = j % 3;
        std::memset(d2.get() + 32 * j, (j % 4) * 31, 32);            // four families ...
        for (int b = 0; b < (int)(lcg(seed) % 10); b++) d2[32 * j + lcg(seed) % 32] ^= (uint8_t)(1u << (lcg(seed) % 8));   // ... a few bits apart
    }
    // ---- the queries: pixels, and map points that project onto them through an identity pose ----
    const float kb8[8] = {200.0f, 200.0f, 160.0f, 120.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    std::unique_ptr<float[]> uv1(new float[2 * n]), pos(new float[3 * n]), normal(new float[3 * n]), dmin(new float[n]), dmax(new float[n]);
    std::unique_ptr<float[]> Tcw(new float[12]), k8(new float[8]);
    std::unique_ptr<int32_t[]> oct1(new int32_t[n]), oct_map(new int32_t[n]);
    std::unique_ptr<uint8_t[]> d1(new uint8_t[32 * n]), has(new uint8_t[n]);
    const float I34[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::memcpy(Tcw.get(), I34, sizeof(I34));
    std::memcpy(k8.get(), kb8, sizeof(kb8));
    for (int32_t i = 0; i < n; i++) {
        float u, v;
        if (i < 12) { u = 100.0f + 0.4f * (float)i; v = 101.0f + 0.3f * (float)i; }            // on the cluster
        else if (i < 12 + 9) { u = scattered[i - 12][0] + 0.5f; v = scattered[i - 12][1] - 0.5f; }
        else { u = 30.0f + 90.0f * (float)(i - 21); v = 170.0f; }                                // empty cells
        uv1[2 * i] = u; uv1[2 * i + 1] = v;
        oct1[i] = i % 5 == 4 ? 1 : 0;                              // match_for_initialization passes octave 1 over
        oct_map[i] = i % 4;                                        // the current frame has octaves 0 .. 2
        has[i] = i % 6 != 5;
        std::memset(d1.get() + 32 * i, (i % 4) * 31, 32);
        d1[32 * i + i % 32] ^= 0x11;
        // KannalaBrandt8 without distortion: r = theta, so the ray of pixel (u, v) has theta = |((u - cx) / fx, (v - cy) / fy)|
        const float a = (u - kb8[2]) / kb8[0], b = (v - kb8[3]) / kb8[1], theta = std::sqrt(a * a + b * b), depth = 2.0f + 0.1f * (float)i;
        const float s = theta > 0.0f ? std::sin(theta) / theta : 1.0f;
        const float ray[3] = {s * a, s * b, std::cos(theta)};
        for (int c = 0; c < 3; c++) { pos[3 * i + c] = depth * ray[c]; normal[3 * i + c] = ray[c]; }
        dmin[i] = 0.5f * depth;
        dmax[i] = depth * (1.0f + 0.3f * (float)(i % 4));          // predicted octaves 0 .. 4
    }
    std::unique_ptr<int32_t[]> match(new int32_t[n]), best(new int32_t[n]), second(new int32_t[n]), pred(new int32_t[n]);
    std::unique_ptr<uint8_t[]> status(new uint8_t[n]);
    std::unique_ptr<float[]> uv_out(new float[2 * n]), view_cos(new float[n]);
    std::string err;
    auto in_range = [&](const char *what) {
        for (int32_t i = 0; i < n; i++)
            if (match[i] < -1 || match[i] >= n2 || match[i] == n_cluster) {   // keypoint n_cluster is the one in no cell
                std::fprintf(stderr, "%s: match %d of query %d is no candidate\n", what, match[i], i);
                return false;
            }
        return true;
    };

    // ---- match_for_initialization: a window of 8 pixels, then one wider than the image ----
    for (float window : {8.0f, 400.0f}) {
        int32_t n_matches = -1;
        int rc = deftri::match_for_initialization(-1, nullptr, grid, n, uv1.get(), oct1.get(), d1.get(), n2, uv2.get(), oct2.get(),
                                                  d2.get(), 100, window, match.get(), best.get(), second.get(), &n_matches, err);
        if (rc) return fail("match_for_initialization", rc, err);
        int held = 0;
        for (int32_t i = 0; i < n; i++) held += match[i] >= 0;
        if (!in_range("match_for_initialization") || held != n_matches) return fail("match_for_initialization: inconsistent", 0, err);
        // the wide window holds every in-grid keypoint of octave 0 or 1, so every searched query has a best distance
        for (int32_t i = 0; window > 300.0f && i < n; i++)
            if ((best[i] == 255) != (oct1[i] > 0)) return fail("match_for_initialization: a wide window without a candidate", 0, err);
        std::printf("match_for_initialization, window %g: %d matches\n", window, n_matches);
        rc = deftri::match_for_initialization(-1, nullptr, grid, n, uv1.get(), oct1.get(), d1.get(), n2, uv2.get(), oct2.get(), d2.get(),
                                              100, window, match.get(), nullptr, nullptr, &n_matches, err);
        if (rc) return fail("match_for_initialization, required outputs only", rc, err);
    }

    // ---- projection_match: search, guided (small and wide windows) and fuse ----
    deftri_projection_report rep{};
    deftri::ProjectionMatchArgs a{};
    a.grid = &grid; a.Tcw = Tcw.get(); a.kb8 = k8.get();
    a.n2 = n2; a.uv2 = uv2.get(); a.octave2 = oct2.get(); a.desc2 = d2.get(); a.slot_point = slot.get();
    a.n = n; a.pos = pos.get(); a.desc = d1.get(); a.th = 100;
    a.normal = normal.get(); a.min_dist = dmin.get(); a.max_dist = dmax.get();
    a.has_point = has.get(); a.octave1 = oct_map.get(); a.window_size_factor = 1;
    a.match = match.get(); a.status = status.get();
    struct Mode { const char *name; bool guided, fuse; int32_t window; };
    const Mode modes[] = {{"search_with_projection", false, false, 1}, {"guided_matching", true, false, 1},
                          {"guided_matching, wide", true, false, 30}, {"fuse_search", true, true, 1}};
    for (const Mode &m : modes)
        for (int optional = 1; optional >= 0; optional--) {
            a.guided = m.guided; a.fuse = m.fuse; a.window_size_factor = m.window;
            a.slot_point = m.fuse ? nullptr : slot.get();
            for (int32_t j = 0; j < n2; j++) slot[j] = j % 5 == 2 ? 1000 + j : -1;     // a fifth is occupied
            a.uv = optional ? uv_out.get() : nullptr; a.view_cos = optional ? view_cos.get() : nullptr;
            a.predicted_octave = optional ? pred.get() : nullptr;
            a.best = optional ? best.get() : nullptr; a.second = optional ? second.get() : nullptr;
            a.report = optional ? &rep : nullptr;
            const int rc = deftri::projection_match(-1, nullptr, a, err);
            if (rc) return fail(m.name, rc, err);
            if (!in_range(m.name)) return 1;
            int counts[7] = {0, 0, 0, 0, 0, 0, 0};
            for (int32_t i = 0; i < n; i++) {
                if (status[i] > 6) return fail("status out of range", status[i], m.name);
                counts[status[i]]++;
                // searchWithProjection keeps the occupied slots (guidedMatching clears them first); a claimed slot names its point
                if (match[i] >= 0 && !m.fuse && slot[match[i]] != i) return fail("a match without its slot", i, m.name);
                if (match[i] >= 0 && !m.guided && match[i] % 5 == 2) return fail("a match into an occupied slot", i, m.name);
            }
            if (optional)
                std::printf("%s: matched %d, view cos %d, distance %d, no candidates %d, rejected %d, undefined %d, empty %d\n", m.name,
                            counts[0], counts[1], counts[2], counts[3], counts[4], counts[5], counts[6]);
            // a window wider than the image holds the whole frame: no considered point is without candidates
            if (m.window > 1 && counts[3] != 0) return fail("a wide window without a candidate", counts[3], m.name);
        }

    // ---- the three octave errors ----
    int32_t n_matches = 0;
    oct1[3] = 8;
    int rc = deftri::match_for_initialization(-1, nullptr, grid, n, uv1.get(), oct1.get(), d1.get(), n2, uv2.get(), oct2.get(), d2.get(),
                                              100, 8.0f, match.get(), nullptr, nullptr, &n_matches, err);
    if (rc != DEFTRI_E_ARG || err != "match_for_initialization: reference keypoint 3 has octave 8, outside [0, nScales = 8)")
        return fail("expected the reference keypoint's octave error", rc, err);
    std::printf("%s\n", err.c_str());
    oct1[3] = 0;
    oct2[7] = -1;
    a.guided = false; a.fuse = false; a.slot_point = slot.get();
    rc = deftri::projection_match(-1, nullptr, a, err);
    if (rc != DEFTRI_E_ARG || err != "search_with_projection: current keypoint 7 has octave -1, outside [0, nScales = 8)")
        return fail("expected the current keypoint's octave error", rc, err);
    std::printf("%s\n", err.c_str());
    oct2[7] = 1;
    oct_map[4] = 9;                                                  // has[4] is set; has[5] is not and its octave is not read
    oct_map[5] = 99;
    a.guided = true; a.fuse = true; a.slot_point = nullptr;
    rc = deftri::projection_match(-1, nullptr, a, err);
    if (rc != DEFTRI_E_ARG || err != "fuse_search: map point 4 has octave 9, outside [0, nScales = 8)")
        return fail("expected the map point's octave error", rc, err);
    std::printf("%s\nclean\n", err.c_str());
    return 0;
}
