// triangulation_matching_asan.cpp — the host loop of deftri_search_for_triangulation (csrc/triangulation_matching.hip,
// a host-only context's path) under AddressSanitizer and UndefinedBehaviorSanitizer, on a scene in heap blocks of
// exactly the sizes the entry documents, so that a read past a frame or a write past an output is caught.  CPU
// only: device = -1, no GPU call is made.
//
// Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/triangulation_matching_asan.cpp \
//         triangulation-in-deformable-scenes_amd/csrc/triangulation_matching.hip \
//         triangulation-in-deformable-scenes_amd/csrc/matching.hip -o triangulation_matching_asan
//   ./triangulation_matching_asan
// The scene: 97 x 133 keypoints (n2 > n1: vMatchedDistance and vnMatches21 are indexed by j), E = 0 and a wide
// threshold so that every pair passes the epipolar test, descriptors in a few families so that rows compete for
// keypoints and rob each other, a NaN pixel, occupied slots on both sides.  It runs both quirk modes, the call
// without its optional outputs, the empty frames and th = 256 (an argument error); it ends with "clean" unless a
// sanitizer stopped it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>

#include "../triangulation-in-deformable-scenes_amd/csrc/triangulation_matching.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

int main() {
    const int32_t n1 = 97, n2 = 133;
    uint32_t seed = 7;
    std::unique_ptr<float[]> uv1(new float[2 * n1]), uv2(new float[2 * n2]), kb8(new float[8]), E(new float[9]);
    std::unique_ptr<uint8_t[]> d1(new uint8_t[32 * n1]), d2(new uint8_t[32 * n2]), h1(new uint8_t[n1]), h2(new uint8_t[n2]);
    const float k[8] = {458.654f, 457.296f, 367.215f, 248.375f, -0.02f, 0.003f, 0.0f, 0.0f};
    std::memcpy(kb8.get(), k, sizeof(k));
    for (int i = 0; i < 9; i++) E[i] = 0.0f;
    auto fill = [&](int32_t n, float *uv, uint8_t *d, uint8_t *h, int every) {
        for (int32_t i = 0; i < n; i++) {
            uv[2 * i] = 100.0f + (float)(lcg(seed) % 500);
            uv[2 * i + 1] = 80.0f + (float)(lcg(seed) % 300);
            std::memset(d + 32 * i, (i % 5) * 17, 32);           // five families ...
            for (int b = 0; b < (int)(lcg(seed) % 12); b++) d[32 * i + lcg(seed) % 32] ^= (uint8_t)(1u << (lcg(seed) % 8));   // ... a few bits apart
            h[i] = i % every == every - 1;
        }
    };
    fill(n1, uv1.get(), d1.get(), h1.get(), 9);
    fill(n2, uv2.get(), d2.get(), h2.get(), 13);
    uv1[2 * 11] = std::numeric_limits<float>::quiet_NaN();

    std::unique_ptr<int32_t[]> matches(new int32_t[n1]), best(new int32_t[n1]);
    std::unique_ptr<uint8_t[]> status(new uint8_t[n1]);
    int32_t n_matches = 0;
    deftri_triangulation_match_report rep{};
    std::string err;
    deftri::TriangulationMatchArgs a{};
    a.n1 = n1; a.uv1 = uv1.get(); a.desc1 = d1.get(); a.has_point1 = h1.get();
    a.n2 = n2; a.uv2 = uv2.get(); a.desc2 = d2.get(); a.has_point2 = h2.get();
    a.kb8 = kb8.get(); a.E = E.get(); a.th = 50; a.epipolar_th = 0.01f;
    a.matches = matches.get(); a.best_dist = best.get(); a.status = status.get(); a.n_matches = &n_matches; a.report = &rep;
    for (int quirk = 1; quirk >= 0; quirk--) {
        a.flag_quirk = quirk;
        const int rc = deftri::search_for_triangulation(-1, nullptr, a, err);
        if (rc) { std::fprintf(stderr, "search_for_triangulation: %d %s\n", rc, err.c_str()); return 1; }
        int held = 0;
        for (int32_t i = 0; i < n1; i++) {
            if (matches[i] < -1 || matches[i] >= n2) { std::fprintf(stderr, "match out of range\n"); return 1; }
            held += matches[i] >= 0;
        }
        std::printf("quirk %d: %d matches, %d occupied, %d unmatched, %d robbed, %d passed over, flag row %d\n", quirk, n_matches,
                    rep.n_occupied, rep.n_unmatched, rep.n_stolen, rep.n_flag_skipped, rep.flag_row);
        // row 11, the NaN pixel, never matches: status 2, or 4 once the flag is set
        if (held != n_matches || matches[11] != -1 || (status[11] != 2 && status[11] != 4)) { std::fprintf(stderr, "inconsistent result\n"); return 1; }
    }
    a.best_dist = nullptr; a.report = nullptr;                   // only the required outputs
    int rc = deftri::search_for_triangulation(-1, nullptr, a, err);
    if (rc) { std::fprintf(stderr, "required outputs only: %d %s\n", rc, err.c_str()); return 1; }
    std::unique_ptr<float[]> none(new float[1]);
    std::unique_ptr<uint8_t[]> none8(new uint8_t[1]);
    deftri::TriangulationMatchArgs e = a;                        // an empty frame 2, then an empty frame 1
    e.n2 = 0; e.uv2 = none.get(); e.desc2 = none8.get(); e.has_point2 = none8.get();
    rc = deftri::search_for_triangulation(-1, nullptr, e, err);
    if (rc || n_matches != 0) { std::fprintf(stderr, "empty frame 2: %d %s\n", rc, err.c_str()); return 1; }
    e = a;
    e.n1 = 0; e.uv1 = none.get(); e.desc1 = none8.get(); e.has_point1 = none8.get();
    std::unique_ptr<int32_t[]> m0(new int32_t[1]);
    e.matches = m0.get(); e.status = none8.get();
    rc = deftri::search_for_triangulation(-1, nullptr, e, err);
    if (rc || n_matches != 0) { std::fprintf(stderr, "empty frame 1: %d %s\n", rc, err.c_str()); return 1; }
    a.th = 256;
    rc = deftri::search_for_triangulation(-1, nullptr, a, err);
    if (rc != DEFTRI_E_ARG) { std::fprintf(stderr, "expected an argument error, got %d\n", rc); return 1; }
    std::printf("%s\nclean\n", err.c_str());
    return 0;
}
