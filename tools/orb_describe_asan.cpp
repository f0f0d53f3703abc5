// orb_describe_asan.cpp — the host loops of deftri_orb_describe (csrc/orb.hip, a host-only context's path)
// under AddressSanitizer and UndefinedBehaviorSanitizer, on images held in heap blocks of exactly rows * cols
// bytes and outputs of exactly n * 32 and n bytes, so that a read past a level's border or a write past a
// descriptor is caught.  CPU only: device = -1, no GPU call is made.  The images and the pattern are generated
// here (a fixed linear congruential sequence); the pattern's first four points are the patch's corners, which
// reach 21 pixels at 45 degrees.
//
// Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/orb_describe_asan.cpp \
//         triangulation-in-deformable-scenes_amd/csrc/orb.hip triangulation-in-deformable-scenes_amd/csrc/features.hip \
//         -o orb_describe_asan
//   ./orb_describe_asan
// It describes keypoints at every level's four corners (status 1), one and three pixels inside, at the centre and
// with non-finite coordinates and angles, on a 97 x 83 image with three levels, on the smallest legal image
// (20 x 20), on a 41 x 41 one whose second level is 20 x 20, and on a 24 x 20 one whose second level would be
// 20 x 17 (an argument error); it reads every level back through the debug stage and ends with "clean" unless
// a sanitizer stopped it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../triangulation-in-deformable-scenes_amd/csrc/orb.h"

static uint32_t lcg_state = 12345u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }

static int run(deftri::OrbState &S, int rows, int cols, int n_scales, float factor, bool expect_arg_error) {
    const size_t npx = (size_t)rows * cols;
    std::unique_ptr<uint8_t[]> image(new uint8_t[npx]);
    for (size_t i = 0; i < npx; i++) image[i] = (uint8_t)(lcg() >> 24);
    const deftri::FastImage im{image.get(), rows, cols, cols};
    const deftri_orb_params p{n_scales, factor};
    std::string err;
    std::vector<float> uv, angle;
    std::vector<int32_t> octave;
    auto key = [&](float x, float y, int l, float a) { uv.push_back(x); uv.push_back(y); octave.push_back(l); angle.push_back(a); };
    float scale = 1.0f;
    for (int l = 0; l < n_scales; l++) {
        if (l) scale *= factor;
        const int lc = (int)lrintf((float)cols * (1.0f / scale)), lr = (int)lrintf((float)rows * (1.0f / scale));
        for (int inset = 0; inset < 4; inset++) {
            const float x0 = (float)inset * scale, y0 = (float)inset * scale;
            const float x1 = (float)(lc - 1 - inset) * scale, y1 = (float)(lr - 1 - inset) * scale;
            for (float a : {0.0f, 45.0f, 135.0f, 359.99f}) { key(x0, y0, l, a); key(x1, y0, l, a); key(x0, y1, l, a); key(x1, y1, l, a); }
        }
        key((float)(lc / 2) * scale, (float)(lr / 2) * scale, l, 30.0f);
    }
    key(NAN, 3.0f, 0, 0.0f); key(3.0f, INFINITY, 0, 0.0f); key(3.0f, 3.0f, 0, NAN); key(-1e30f, 3e38f, 0, INFINITY);
    const size_t n = octave.size();
    std::unique_ptr<uint8_t[]> desc(new uint8_t[32 * n]), status(new uint8_t[n]);
    deftri_orb_report rep{};
    int rc = deftri::orb_describe(S, -1, nullptr, im, p, (int32_t)n, uv.data(), octave.data(), angle.data(), desc.get(), status.get(), &rep,
                                  err);
    if (expect_arg_error) {
        if (rc != DEFTRI_E_ARG) { std::fprintf(stderr, "%d x %d: expected an argument error, got %d\n", cols, rows, rc); return 1; }
        std::printf("%d x %d: %s\n", cols, rows, err.c_str());
        return 0;
    }
    if (rc) { std::fprintf(stderr, "orb_describe: %d %s\n", rc, err.c_str()); return 1; }
    size_t corners_outside = 0;
    for (size_t k = 0; k < n; k++) {
        bool any = false;
        for (int b = 0; b < 32; b++) any |= desc[32 * k + b] != 0;
        if (status[k] > 1 || (status[k] == 1 && any)) { std::fprintf(stderr, "keypoint %zu: status %d\n", k, status[k]); return 1; }
    }
    // the first 16 keypoints of every level stand on its corners; those at 45 and 135 degrees read 21 pixels out
    for (int l = 0, at = 0; l < n_scales; l++, at += 65)
        for (int k = 4; k < 12; k++) corners_outside += status[at + k];
    if (corners_outside != (size_t)8 * n_scales) { std::fprintf(stderr, "%zu corner keypoints outside\n", corners_outside); return 1; }
    std::printf("%d x %d: %zu keypoints, %d outside\n", cols, rows, n, rep.n_outside);
    for (int l = 0; l < rep.n_levels; l++) {
        std::unique_ptr<uint8_t[]> level(new uint8_t[(size_t)(rep.level_rows[l] + 38) * (rep.level_cols[l] + 38)]);
        int32_t r = 0, c = 0;
        rc = deftri::orb_pyramid_level(S, -1, nullptr, im, p, l, level.get(), &r, &c, err);
        if (rc || r != rep.level_rows[l] + 38 || c != rep.level_cols[l] + 38) { std::fprintf(stderr, "level %d: %d %s\n", l, rc, err.c_str()); return 1; }
        std::printf("  level %d: %d x %d\n", l, rep.level_cols[l], rep.level_rows[l]);
    }
    return 0;
}

int main() {
    deftri::OrbState S;
    std::string err;
    std::unique_ptr<int32_t[]> pattern(new int32_t[1024]);
    for (int i = 0; i < 1024; i++) pattern[i] = (int32_t)(lcg() >> 16) % 31 - 15;
    const int32_t corners[8] = {15, 15, -15, -15, 15, -15, -15, 15};
    for (int i = 0; i < 8; i++) pattern[i] = corners[i];
    if (deftri::orb_set_pattern(S, -1, nullptr, pattern.get(), err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    if (run(S, 83, 97, 3, 1.2f, false)) return 1;
    if (run(S, 20, 20, 1, 1.2f, false)) return 1;       // the smallest legal level
    if (run(S, 41, 41, 2, 2.0000002f, false)) return 1; // ... and as a second level: 41 -> 20
    if (run(S, 20, 24, 2, 1.2f, true)) return 1;        // 24 x 20 -> 20 x 17: refused
    std::printf("clean\n");
    return 0;
}
