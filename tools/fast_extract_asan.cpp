// fast_extract_asan.cpp — the host loops of deftri_fast_extract (csrc/features.hip, a host-only context's
// path) under AddressSanitizer and UndefinedBehaviorSanitizer, on images held in heap blocks of exactly
// rows * cols bytes, so that a read past a cell's or a patch's edge is caught.  CPU only: device = -1, no
// GPU call is made.
//
// Build and run from the repository root (the scenes are those of tests/test_features.py):
//   python -c "import sys; sys.path.insert(0, 'tests'); import features_ref as fr; \
//              fr.make_scene(83, 97, 2)[0].tofile('s97.raw'); fr.make_scene(90, 200, 1)[0].tofile('s200.raw'); \
//              a, b = fr.make_scene(120, 160, 1, frame=16); a.tofile('s160.raw'); b.tofile('m160.raw')"
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wno-unused-value -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/fast_extract_asan.cpp \
//         triangulation-in-deformable-scenes_amd/csrc/features.hip -o fast_extract_asan
//   ./fast_extract_asan 83 97 1 1.2 400 300 s97.raw
//   ./fast_extract_asan 90 200 3 1.2 400 300 s200.raw
//   ./fast_extract_asan 120 160 2 1.2 400 300 s160.raw m160.raw
// Each run prints the report's counts (those test_features.py prints with -s) and ends with "clean" unless a
// sanitizer stopped it.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "../triangulation-in-deformable-scenes_amd/csrc/features.h"

static std::unique_ptr<uint8_t[]> read_exact(const char *path, size_t n) {
    std::unique_ptr<uint8_t[]> a(new uint8_t[n]);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(a.get(), 1, n, f) != n || std::fgetc(f) != EOF) {
        std::fprintf(stderr, "%s: not a file of %zu bytes\n", path, n);
        std::exit(2);
    }
    std::fclose(f);
    return a;
}

int main(int argc, char **argv) {
    if (argc != 8 && argc != 9) {
        std::fprintf(stderr, "usage: %s rows cols n_scales scale_factor n_max_features max_keys image.raw [mask.raw]\n", argv[0]);
        return 2;
    }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]);
    deftri_fast_params p{std::atoi(argv[3]), (float)std::atof(argv[4]), std::atoi(argv[5]), 10, 4, std::atoi(argv[6])};
    if (rows < 1 || cols < 1 || p.max_keys < 0) return 2;
    const size_t n = (size_t)rows * cols, cap = (size_t)p.max_keys;
    const auto image = read_exact(argv[7], n);
    const auto mask = argc == 9 ? read_exact(argv[8], n) : nullptr;
    std::unique_ptr<float[]> uv(new float[2 * cap]), angle(new float[cap]), response(new float[cap]), size(new float[cap]);
    std::unique_ptr<int32_t[]> octave(new int32_t[cap]);
    int32_t n_keys = 0;
    deftri_fast_report rep{};
    std::string err;
    const deftri::FastImage im{image.get(), rows, cols, cols}, bm{mask.get(), mask ? rows : 0, mask ? cols : 0, mask ? cols : 0};
    int rc = deftri::fast_extract(-1, nullptr, im, bm, p, uv.get(), octave.get(), angle.get(), response.get(), size.get(), &n_keys,
                                  &rep, err);
    if (rc) { std::fprintf(stderr, "fast_extract: %d %s\n", rc, err.c_str()); return 1; }
    std::printf("n_keys %d\n", n_keys);
    for (int l = 0; l < rep.n_levels; l++)
        std::printf("level %d %dx%d: candidates %d octree %d after_mask %d fallback %d empty %d truncated %d\n", l, rep.level_cols[l],
                    rep.level_rows[l], rep.n_candidates[l], rep.n_octree[l], rep.n_after_mask[l], rep.n_fallback_cells[l],
                    rep.n_empty_cells[l], rep.n_truncated[l]);
    // the debug stages and the mask reads at the image's corners, through the same buffers' edges
    for (int l = 0; l < rep.n_levels; l++) {
        std::unique_ptr<uint8_t[]> level(new uint8_t[(size_t)rep.level_rows[l] * rep.level_cols[l]]);
        int32_t r = 0, c = 0, nc = 0;
        rc = deftri::fast_pyramid_level(-1, nullptr, im, p, l, level.get(), &r, &c, err);
        const size_t nk = (size_t)rep.n_candidates[l];
        std::unique_ptr<int32_t[]> xy(new int32_t[2 * nk]);
        std::unique_ptr<float[]> resp(new float[nk]);
        if (!rc) rc = deftri::fast_candidates(-1, nullptr, im, p, l, (int32_t)nk, xy.get(), resp.get(), &nc, err);
        if (rc || r != rep.level_rows[l] || c != rep.level_cols[l] || nc != rep.n_candidates[l]) {
            std::fprintf(stderr, "stage %d: %d %s\n", l, rc, err.c_str());
            return 1;
        }
    }
    const int32_t corners[8] = {0, 0, cols - 1, 0, 0, rows - 1, cols - 1, rows - 1};
    uint8_t hit[4];
    for (int l = 0; l < 6; l++)
        if (deftri::fast_mask_reads(-1, nullptr, im, bm, l, 4, corners, hit, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
    std::printf("clean\n");
    return 0;
}
