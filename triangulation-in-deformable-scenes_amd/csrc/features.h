// features.h — FAST::extract (reference Modules/Features/FAST.cc:81-118) on an 8-bit image: the pyramid,
// cv::FAST per cell with the min_th_fast fallback, distributeOctTree, the reflection / border mask and
// IC_Angle (features.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/deftri.h"

namespace deftri {

// an 8-bit single-channel image; px == nullptr: none (the border mask may be absent)
struct FastImage {
    const uint8_t *px;
    int32_t rows, cols, stride;
};

// "<entry>: <why>" into err; the return value of an entry that refuses its arguments
inline int arg_fail(std::string &err, const char *entry, const std::string &why) {
    err = std::string(entry) + ": " + why;
    return DEFTRI_E_ARG;
}

// cvRound: round half to even
inline int cv_round(float v) { return (int)lrintf(v); }

// device < 0: the sequential host loops; else the kernels on `st`.  The arguments are those of the C
// entries, already checked for null pointers by the callers.  uv [max_keys * 2], the others [max_keys].
int fast_extract(int device, hipStream_t st, const FastImage &image, const FastImage &border_mask, const deftri_fast_params &p,
                 float *uv, int32_t *octave, float *angle, float *response, float *size, int32_t *n_keys,
                 deftri_fast_report *report, std::string &err);
// one pyramid level's pixels, packed: out [level rows * level cols] (at most rows * cols)
int fast_pyramid_level(int device, hipStream_t st, const FastImage &image, const deftri_fast_params &p, int32_t level,
                       uint8_t *out, int32_t *out_rows, int32_t *out_cols, std::string &err);
// one level's candidates in front of distributeOctTree, in the reference's order: xy relative to the
// 16-pixel border (vToDistributeKeys' pt), the first min(*n, max_cand) written
int fast_candidates(int device, hipStream_t st, const FastImage &image, const deftri_fast_params &p, int32_t level,
                    int32_t max_cand, int32_t *xy, float *response, int32_t *n, std::string &err);
// the reads of level `level`'s dilated mask at n positions xy (x, y) of the full-resolution image
int fast_mask_reads(int device, hipStream_t st, const FastImage &image, const FastImage &border_mask, int32_t level, int32_t n,
                    const int32_t *xy, uint8_t *hit, std::string &err);


// OpenCV's 8-bit fixed-point bilinear resize (deftri.h, deftri_fast_extract 2.), for the other pyramids
// built from it (orb.hip).  A Tap holds the two source indices of one destination index and their weights.
namespace dev {
struct Tap { int s0, s1, a0, a1; };
}
std::vector<dev::Tap> resize_taps(int src, int dst);
// dst [drows x dcols, packed] from src (row pitch spitch): one launch on `st` (xt, yt on the device) / the host loop
void resize_launch(hipStream_t st, const uint8_t *src, int spitch, uint8_t *dst, int dcols, int drows, const dev::Tap *xt,
                   const dev::Tap *yt);
void resize_host(const uint8_t *src, int spitch, uint8_t *dst, int dcols, int drows, const dev::Tap *xt, const dev::Tap *yt);

}  // namespace deftri
