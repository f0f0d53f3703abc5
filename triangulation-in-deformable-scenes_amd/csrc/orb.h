// orb.h — ORB::describe (reference Modules/Features/ORB.cc:20-90, ORB.h:34-68) on an 8-bit image: the
// blurred, bordered pyramid and the 256 rotated comparisons per keypoint (orb.hip).  The sampling pattern
// comes from the caller and lives on the context.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/deftri.h"
#include "features.h"

namespace deftri {

// what a context keeps between calls: the pattern (host and device copy), the device arena of the calls,
// which only grows, and the events of the stage times
struct OrbState {
    int8_t pattern[1024] = {};
    bool have_pattern = false;
    int8_t *d_pattern = nullptr;
    char *d_arena = nullptr;
    size_t arena_size = 0;
    hipEvent_t ev[3] = {};
    OrbState() = default;
    OrbState(const OrbState &) = delete;
    OrbState &operator=(const OrbState &) = delete;
    ~OrbState();
};

// device < 0: host only; else the pattern is also copied to the device (on `st`, waited for)
int orb_set_pattern(OrbState &S, int device, hipStream_t st, const int32_t *xy, std::string &err);
// device < 0: the sequential host loops; else the kernels on `st`.  The arguments are those of the C
// entry, already checked for null pointers by the caller.
int orb_describe(OrbState &S, int device, hipStream_t st, const FastImage &image, const deftri_orb_params &p, int32_t n,
                 const float *uv, const int32_t *octave, const float *angle, uint8_t *desc, uint8_t *status,
                 deftri_orb_report *report, std::string &err);
// one level with its border, packed: out [(level rows + 38) * (level cols + 38)]
int orb_pyramid_level(OrbState &S, int device, hipStream_t st, const FastImage &image, const deftri_orb_params &p, int32_t level,
                      uint8_t *out, int32_t *out_rows, int32_t *out_cols, std::string &err);
// the integer 1-D kernel of the blur, computed from its definition: k [7]
void orb_blur_kernel(int32_t *k);

}  // namespace deftri
