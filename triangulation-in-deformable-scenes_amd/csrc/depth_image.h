// depth_image.h — the keyframes' depth images of a context (deftri_set_depth_images): resident copies
// (device memory on a device context), the per-keyframe sampled depth cache the graph builds and the
// image measurements read, and the measurements that need the images.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/deftri.h"

namespace deftri {

// the depth source of one keyframe (map order) for a graph build or measurement: raw != nullptr when
// the keyframe has an image — raw[o] = getDepthMeasure(kp_uv[o], true), meas[o] = (.., false), both
// NaN where status[o] != 0
struct DepthView {
    const double *raw = nullptr, *meas = nullptr;
    const uint8_t *status = nullptr;
    const float *ph = nullptr;       // the image's pinhole calibration fx fy cx cy
};

// a keyframe's depth image resident on the device (DepthImages::device_image)
struct DepthImageDev {
    const float *pixels = nullptr;
    int rows = 0, cols = 0;
    double scale = 1;
};

class DepthImages {
 public:
    DepthImages() = default;
    ~DepthImages() { clear(); }
    DepthImages(const DepthImages &) = delete;
    DepthImages &operator=(const DepthImages &) = delete;
    // device < 0: host-only (the same sampling function runs on the host)
    void bind(int device, hipStream_t st) { dev_ = device; st_ = st; }
    int set(int32_t n, const deftri_depth_image *images, std::string &err);
    bool any() const { return !imgs_.empty(); }
    int measure(int64_t kf_id, int32_t n, const float *uv, int scaled, double *depth, uint8_t *status, std::string &err);
    // the views of every keyframe of `map` (sampling the keyframes whose keypoints the cache does not
    // hold); valid until the next set() or views()
    int views(const deftri_map &map, std::vector<DepthView> &out, std::string &err);
    // the resident image of a keyframe on a device context, for kernels that sample it themselves
    // (k_init_depth_scales); false when the keyframe has no image or the context is host-only
    bool device_image(int64_t kf_id, const float **pixels, int32_t *rows, int32_t *cols, double *scale);
    int64_t uploads = 0, samplings = 0;

 private:
    struct Image {
        int64_t kf_id = 0;
        int32_t rows = 0, cols = 0;
        double scale = 1;
        float ph[4] = {1, 1, 0, 0};
        std::vector<float> host;      // host-only context
        float *dev = nullptr;         // device context
        // cache: the keypoints sampled last and their depths
        bool cached = false;
        std::vector<float> uv;
        std::vector<double> raw, meas;
        std::vector<uint8_t> status;
    };
    void clear();
    Image *find(int64_t kf_id);
    int sample(Image &im, int32_t n, const float *uv, int scaled, double *depth, uint8_t *status, std::string &err);
    int dev_ = -1;
    hipStream_t st_ = nullptr;
    std::vector<Image> imgs_;
};

// "keyframe <id> observation <o>: pixel (<u>, <v>) ..." for a used observation whose status is not 0
std::string depth_status_message(int64_t kf_id, int32_t obs, const float *uv, int status);

int measure_real_absolute(DepthImages &di, int device, hipStream_t st, const deftri_map &map, deftri_real_abs_errors *out,
                          std::string &err);
// measureRelativeMapErrors; di == nullptr: every depth from the per-index vector
int measure_relative(DepthImages *di, int device, hipStream_t st, const deftri_map &map, deftri_rel_errors *out,
                     int32_t max_pairs, int32_t *n_pairs, std::string &err);

}  // namespace deftri
