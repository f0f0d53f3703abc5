// depth_image_driver — test harness only: a map dumped by tests/adapter_io.py plus the keyframes'
// depth images from a side file, driven through the adapter, for the Python side to compare with its
// own host mirror on the same map and images.
//
//   depth_image_driver <map.bin> <images.bin> <out.bin> lookup
//       KeyFrame::getDepthMeasure(x, y, true) and (x, y, false) of every keypoint of every keyframe
//       that has an image, in keyframe and keypoint order (the model's restatement; no GPU)
//   depth_image_driver <map.bin> <images.bin> <out.bin> arap <rep> <global> <arap> <depthError> <nIt>
//       arapOptimization with the depth measurements taken from the images
//
// images.bin (little-endian): "DTIMG001" | n i32 | per image: kf id i64, rows i32, cols i32,
// imageDepthScale f64, pixels[rows * cols] f32.  Output: adapter_driver's layout ("DTOUT001").
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <set>
#include <string>

#include "../test/map_io.h"
#include "Optimization/g2oBundleAdjustment.h"
#include "deftri_adapter.h"

namespace {

struct Writer {
    std::FILE *f;
    explicit Writer(const std::string &p) : f(std::fopen(p.c_str(), "wb")) {
        if (!f) throw std::runtime_error("cannot write " + p);
    }
    ~Writer() { std::fclose(f); }
    template <typename T>
    void put(const T &v) { std::fwrite(&v, sizeof(T), 1, f); }
    template <typename T>
    void put(const T *v, size_t n) { std::fwrite(v, sizeof(T), n, f); }
};

void write_state(const std::string &path, MapDump &d, const std::vector<double> &extra) {
    Writer w(path);
    w.put("DTOUT001", 8);
    w.put((int32_t)d.kfs.size());
    std::set<MapPoint *> present;
    for (auto &kf : d.kfs) {
        w.put((int64_t)kf->getId());
        w.put(kf->getEstimatedDepthScale());
        double p7[7];
        deftri_adapter::se3quat7(kf->getPose(), p7);
        w.put(p7, 7);
        for (auto &mp : kf->getMapPoints())
            if (mp) present.insert(mp.get());
    }
    w.put((int32_t)d.mps.size());
    for (auto &mp : d.mps) {
        w.put((int64_t)mp->getId());
        const Eigen::Vector3f p = mp->getWorldPosition();
        w.put(p.data(), 3);
        w.put((uint8_t)(present.count(mp.get()) ? 1 : 0));
    }
    double g[14] = {};
    if (d.kfs.size() >= 2) {
        deftri_adapter::se3quat7(d.map->getGlobalKeyFramesTransformation(0, 1), g);
        deftri_adapter::se3quat7(d.map->getGlobalKeyFramesTransformation(1, 0), g + 7);
    }
    w.put(g, 14);
    w.put((int32_t)extra.size());
    w.put(extra.data(), extra.size());
}

void read_images(const std::string &path, MapDump &d) {
    Reader r(path);
    const auto magic = r.vec<char>(8);
    if (std::string(magic.begin(), magic.end()) != "DTIMG001") throw std::runtime_error("not an image side file");
    const int32_t n = r.get<int32_t>();
    for (int i = 0; i < n; i++) {
        const int64_t id = r.get<int64_t>();
        const int32_t rows = r.get<int32_t>(), cols = r.get<int32_t>();
        const double scale = r.get<double>();
        const auto px = r.vec<float>((size_t)rows * cols);
        cv::Mat im(rows, cols, CV_32F);
        std::memcpy(im.ptr<float>(0), px.data(), sizeof(float) * px.size());
        d.map->getKeyFrame((ID)id)->setDepthIm(im, scale);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 5) {
        std::cerr << "usage: depth_image_driver map.bin images.bin out.bin mode [args]" << std::endl;
        return 2;
    }
    MapDump d = read_map(argv[1]);
    read_images(argv[2], d);
    const std::string mode = argv[4];
    std::vector<double> extra;
    if (mode == "lookup") {
        for (auto &kf : d.kfs) {
            if (kf->getDepthIm().empty()) continue;
            for (const cv::KeyPoint &kp : kf->getKeyPoints()) {
                extra.push_back(kf->getDepthMeasure(kp.pt.x, kp.pt.y));
                extra.push_back(kf->getDepthMeasure(kp.pt.x, kp.pt.y, false));
            }
        }
    } else if (mode == "arap") {
        if (argc < 10) return 2;
        double upd = -1.0;
        arapOptimization(d.map.get(), std::atof(argv[5]), std::atof(argv[6]), std::atof(argv[7]), 0.0, 0.0,
                         (float)std::atof(argv[8]), std::atoi(argv[9]), &upd);
        const deftri_report &r = deftri_adapter::last_report();
        int64_t uploads = 0, samplings = 0;
        if (deftri_ctx *ctx = deftri_adapter::context()) deftri_depth_image_stats(ctx, &uploads, &samplings);
        extra = {upd, r.chi2_initial, r.chi2_final, (double)r.iterations, (double)r.trials_total, (double)uploads,
                 (double)samplings};
    } else {
        std::cerr << "unknown mode " << mode << std::endl;
        return 2;
    }
    write_state(argv[3], d, extra);
    return 0;
}
