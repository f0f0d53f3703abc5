// open3d_arap_driver — test harness only: deformationOptimization through the adapter on a map dumped by
// tests/adapter_io.py, with the settings file's Optimization.selection ("open3DArap": the rounds of
// arapOpen3DOptimization), and the map's state afterwards for the Python side to compare with
// deftri.optimization on the same map.
//
//   open3d_arap_driver <map.bin> <out.bin> <settings.yaml>
//
// Output: adapter_driver's layout ("DTOUT001"), extra = {visualizer updates}.
#include <cstdio>
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

}  // namespace

int main(int argc, char **argv) {
    if (argc < 4) {
        std::cerr << "usage: open3d_arap_driver map.bin out.bin settings.yaml" << std::endl;
        return 2;
    }
    MapDump d = read_map(argv[1]);
    Settings settings(argv[3]);
    auto viz = std::make_shared<MapVisualizer>(d.map);
    deformationOptimization(d.map, settings, viz);
    write_state(argv[2], d, {(double)viz->updates()});
    return 0;
}
