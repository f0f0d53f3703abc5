// delaunay_dev.h — the Delaunay mesh built star by star (delaunay_star.h): on the device, one wave per point,
// or on the host with the exact predicates (delaunay_dev.hip).  The result is delaunay2d's on every input.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/deftri.h"

namespace deftri {

// the device buffers and the pinned staging of the star path, kept across calls (grow-only) on the context
class DelaunayDevice {
 public:
    DelaunayDevice(int device, hipStream_t st) : dev_(device), st_(st) {}
    ~DelaunayDevice();
    DelaunayDevice(const DelaunayDevice &) = delete;
    DelaunayDevice &operator=(const DelaunayDevice &) = delete;

 private:
    friend int delaunay_stars(DelaunayDevice *, int32_t, const double *, std::vector<int32_t> &, deftri_delaunay_report &,
                              std::string &);
    bool reserve(size_t dev_bytes, size_t pin_bytes);
    int dev_;
    hipStream_t st_;
    char *buf_ = nullptr, *pin_ = nullptr;
    size_t cap_ = 0, pin_cap_ = 0;
    hipEvent_t ev_[3] = {nullptr, nullptr, nullptr};
    std::mutex mu_;              // the graph builder triangulates its keyframes on parallel host threads
};

// The triangulation of xy [2 * n] (finite coordinates) into tris, canonical, and *rep.  dd == nullptr: every star
// on the host with the exact predicates.  Returns 0; DEFTRI_E_GRAPH when no triangle exists (n < 3, collinear; rep
// is written); DEFTRI_E_HIP with err.
int delaunay_stars(DelaunayDevice *dd, int32_t n, const double *xy, std::vector<int32_t> &tris, deftri_delaunay_report &rep,
                   std::string &err);

}  // namespace deftri
