// triangulation_matching.h — searchForTriangulation (Modules/Matching/DescriptorMatching.cc:255-328): the
// correspondences between two keyframes' keypoints that hold no map point yet, what deftri_triangulate is
// fed with: triangulation_matching.hip.  (fuse, :330-428, searches with the projection matchers' kernel and
// lives in projection_matching.hip.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/deftri.h"

namespace deftri {

// The arguments of deftri_search_for_triangulation, already checked for null required pointers and
// negative sizes by the caller.  best_dist and report may be null.
struct TriangulationMatchArgs {
    int32_t n1;
    const float *uv1;
    const uint8_t *desc1, *has_point1;
    int32_t n2;
    const float *uv2;
    const uint8_t *desc2, *has_point2;
    const float *kb8, *E;
    int32_t th;
    float epipolar_th;
    int32_t flag_quirk;
    int32_t *matches, *best_dist;
    uint8_t *status;
    int32_t *n_matches;
    deftri_triangulation_match_report *report;
};

// device < 0: the reference's loop over all n1 x n2 pairs; else the ray and candidate kernels on `st`, one
// download, and the loop over the rows' compact candidate lists (deftri.h)
int search_for_triangulation(int device, hipStream_t st, const TriangulationMatchArgs &a, std::string &err);

}  // namespace deftri
