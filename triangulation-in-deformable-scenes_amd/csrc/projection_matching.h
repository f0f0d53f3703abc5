// projection_matching.h — the two matchers that put map points into a frame's keypoint slots by
// projection (guidedMatching, Modules/Matching/DescriptorMatching.cc:101-162; searchWithProjection,
// :164-253) and what searchWithProjection reads of a map point (Map::updateOrientationAndDescriptor,
// Map.cc:270-321): projection_matching.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/deftri.h"

namespace deftri {

// The arguments of deftri_search_with_projection (guided == false) and deftri_guided_matching (guided ==
// true; fuse == true on top of it: deftri_fuse_search, DescriptorMatching.cc:330-428), already checked for null required pointers by the callers.  The per-point outputs other than
// match may be null.
struct ProjectionMatchArgs {
    bool guided;
    bool fuse;                     // the search of fuse: guided's inputs (has_point: consider), no slots, one round
    const deftri_feature_grid *grid;
    const float *Tcw, *kb8;
    int32_t n2;
    const float *uv2;
    const int32_t *octave2;
    const uint8_t *desc2;
    int32_t *slot_point;           // searchWithProjection: in and out; guidedMatching: out; fuse: null
    int32_t n;
    const float *pos;
    const uint8_t *desc;
    int32_t th;
    // searchWithProjection
    const float *normal, *min_dist, *max_dist;
    // guidedMatching
    const uint8_t *has_point;
    const int32_t *octave1;
    int32_t window_size_factor;
    // outputs
    int32_t *match;
    uint8_t *status;
    float *uv, *view_cos;
    int32_t *predicted_octave, *best, *second;
    deftri_projection_report *report;
};

// device < 0: the reference's sequential loop; else the kernels on `st` (claims resolved in rounds, see
// deftri.h)
int projection_match(int device, hipStream_t st, const ProjectionMatchArgs &a, std::string &err);

// deftri_map_point_descriptors; device < 0: the sequential loop, else one wave per map point
int map_point_descriptors(int device, hipStream_t st, int32_t n, const float *pos, const int32_t *obs_start, const int32_t *obs_kf,
                          const int32_t *obs_slot, int32_t n_kf, const float *kf_Tcw, const int32_t *kf_slot_start,
                          const uint8_t *kf_desc, const int32_t *kf_octave, int32_t n_scales, float scale_factor, float *normal,
                          float *max_dist, float *min_dist, uint8_t *desc, int32_t *ref_obs, uint8_t *status, std::string &err);

}  // namespace deftri
