// metrics.h — calculatePixelsStandDev of a map on the device (metrics.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/deftri.h"

namespace deftri {

// `map` already checked by the caller (deftri_pixels_stand_dev); a map without a matched pair launches
// nothing
int pixels_stand_dev(int device, hipStream_t st, const deftri_map &map, deftri_pixels_error *out, std::string &err);

}  // namespace deftri
