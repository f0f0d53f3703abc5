"""From an image to keypoints, their descriptors and the frame's grid: Mapping::extractFeatures' three lines
(reference Modules/Mapping/Mapping.cc:120-129).

FAST::extract (Modules/Features/FAST.cc:81-118) through deftri_fast_extract — the pyramid, cv::FAST per cell,
distributeOctTree, the reflection / border mask and IC_Angle — and ORB::describe (Modules/Features/
ORB.cc:20-90) through deftri_orb_describe — the blurred, bordered pyramid and the 256 rotated comparisons per
keypoint — and Frame::distributeFeatures (Modules/Mapping/Frame.cc:188-211) through deftri_distribute_features —
cv::undistortPoints of the keypoints under Camera.k1, k2, p1, p2[, k3] and the grid over the undistorted image
bounds — on the device of the context or as sequential host loops on a host-only one.

The settings map as Mapping's constructor passes them (Mapping.cc:46): 2 * FeatureExtractor.nFeatures wanted,
thresholds 10 and 4, and the frame's vKeys capacity nFeatures (Frame.cc:35).  FeatureExtractor.imageBoderMask
names an image file; there is no image decoder here, so the caller reads it (Settings.border_mask_path) and
passes the pixels.

The 256 x 4 sampling table of ORB::describe exists only as the reference's program text (ORB.h:70-328) and is
not part of this library: describe() takes it from the caller, who passes the 512 points of their own copy
of the reference.
"""
import numpy as np

TH_FAST, MIN_TH_FAST = 10, 4            # Mapping.cc:46


def fast_params(settings, max_keys=None):
    """deftri_fast_params' fields from a Settings, as a dict (Context.fast_extract takes it)."""
    n = int(settings.n_features)
    return {"n_scales": int(settings.n_scales), "scale_factor": float(settings.scale_factor), "n_max_features": 2 * n,
            "th_fast": TH_FAST, "min_th_fast": MIN_TH_FAST, "max_keys": n if max_keys is None else int(max_keys)}


def orb_params(settings):
    """deftri_orb_params' fields from a Settings, as a dict (Context.orb_describe takes it): the ORB object is
    built with the extractor's nScales and fScaleFactor (Mapping.cc:46)."""
    return {"n_scales": int(settings.n_scales), "scale_factor": float(settings.scale_factor)}


def extract(ctx, image, settings, border_mask=None):
    """Mapping::extractFeatures' first half (Mapping.cc:120-129) for one 8-bit grey image: a capi.FastResult.
    FAST runs on the distorted image whatever Camera.k1 says, as in the reference: the result's uv are distorted
    pixels (vKeysDis_), which ORB::describe reads; distribute() undistorts them."""
    if settings.border_mask_path and border_mask is None:
        raise ValueError(f"FeatureExtractor.imageBoderMask names {settings.border_mask_path!r}: decode it and pass border_mask")
    return ctx.fast_extract(np.asarray(image), fast_params(settings), border_mask)


def distribute(ctx, keys, settings, n_slots=None):
    """Mapping::extractFeatures' third line, currFrame_.distributeFeatures() (Frame.cc:188-211), with the bounds
    Frame's constructor computes (:221-250), on `ctx`: `keys` (a capi.FastResult or float32 [n, 2] distorted pixels)
    are undistorted when Camera.k1 is set and copied when it is not, and every keypoint whose own posInGrid is true
    goes into its grid cell.  n_slots: the frame's capacity (FeatureExtractor.nFeatures in the reference); the slots
    behind the keypoints are zeros and are undistorted and distributed like any other, as the reference's loop over
    all of vKeysDis_ does.  Default: the keypoints alone.  Returns a capi.DistributedFeatures: the undistorted
    keys, the grid (what the matchers take) and the cell lists."""
    from . import matching
    uv = np.ascontiguousarray(keys.uv if hasattr(keys, "uv") else keys, np.float32).reshape(-1, 2)
    if n_slots is not None:
        if len(uv) > n_slots:
            raise ValueError(f"{len(uv)} keypoints for {n_slots} slots")
        uv = np.concatenate([uv, np.zeros((n_slots - len(uv), 2), np.float32)])
    calib, dist = matching.camera_of(settings, "distribute")
    return ctx.distribute_features(settings.grid_cols, settings.grid_rows, settings.n_scales, settings.scale_factor,
                                   int(settings.cols), int(settings.rows), calib, dist, uv)


def describe(ctx, image, keys, settings, pattern):
    """Mapping::extractFeatures' second half for the same image: ORB::describe of `keys`, a capi.FastResult or a
    tuple (uv, octave, angle).  pattern: the 512 sampling points as an int array of shape (512, 2) or
    (256, 4); there is no default.  Returns a capi.OrbResult."""
    if pattern is None:
        raise ValueError("pattern is required: the sampling table is not part of this library; pass the 512 points of "
                         "bit_pattern_31_ from your copy of the reference (Modules/Features/ORB.h) as an int array of "
                         "shape (512, 2) or (256, 4)")
    uv, octave, angle = (keys.uv, keys.octave, keys.angle) if hasattr(keys, "uv") else keys
    ctx.orb_set_pattern(pattern)
    return ctx.orb_describe(np.asarray(image), orb_params(settings), uv, octave, angle)
