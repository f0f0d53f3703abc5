"""From an image to keypoints: FAST::extract (reference Modules/Features/FAST.cc:81-118) through
deftri_fast_extract — the pyramid, cv::FAST per cell, distributeOctTree, the reflection / border mask and
IC_Angle, on the device of the context or as sequential host loops on a host-only one.

The settings map as Mapping's constructor passes them (Mapping.cc:46): 2 * FeatureExtractor.nFeatures wanted,
thresholds 10 and 4, and the frame's vKeys capacity nFeatures (Frame.cc:35).  FeatureExtractor.imageBoderMask
names an image file; there is no image decoder here, so the caller reads it (Settings.border_mask_path) and
passes the pixels.  Descriptors (ORB::describe) are not computed: they remain the caller's.
"""
import numpy as np

TH_FAST, MIN_TH_FAST = 10, 4            # Mapping.cc:46


def fast_params(settings, max_keys=None):
    """deftri_fast_params' fields from a Settings, as a dict (Context.fast_extract takes it)."""
    n = int(settings.n_features)
    return {"n_scales": int(settings.n_scales), "scale_factor": float(settings.scale_factor), "n_max_features": 2 * n,
            "th_fast": TH_FAST, "min_th_fast": MIN_TH_FAST, "max_keys": n if max_keys is None else int(max_keys)}


def extract(ctx, image, settings, border_mask=None):
    """Mapping::extractFeatures' first half (Mapping.cc:120-129) for one 8-bit grey image: a capi.FastResult."""
    if settings.has_distortion:
        raise ValueError("Camera.k1 is set: the reference undistorts the keypoints with OpenCV, which is not restated")
    if settings.border_mask_path and border_mask is None:
        raise ValueError(f"FeatureExtractor.imageBoderMask names {settings.border_mask_path!r}: decode it and pass border_mask")
    return ctx.fast_extract(np.asarray(image), fast_params(settings), border_mask)
