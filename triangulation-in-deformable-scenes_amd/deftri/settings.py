"""Settings — the solver-relevant subset of the reference's cv::FileStorage YAML reader
(Modules/System/Settings.cc:27-190).  Missing numeric keys read as 0 (as cv::FileNode does),
missing strings as "".  `validate_for_solver()` rejects the one value that makes the reference's
depth information infinite (Measurements.DepthWeight absent -> sigma_d = 0).
"""
import re

NUMERIC = {
    "Camera.fx": "fx", "Camera.fy": "fy", "Camera.cx": "cx", "Camera.cy": "cy",
    "Camera.d0": "k0", "Camera.d1": "k1", "Camera.d2": "k2", "Camera.d3": "k3",
    "Camera.cols": "cols", "Camera.rows": "rows",
    "FeatureExtractor.nScales": "n_scales", "FeatureExtractor.fScaleFactor": "scale_factor",
    "Camera.FirstPose.x": "c1x", "Camera.FirstPose.y": "c1y", "Camera.FirstPose.z": "c1z",
    "Camera.SecondPose.x": "c2x", "Camera.SecondPose.y": "c2y", "Camera.SecondPose.z": "c2z",
    "Keypoints.RepError": "rep_error", "Keypoints.decimalsApproximation": "decimals",
    "Measurements.DepthError": "depth_error", "Measurements.DepthWeight": "depth_weight",
    "Measurements.DepthScale.C1": "depth_scale_c1", "Measurements.DepthScale.C2": "depth_scale_c2",
    "Optimization.rep": "rep", "Optimization.arap": "arap", "Optimization.global": "global_",
    "Optimization.alpha": "alpha", "Optimization.beta": "beta",
    "Optimization.numberOfOptimizations": "n_optimizations",
    "Optimization.numberOfIterations": "n_iterations",
    "Optimization.nlopt.numberOfIterations": "nlopt_iterations",
    "Optimization.nlopt.relTolerance": "nlopt_rel_tol", "Optimization.nlopt.absTolerance": "nlopt_abs_tol",
    "Optimization.nlopt.rep.lowerBound": "nlopt_rep_lb", "Optimization.nlopt.rep.upperBound": "nlopt_rep_ub",
    "Optimization.nlopt.global.lowerBound": "nlopt_global_lb", "Optimization.nlopt.global.upperBound": "nlopt_global_ub",
    "Optimization.nlopt.arap.lowerBound": "nlopt_arap_lb", "Optimization.nlopt.arap.upperBound": "nlopt_arap_ub",
    "Triangulation.minCos": "min_cos", "Triangulation.depthLimit": "depth_limit",
    "FeatureGrid.nGridCols": "grid_cols", "FeatureGrid.nGridRows": "grid_rows",
    "FeatureExtractor.nFeatures": "n_features", "Epipolar.th": "epipolar_th",
    "Matching.initialization": "matching_init_th", "Matching.initialization.radius": "matching_init_radius",
    "Triangulation.minMatches": "min_matches",
}
STRINGS = {
    "Optimization.selection": "selection", "Optimization.weightsSelection": "weights_selection",
    "Triangulation.method": "trian_method", "Triangulation.seed.location": "trian_location",
    "Experiment.Filepath": "exp_file", "FeatureExtractor.imageBoderMask": "border_mask_path",
}


def parse_yaml_subset(text):
    out = {}
    for line in text.splitlines():
        line = line.split("#", 1)[0].strip()
        if not line or line.startswith("%") or ":" not in line:
            continue
        k, v = line.split(":", 1)
        v = v.strip()
        if v.startswith('"') and v.endswith('"'):
            v = v[1:-1]
        out[k.strip()] = v
    return out


class Settings:
    def __init__(self, text=None, path=None):
        if path is not None:
            with open(path) as f:
                text = f.read()
        kv = parse_yaml_subset(text or "")
        for key, attr in NUMERIC.items():
            v = kv.get(key)
            try:
                setattr(self, attr, float(v) if v is not None and re.match(r"^[-+0-9.eE]+$", v) else 0.0)
            except ValueError:
                setattr(self, attr, 0.0)
        for key, attr in STRINGS.items():
            setattr(self, attr, kv.get(key, ""))
        # Triangulation.checks: true only for the string "true" (Settings.cc:101-108)
        self.trian_checks = kv.get("Triangulation.checks", "") == "true"
        # Camera.k1 present: the reference undistorts keys and image bounds with OpenCV (Settings.cc:54-66)
        self.has_distortion = "Camera.k1" in kv
        # vDistortion_ (Settings.cc:54-67): Camera.k1, k2, p1, p2 and, only where Camera.k3 is present, k3 — float32,
        # empty without Camera.k1.  Not the attributes k0..k3 above, which are Camera.d0..d3 (the KB8 coefficients).
        import numpy as np
        names = ["Camera.k1", "Camera.k2", "Camera.p1", "Camera.p2"] + (["Camera.k3"] if "Camera.k3" in kv else [])
        self.distortion = np.array([self._number(kv.get(k)) for k in names] if self.has_distortion else [], np.float32)
        self.n_scales = int(self.n_scales)
        for attr in ("grid_cols", "grid_rows", "n_features", "matching_init_th"):     # ints in Settings.h
            setattr(self, attr, int(getattr(self, attr)))
        self.n_optimizations = int(self.n_optimizations)
        self.n_iterations = int(self.n_iterations)

    @staticmethod
    def _number(v):
        """A numeric node as the loop above reads it: 0 when missing or not a number."""
        try:
            return float(v) if v is not None and re.match(r"^[-+0-9.eE]+$", v) else 0.0
        except ValueError:
            return 0.0

    @property
    def depth_sigma(self):
        """SimulatedDepthErrorStanDesv = DepthWeight / 1000 (float), g2oBundleAdjustment.cc:449."""
        import numpy as np
        return np.float32(np.float32(self.depth_weight) / np.float32(1000.0))

    def validate_for_solver(self):
        if self.depth_weight == 0.0:
            raise ValueError("Measurements.DepthWeight is missing/0: depth information 1/sigma^2 would be "
                             "infinite (reference Settings.cc:124, g2oBundleAdjustment.cc:823-824)")
        return True
