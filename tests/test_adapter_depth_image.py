"""The C++ adapter with real keyframes: the model's KeyFrame::getDepthMeasure(x, y, scaled) over a set
depth image equals the numpy restatement bit for bit (CPU), and arapOptimization through the adapter
— MapView registers the keyframes' images on the context — equals the Python mirror on the same map
and images bit for bit (GPU).  The images travel in a side file (adapter/test/depth_image_driver.cc)."""
import copy
import struct
import subprocess

import numpy as np
import pytest

from adapter_io import read_state, write_map
from conftest import ROOT
from deftri import sim
import depth_image_ref as ref

ADAPTER = ROOT / "adapter"
SIGMA = np.float32(0.003)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    prebuilt = ADAPTER / "build" / "depth_image_driver"
    if prebuilt.exists():
        return prebuilt
    out = tmp_path_factory.mktemp("adapter")
    subprocess.run(["make", "-s", "-C", str(ADAPTER), f"OBJDIR={out}"], check=True)
    return out / "depth_image_driver"


def write_images(path, m):
    kfs = [kf for kf in m.keyframes.values() if kf.depth_image is not None]
    out = [b"DTIMG001", struct.pack("<i", len(kfs))]
    for kf in kfs:
        rows, cols = kf.depth_image.shape
        out.append(struct.pack("<qiid", kf.id, rows, cols, float(kf.image_depth_scale)))
        out.append(np.ascontiguousarray(kf.depth_image, np.float32).tobytes())
    path.write_bytes(b"".join(out))


def _scene():
    m, _ = sim.simulate_two_view(n=300, seed=3)
    return ref.synthetic_images(m, (560, 640), seed=7)


def _run(exe, *args):
    r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def test_model_lookup_equals_the_restatement(driver, tmp_path):
    m = _scene()
    m.keyframes[0].keypoints[3] = [639.5, 100.25]        # the next-row spill
    write_map(tmp_path / "m.bin", m)
    write_images(tmp_path / "i.bin", m)
    _run(driver, tmp_path / "m.bin", tmp_path / "i.bin", tmp_path / "o.bin", "lookup")
    got = np.array(read_state(tmp_path / "o.bin")["extra"]).reshape(-1, 2)
    want = []
    for kf in m.keyframes.values():
        a, sa = ref.keyframe_depths(kf, True)
        b, sb = ref.keyframe_depths(kf, False)
        assert (sa == 0).all() and (sb == 0).all()
        want.append(np.column_stack([a, b]))
    want = np.concatenate(want)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


def test_model_without_an_image_still_throws(driver, tmp_path):
    m, _ = sim.simulate_two_view(n=50, seed=3)
    write_map(tmp_path / "m.bin", m)
    (tmp_path / "i.bin").write_bytes(b"DTIMG001" + struct.pack("<i", 0))
    _run(driver, tmp_path / "m.bin", tmp_path / "i.bin", tmp_path / "o.bin", "lookup")
    assert read_state(tmp_path / "o.bin")["extra"] == []


@pytest.mark.gpu
def test_arap_optimization_with_images_matches_host_mirror(driver, tmp_path):
    from deftri import optimization
    m = _scene()
    write_map(tmp_path / "m.bin", copy.deepcopy(m))
    write_images(tmp_path / "i.bin", m)
    upd = optimization.arapOptimization(m, 1.0, 50.0, 2e5, 0.0, 0.0, SIGMA, 5)
    _run(driver, tmp_path / "m.bin", tmp_path / "i.bin", tmp_path / "o.bin", "arap", "1", "50", "200000",
         repr(float(SIGMA)), "5")
    s = read_state(tmp_path / "o.bin")
    for pid, mp in m.map_points.items():
        assert np.array_equal(s["points"][pid], mp.position), pid
    for kid, kf in m.keyframes.items():
        assert s["keyframes"][kid]["depth_scale"] == kf.estimated_depth_scale
    assert s["extra"][0] == upd and upd > 0
    assert s["extra"][5:7] == [2.0, 2.0]                 # both images sent once, both keyframes sampled once
    assert np.array_equal(s["global01"], m.global_T[(0, 1)].as7())
    # the per-index depths give another result: the images were read
    plain = _scene()
    for kf in plain.keyframes.values():
        kf.set_depth_image(None)
    assert optimization.arapOptimization(plain, 1.0, 50.0, 2e5, 0.0, 0.0, SIGMA, 5) != upd
