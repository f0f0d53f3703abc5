"""The C++ adapter's open3DArap branch: deformationOptimization with Optimization.selection "open3DArap" through
adapter/test/open3d_arap_driver.cc moves keyframe 2's points to the Python path's result, bit for bit.  The
adapter's context needs a device, so the comparison is a GPU test; the build is not."""
import copy
import subprocess

import numpy as np
import pytest

import arap_deform_cases as cases
from adapter_io import read_state, write_map
from conftest import ROOT
from deftri import optimization
from deftri.settings import Settings

ADAPTER = ROOT / "adapter"
GOLDEN = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    prebuilt = ADAPTER / "build" / "open3d_arap_driver"
    if prebuilt.exists():
        return prebuilt
    out = tmp_path_factory.mktemp("adapter")
    subprocess.run(["make", "-s", "-C", str(ADAPTER), f"OBJDIR={out}"], check=True)
    return out / "open3d_arap_driver"


def _settings_text(tmp_path):
    over = {"Optimization.selection": '"open3DArap"', "Optimization.numberOfOptimizations": "2",
            "Measurements.DepthWeight": "3.0", "Experiment.Filepath": f'"{tmp_path / "Experiment.txt"}"'}
    out = []
    for line in (GOLDEN / "sim_default" / "settings.yaml").read_text().splitlines():
        k = line.split(":", 1)[0].strip()
        out.append(f"{k}: {over.pop(k)}" if k in over else line)
    out += [f"{k}: {v}" for k, v in over.items()]
    return "\n".join(out) + "\n"


def test_the_driver_builds_with_werror(driver):
    assert driver.exists()


@pytest.mark.gpu
def test_open3d_arap_through_the_adapter_equals_the_python_path(driver, tmp_path):
    m = cases.two_view_map()
    m0 = copy.deepcopy(m)
    (tmp_path / "s.yaml").write_text(_settings_text(tmp_path))
    st = Settings(path=tmp_path / "s.yaml")
    assert st.selection == "open3DArap" and st.n_optimizations == 2
    write_map(tmp_path / "m.bin", m0)
    rounds = optimization.deformationOptimization(m, st)
    assert [r["round"] for r in rounds] == [1, 2]
    r = subprocess.run([str(driver), str(tmp_path / "m.bin"), str(tmp_path / "o.bin"), str(tmp_path / "s.yaml")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    s = read_state(tmp_path / "o.bin")
    moved = 0
    for pid, mp in m.map_points.items():
        assert np.array_equal(s["points"][pid], mp.position), pid
        moved += int(not np.array_equal(mp.position, m0.map_points[pid].position))
    assert moved > 0
    assert s["extra"][0] == len(rounds) + 1                      # one visualizer update per round and the final one
