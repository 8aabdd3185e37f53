"""Tile geometry of the headline plan (bench.py, BASELINE configs[1]: 1920 x 1080 full resolution, scaleFactor 1.1, minSize w/20 x
h/20, the calibrated cascade), built by the product's plan.cpp on the CPU through tests/geom/tile_geom_driver.cpp: the tiles fit
the LDS budget that keeps three tile workgroups resident per CU, and the plan stays the one the tile kernels are tuned for (every
stage on the tiles, no row strips, the largest scale on full-width tiles)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = os.path.join(ROOT, "tests", "geom")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def driver():
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    csrc = os.path.join(ROOT, "nubomedia-vca_amd", "csrc")
    out = os.path.join(GEOM, "build", "tile_geom_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(GEOM, "tile_geom_driver.cpp")] + [os.path.join(csrc, f) for f in ("cascade_xml.cpp", "plan.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = [CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
               "-I", os.path.join(ROOT, "include"), "-w"] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def plan(driver, tmp_path_factory, calibrated_xml):
    p = tmp_path_factory.mktemp("geom") / "face.xml"
    p.write_text(calibrated_xml)
    r = subprocess.run([driver, str(p), "1920", "1080", "1.1", "96", "54"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    return lines[0], lines[1:]


def test_tiles_fit_three_per_cu(plan):
    head, scales = plan
    assert head["tile_rows"] == 16 and head["tile_threads"] == 512 and head["tile_win"] == 32
    assert 3 * head["lds_budget"] <= LDS_PER_CU
    assert head["tile_lds"] <= head["lds_budget"]
    assert 3 * head["tile_lds"] <= LDS_PER_CU
    for s in scales:
        assert s["bytes"] <= head["lds_budget"], s
        assert s["tile"][1] <= head["tile_rows"] and s["tile"][0] <= head["tile_win"], s
        assert s["samples"][0] <= 256 and s["samples"][1] <= head["tile_threads"], s


def test_headline_plan_keeps_the_whole_cascade_on_tiles(plan):
    head, scales = plan
    # every scale tiled (no row strips) on tiles of at least 20 windows a side where the grid is that wide: the plan keeps every
    # stage on the tiles (no k_deep split, plan.cpp build_custom)
    assert head["strips"] == 0 and head["bands"] > 0
    assert head["deep_stage"] == head["stages"]
    assert len(scales) == 25
    for s in scales:
        assert s["tile"][0] >= min(20, s["windows"][0]), s
    # the scale with the most windows keeps full-width tiles
    big = max(scales, key=lambda s: s["windows"][0] * s["windows"][1])
    assert big["factor"] < 8 and big["tile"] == [32, 16], big
