"""Register budget of the tile kernels, from the code-object notes of the built library (numbers of the metadata only).

k_band and k_tile are launched with __launch_bounds__(kTileThreads, kTileWavesPerSimd): three 512-thread workgroups per CU are six
waves a SIMD, and six waves share the SIMD's 512 registers per lane only if each takes at most 80 (allocated in blocks of 8).
The band kernel sits right at that limit -- its spilled scalar registers live in lanes of vector registers -- so one register
more is a third of the residency gone, or a spill to scratch memory, without any test of results noticing."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
SIMD_VGPRS, VGPR_BLOCK = 512, 8


def _constant(name):
    txt = open(os.path.join(ROOT, "nubomedia-vca_amd", "csrc", "device_records.h")).read()
    return re.search(r"static constexpr int %s = ([^;]+);" % name, txt).group(1)


def waves_per_simd():
    threads = int(_constant("kTileWin")) * int(_constant("kTileRows"))          # kTileThreads = kTileSlots = kTileWin * kTileRows
    assert _constant("kTileThreads") == "kTileSlots" and _constant("kTileSlots") == "kTileWin * kTileRows"
    assert _constant("kTileWavesPerSimd") == "(kTilesPerCu * kTileThreads / 64 + 3) / 4"
    return (int(_constant("kTilesPerCu")) * threads // 64 + 3) // 4


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    """kernel name -> {note key: value} of kernels_cascade_tile.hip's gfx950 code object"""
    import __graft_entry__ as ge
    ge.build()
    obj = os.path.join(ROOT, "nubomedia-vca_amd", "build", "kernels_cascade_tile.hip.o")
    if not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("no LLVM tools")
    assert os.path.exists(obj), obj
    tmp = tmp_path_factory.mktemp("co")
    fb, co = str(tmp / "tile.fatbin"), str(tmp / "tile.co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, obj], check=True, capture_output=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fb, "--output=" + co], check=True, capture_output=True)
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for ln in out.splitlines():
        m = re.match(r"\s*-?\s*\.([a-z_]+):\s+(\S+)\s*$", ln)
        if not m:
            continue
        if m.group(1) == "agpr_count" or (cur is None and m.group(1) != "name"):          # a kernel's keys are sorted: .agpr_count opens its map, .name follows
            cur = {}
        if cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                kernels[m.group(2)] = cur
    return kernels


def _kernel(notes, name):
    hit = [v for k, v in notes.items() if re.fullmatch(r"_ZN4nvca\d+%sENS_11CascadeArgsE" % name, k)]
    assert len(hit) == 1, (name, sorted(notes))
    return hit[0]


def test_budget_is_80_registers():
    assert waves_per_simd() == 6 and SIMD_VGPRS // 6 // VGPR_BLOCK * VGPR_BLOCK == 80


@pytest.mark.parametrize("name", ["k_band", "k_tile"])
def test_tile_kernels_keep_their_registers(notes, name):
    k = _kernel(notes, name)
    budget = SIMD_VGPRS // waves_per_simd() // VGPR_BLOCK * VGPR_BLOCK
    print(name, {f: k[f] for f in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size")})
    assert int(k["private_segment_fixed_size"]) == 0 and k.get("uses_dynamic_stack", "false") == "false", k
    assert int(k["vgpr_spill_count"]) == 0, k
    assert int(k["vgpr_count"]) + int(k.get("agpr_count", 0)) <= budget, k
