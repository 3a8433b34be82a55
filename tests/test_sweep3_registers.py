"""Register budget of the k_sweep3 / k_sweep3p kernels, read from the AMDGPU metadata of the built library (CPU only).

Each kernel is one workgroup of 512 threads per compute unit whose waves run different roles.  The compiler
allocates registers for the union of the roles, so state that one role keeps live through another's code costs every wave: spilled SGPRs
live in VGPR lanes and are read back with v_readlane.  This test keeps the budget from creeping back: no scratch, the VGPRs at most
what the kernels had before the roles got loops of their own, and the SGPR spills at most what remains now."""
import os
import re
import shutil
import subprocess

import pytest

from bwgr_amd import build as B

LLVM = "/opt/rocm/llvm/bin"
TOOLS = {t: os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

# mangled name -> (max .vgpr_count, max .sgpr_spill_count).  The VGPR caps are the counts before the per-role loops (180 / 185 for the
# 16-bit Gram, 149 for the 32-bit one, the pair kernels 180 / 159); the spill caps are what is left after them (99 / 101 / 92 / 94 and
# 131 / 80 before).  A 512-thread workgroup needs at most 256 VGPRs to stay resident.
LIMITS = {
    "_ZN4bwgr8k_sweep3ItLb0EEEvNS_10Sweep3ArgsE": (180, 17),   # k_sweep3<uint16_t, false>: the headline
    "_ZN4bwgr8k_sweep3ItLb1EEEvNS_10Sweep3ArgsE": (185, 17),   # k_sweep3<uint16_t, true>: implicitly centred
    "_ZN4bwgr8k_sweep3IiLb0EEEvNS_10Sweep3ArgsE": (149, 17),
    "_ZN4bwgr8k_sweep3IiLb1EEEvNS_10Sweep3ArgsE": (149, 17),
    "_ZN4bwgr9k_sweep3pItEEvNS_10Sweep3ArgsES1_": (180, 18),   # k_sweep3p: two sequencers
    "_ZN4bwgr9k_sweep3pIiEEvNS_10Sweep3ArgsES1_": (159, 18),
}


def kernel_metadata(lib, workdir):
    """{kernel name: {field: int}} from the gfx950 code object inside lib's .hip_fatbin section."""
    fatbin, co = os.path.join(workdir, "fatbin.bin"), os.path.join(workdir, "gfx950.co")
    subprocess.run([TOOLS["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + fatbin, lib, os.path.join(workdir, "stripped.so")],
                   check=True, capture_output=True)
    subprocess.run([TOOLS["clang-offload-bundler"], "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fatbin, "--output=" + co],
                   check=True, capture_output=True)
    notes = subprocess.run([TOOLS["llvm-readelf"], "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for rec in re.split(r"\n  - ", notes):   # one item of amdhsa.kernels per chunk (the argument lists are indented deeper)
        name = re.search(r"\n    \.name:\s+(\S+)", rec)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\n    \.(\w+):\s+(\d+)\s*(?=\n)", rec)}
    return out


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    missing = [t for t, p in TOOLS.items() if not os.access(p, os.X_OK)]
    if missing:
        pytest.skip("ROCm LLVM tools missing: %s" % ", ".join(missing))
    if not os.path.exists(B.LIB):
        pytest.skip("libbwgr_hip.so is not built")
    return kernel_metadata(B.LIB, str(tmp_path_factory.mktemp("sweep3_registers")))


def test_metadata_is_readable(metadata):
    assert metadata, "no kernels in the gfx950 code object's notes"
    assert set(LIMITS) <= set(metadata), sorted(set(LIMITS) - set(metadata))


@pytest.mark.parametrize("name", sorted(LIMITS))
def test_sweep3_register_budget(metadata, name):
    md = metadata[name]
    vmax, smax = LIMITS[name]
    assert md["private_segment_fixed_size"] == 0, (name, md)   # no scratch
    assert md["vgpr_count"] <= vmax and md["vgpr_count"] <= 256, (name, md)
    assert md["sgpr_spill_count"] <= smax, (name, md)
    assert md["vgpr_spill_count"] == 0, (name, md)
