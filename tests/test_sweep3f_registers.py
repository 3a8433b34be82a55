"""Register budget of k_sweep3f, the fixed-shape instantiation of the trajectory engine, read from the built library's AMDGPU metadata (CPU only).

k_sweep3f carries the sequencer, the 128-row DMA streamers and the prefetchers only, with the block geometry as constants: it must need no
scratch, spill no VGPR, and be no worse than the headline instantiation it replaces, k_sweep3<uint16_t, false> (149 VGPRs, 17 SGPR spills)."""
import os

import pytest

from bwgr_amd import build as B
from test_sweep3_registers import TOOLS, kernel_metadata

NAME = "_ZN4bwgr9k_sweep3fENS_10Sweep3ArgsE"
MAX_VGPRS, MAX_SGPR_SPILLS = 149, 17


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    missing = [t for t, p in TOOLS.items() if not os.access(p, os.X_OK)]
    if missing:
        pytest.skip("ROCm LLVM tools missing: %s" % ", ".join(missing))
    if not os.path.exists(B.LIB):
        pytest.skip("libbwgr_hip.so is not built")
    return kernel_metadata(B.LIB, str(tmp_path_factory.mktemp("sweep3f_registers")))


def test_sweep3f_register_budget(metadata):
    assert NAME in metadata, sorted(k for k in metadata if "sweep3" in k)
    md = metadata[NAME]
    assert md["private_segment_fixed_size"] == 0, md   # no scratch
    assert md["vgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= MAX_VGPRS, md
    assert md["sgpr_spill_count"] <= MAX_SGPR_SPILLS, md
