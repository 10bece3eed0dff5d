"""Register budget of csrc/speed.hip: the plan kernel and both instantiations of the apply kernel
compile for gfx950 without a spilled register and without scratch memory (the variant records are
selected, never indexed, so no copy of them lands in private memory)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="needs hipcc")
def test_speed_kernels_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    rows = KR.analyse(os.path.join(ROOT, "deepspeech_amd", "csrc", "speed.hip"))
    names = [r["name"] for r in rows]
    assert sum("speed_plan_kernel" in n for n in names) == 1, names
    assert sum("speed_apply_kernel" in n for n in names) == 2, names          # fp32 and int16 input
    bad = [r["name"] for r in rows if r.get("VGPRs Spill", 0) or r.get("ScratchSize [bytes/lane]", 0)]
    assert not bad, bad
    for r in rows:
        print(r["name"], r.get("VGPRs"), r.get("Occupancy [waves/SIMD]"))
