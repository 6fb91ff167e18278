"""CPU: the recording launch of several steps (auv_step_multi_record / k_step_record) exists in every layer, and its kernel keeps
the register budget the launch of several steps rests on (four waves per SIMD, nothing in scratch beyond k_step_multi's)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from gym_auv_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_library_header_and_binding_have_the_recording_call():
    if not os.path.exists(_capi.LIB_PATH):
        pytest.fail("libauv_hip.so not built: run __graft_entry__.build()")
    lib = _capi.load_library()
    assert hasattr(lib, "auv_step_multi_record")
    hdr = open(os.path.join(ROOT, "include", "auv_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+auv_step_multi_record\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/auv_hip.h does not declare auv_step_multi_record"
    assert len(m.group(1).split(",")) == 15
    assert "auv_step_multi_record" in _capi.EXPORTED_SYMBOLS
    assert len(lib.auv_step_multi_record.argtypes) == 15
    # a pure addition: the ABI version and the plain call's signature stay
    assert _capi.ABI_VERSION == 5 and len(lib.auv_step_multi.argtypes) == 12


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_recording_kernel_fits_the_register_budget():
    src = os.path.join(ROOT, "gym_auv_amd", "csrc", "k_step_fused.hip")
    tmp = tempfile.mkdtemp(prefix="auv_rec_")
    try:
        subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-c", src,
                        "-o", os.path.join(tmp, "k.o"), "-save-temps"], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        assert asm, os.listdir(tmp)
        text = open(os.path.join(tmp, asm[0])).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    blocks = re.split(r"\n\s+- \.agpr_count:", text)[1:]

    def field(b, key):
        return int(re.search(r"\.%s:\s+(\d+)" % key, b).group(1))

    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks]
    rec = [b for b, nm in zip(blocks, names) if "k_step_record" in nm]
    assert len(rec) == 1, names                                  # exactly one recording kernel
    name = re.search(r"\.name:\s+(\S+)", rec[0]).group(1)
    assert "k_step_multi" not in name and "k_step_roles" not in name, name
    assert field(rec[0], "vgpr_count") <= 128                    # four waves per SIMD
    assert field(rec[0], "vgpr_spill_count") == 0
    assert field(rec[0], "group_segment_fixed_size") == 0        # the per-wave slice is dynamic LDS
    assert field(rec[0], "private_segment_fixed_size") <= 16
    # ... and no larger than the plain launch's, which is still the only kernel of its name
    mul = [b for b, nm in zip(blocks, names) if "k_step_multi" in nm]
    assert len(mul) == 1, names
    assert field(rec[0], "private_segment_fixed_size") <= field(mul[0], "private_segment_fixed_size")
