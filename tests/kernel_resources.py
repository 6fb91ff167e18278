"""Cross-compile one source file of gym_auv_amd/csrc for gfx950 and read every kernel's resource fields from the code object's metadata
-- TEST TOOLING ONLY (tests/test_policy_arch.py and the *_resources.py tests of k9, k11 and k12).  Nothing is run; no GPU is needed."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = {"vgpr": "vgpr_count", "vgpr_spill": "vgpr_spill_count", "sgpr_spill": "sgpr_spill_count",
          "private": "private_segment_fixed_size", "static_lds": "group_segment_fixed_size"}


@functools.lru_cache(maxsize=None)
def kernel_resources(src_name):
    """A tuple of dicts, one per kernel of csrc/<src_name>: name (mangled) and the integer fields of FIELDS.  Compiled once per file
    and process; the result is shared, so leave it unchanged."""
    src = os.path.join(ROOT, "gym_auv_amd", "csrc", src_name)
    tmp = tempfile.mkdtemp(prefix="auv_res_")
    try:
        subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-c", src,
                        "-o", os.path.join(tmp, "k.o"), "-save-temps"], cwd=tmp, check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
        assert asm, os.listdir(tmp)
        text = open(os.path.join(tmp, asm[0])).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kernels = []
    for b in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        k = {"name": re.search(r"\.name:\s+(\S+)", b).group(1)}
        for key, field in FIELDS.items():
            k[key] = int(re.search(r"\.%s:\s+(\d+)" % field, b).group(1))
        kernels.append(k)
    return tuple(kernels)


def describe(k):
    return "%s: %d VGPRs, %d + %d spilled (VGPR + SGPR), %d bytes private, %d bytes static LDS" % (
        k["name"], k["vgpr"], k["vgpr_spill"], k["sgpr_spill"], k["private"], k["static_lds"])


def assert_policy_budget(k):
    """What a forward launch's shape -- 512 threads and up to 65 KB of LDS per workgroup, two workgroups per CU -- allows: 128 VGPRs,
    nothing in scratch memory, and no static LDS in front of the 16-byte aligned dynamic tiles."""
    print(describe(k))
    assert k["vgpr"] <= 128, (k["name"], k["vgpr"])
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["private"] == 0, describe(k)
    assert k["static_lds"] == 0, (k["name"], k["static_lds"])
