"""The generated code of vn_threshold_kernel (csrc/vn_threshold.hip), without a GPU, by the method of
tests/test_thresh_resources.py: the file compiled device-only for gfx950 with the compiler's resource report, and the
conditions the design states for every instance: twelve instances (three CN-word forms x dv = 4 or generic x two adjacency
widths), at most 64 VGPRs, no VGPR spill, 8 waves per SIMD (two 1024-thread workgroups per CU).
profiles/vn_threshold_static.txt has the figures."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = {"VGPRs": "vgprs", "VGPRs Spill": "vgpr_spills", "Occupancy [waves/SIMD]": "waves"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="needs hipcc for the resource report")


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    """{mangled kernel name: {vgprs, vgpr_spills, waves}}"""
    out = tmp_path_factory.mktemp("vn_threshold")
    src = os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "vn_threshold.hip")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only",
           "-S", "-Rpass-analysis=kernel-resource-usage", "-o", str(out / "vn_threshold.s"), src]
    report = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    found = {}
    for block in report.split("remark: Function Name: ")[1:]:
        name = block.split()[0]
        found[name] = {key: int(re.search(re.escape(field) + r": (\d+)", block).group(1)) for field, key in FIELDS.items()}
    return found


def test_twelve_instances_of_the_kernel(instances):
    assert len(instances) == 12 and all("vn_threshold_kernel" in name for name in instances), sorted(instances)
    for form in ("Packed", "WideTILb0E", "WideTILb1E"):
        assert sum(form in name for name in instances) == 4, form


def test_every_instance_keeps_two_workgroups_per_cu_without_spills(instances):
    for name, res in instances.items():
        assert res["vgprs"] <= 64 and res["vgpr_spills"] == 0 and res["waves"] == 8, (name, res)
