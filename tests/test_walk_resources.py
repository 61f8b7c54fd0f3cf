"""The generated code of the four kernels that walk one sampled code per frame, without a GPU: eps_walk_kernel (csrc/eps_stages.h,
instantiated by peel_sweep_eps.hip and by full_bp_eps.hip), frame_threshold_kernel (csrc/frame_threshold.hip) and
vn_threshold_kernel (csrc/vn_threshold.hip).  Each source is compiled device-only for gfx950 with the compiler's resource report,
and the conditions the design states hold for every instance: twelve instances per source (three CN-word forms x dv = 4 or
generic x two adjacency widths), at most 64 VGPRs, no VGPR spill, 8 waves per SIMD (two 1024-thread workgroups per CU).
profiles/eps_walk_static.txt, profiles/frame_threshold_static.txt and profiles/vn_threshold_static.txt have the figures."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = {"peel_sweep_eps": "eps_walk_kernel", "full_bp_eps": "eps_walk_kernel", "frame_threshold": "frame_threshold_kernel",
           "vn_threshold": "vn_threshold_kernel"}
THRESHOLD_SOURCES = ("frame_threshold", "vn_threshold")
FIELDS = {"VGPRs": "vgprs", "VGPRs Spill": "vgpr_spills", "Occupancy [waves/SIMD]": "waves"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="needs hipcc for the resource report")


@pytest.fixture(scope="module")
def instances(tmp_path_factory):
    """source -> {mangled kernel name: {vgprs, vgpr_spills, waves}}, every source compiled once"""
    out = tmp_path_factory.mktemp("walk_resources")
    found = {}

    def of(f):
        if f not in found:
            src = os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", f + ".hip")
            cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950",
                   "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", str(out / (f + ".s")), src]
            report = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
            found[f] = {}
            for block in report.split("remark: Function Name: ")[1:]:
                name = block.split()[0]
                found[f][name] = {key: int(re.search(re.escape(field) + r": (\d+)", block).group(1)) for field, key in FIELDS.items()}
        return found[f]
    return of


@pytest.mark.parametrize("f", list(SOURCES))
def test_twelve_instances_of_the_kernel(instances, f):
    assert len(instances(f)) == 12 and all(SOURCES[f] in name for name in instances(f)), sorted(instances(f))


@pytest.mark.parametrize("f", THRESHOLD_SOURCES)
def test_four_instances_of_every_form(instances, f):
    for form in ("Packed", "WideTILb0E", "WideTILb1E"):
        assert sum(form in name for name in instances(f)) == 4, form


@pytest.mark.parametrize("f", list(SOURCES))
def test_every_instance_keeps_two_workgroups_per_cu_without_spills(instances, f):
    for name, res in instances(f).items():
        assert res["vgprs"] <= 64 and res["vgpr_spills"] == 0 and res["waves"] == 8, (name, res)
