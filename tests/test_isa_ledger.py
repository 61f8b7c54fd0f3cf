"""tools/isa_ledger.py (CPU only): the instruction price classes, and a ledger of the C2 sampler's per-position loop read
from a gfx950 assembly built here — phases found, the exact fallback left out, and a resource line that still fits two
1024-thread workgroups per CU (<= 64 VGPRs, <= 72 SGPRs, no scratch)."""
import io
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_ledger as IL  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.parametrize("mnem,ops,cyc", [
    ("v_add_u32_e32", "v1, v2, v3", 2), ("v_add_u32_e32", "v1, s2, v3", 4), ("v_lshrrev_b32_e32", "v1, 18, v7", 2),
    ("v_lshlrev_b32_e32", "v1, 13, v7", 4), ("v_and_b32_e32", "v1, 0x3ffc, v1", 2), ("v_bitop3_b32", "v1, v2, v3, v4 bitop3:0x96", 2),
    ("v_mad_u64_u32", "v[6:7], s[12:13], v6, s48, 0", 4), ("v_cmp_lt_u32_e32", "vcc, 7, v6", 2),
    ("v_cmp_gt_i32_e32", "vcc, s2, v41", 4), ("v_cndmask_b32_e64", "v6, 0, 1, s[10:11]", 4),
    ("v_add_u32_dpp", "v49, v48, v48 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1", 4),
    ("v_add_u32_sdwa", "v23, v45, v23 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1", 4),
    ("v_mbcnt_lo_u32_b32", "v41, s52, 0", 4), ("v_mov_b32_e32", "v42, s58", 2), ("v_add3_u32", "v1, v2, v3, v4", 4),
])
def test_price_classes(mnem, ops, cyc):
    assert IL.price(mnem, ops) == cyc


@pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="needs hipcc to build the assembly")
def test_ledger_of_the_c2_sampler(tmp_path):
    out = tmp_path / "s.s"
    IL.compile_asm(IL.DEFAULT_SRC, str(out))
    name, blocks, res = IL.parse_kernel(out.read_text(), IL.DEFAULT_KERNEL)
    buf = io.StringIO()
    r = IL.report(name, blocks, res, out=buf)
    text = buf.getvalue()
    assert "sample_philox_v2_kernel" in name and "1 cold region(s) left out" in text
    assert len(r["phases"]) >= 4 and r["total"]["cyc"] > 0
    assert r["lds"]["ds_add_rtn_u32"] >= 4                               # the four keys' histogram atomics
    assert res["NumVgprs"] <= 64 and res["TotalNumSgprs"] <= 72 and res["ScratchSize"] == 0 and res["VgprSpills"] == 0
