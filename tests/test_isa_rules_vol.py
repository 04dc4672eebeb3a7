"""CPU: the rules of tests/test_isa_rules.py for the two volume shade kernels that ship in libtvr.so (shade16_vol_kernel<RC>, csrc/tvr_shade16.hip) — their names hold
neither `shade_kernel` nor `shade16_kernel`, so that file's audit does not reach them — and the resource bound their launch rests on: three waves per SIMD
 need at most 168 VGPRs (512 per SIMD lane, allocated in eights) and no scratch."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "scripts"))
LIB = os.path.join(ROOT, "jittor-myc-nerfs_amd", "lib", "libtvr.so")


@pytest.fixture(scope="module")
def report():
    import __graft_entry__ as g
    import isa_check
    if not os.path.exists(LIB):
        g.build()
    return isa_check.audit(LIB, "shade16_vol_kernel")


def test_both_volume_kernels_are_audited(report):
    assert len(report) == 2, sorted(report)                        # range check on / off
    assert all(v["mfma"] == 432 for v in report.values())          # layers 1 and 2: 72 x 6; the basis product is absent


def test_vmcnt_accounting_war_and_valu_to_mfma(report):
    for name, v in report.items():
        assert v["raw_violations_fallthrough"] == 0 and v["raw_violations_execz_taken"] == 0, (name, v["examples"]["raw"])
        assert v["war_adjacent"] == 0, (name, v["examples"]["war"])
        assert v["valu_to_mfma_adjacent"] == 0, (name, v["examples"]["valu_to_mfma"])


def test_no_global_load_between_the_mfmas(report):
    for name, v in report.items():
        assert v["vmem_loads_between_first_and_last_mfma"] == 0, f"{name}: a global (or spill) load sits between the MFMAs of a tile"


def test_three_waves_per_simd_fit(report):
    for name, v in report.items():
        assert v["vgprs"] + v["agprs"] <= 168, (name, v["vgprs"], v["agprs"])
        assert v["scratch_bytes"] == 0 and v["vgpr_spills"] == 0 and v["sgpr_spills"] == 0, name


def test_resources_are_the_code_objects_notes():
    """isa_check reports the resources of every kernel it audits: the factored shade16 kernels beside the volume kernels."""
    import isa_check
    rep = isa_check.audit(LIB, "shade16")
    assert len(rep) == 6 and all(isinstance(v["vgprs"], int) and v["vgprs"] > 0 and v["scratch_bytes"] == 0 for v in rep.values())
    assert all(v["vgprs"] > 168 for k, v in rep.items() if "shade16_kernel" in k)          # the factored kernels: two waves per SIMD
