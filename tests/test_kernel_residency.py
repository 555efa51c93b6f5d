"""The flagship run's kernels fit the GPU in one round of workgroups.

Read from the compiler's resource listing the build saves next to the kernels' object
(weightedsampling.jl_amd/build/wsmc_kernels.resources.txt, tools/kres.py): register, LDS and
scratch counts only. The rule for the waves a SIMD admits as a function of the scalar registers is
the measured one (8 up to 80 SGPRs, 7 up to 96, 6 from 98), not the compiler's occupancy line.
"""
import importlib.util
import pathlib

import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
_spec = importlib.util.spec_from_file_location("kres", REPO / "tools" / "kres.py")
kres = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kres)

CUS = 256
# the instantiations the 1M one-GPU run launches (mangled-name parts)
PROP_1M = "k_ssm2d_propILi0ELi1ELi512ELb1ELb0EE"    # <MODE 0, IT 1, NT 512, QS, not ISL>
FINAL_1M = "k_ssm2d_finalILb0ELi2ELi0EE"            # <not ISL, P 2, DG 0>
FILLS = ("k_rs_fill_fusedILi0ELb0EE", "k_rs_fill_fusedILi0ELb1EE")


@pytest.fixture(scope="module")
def res():
    if not kres.LISTING.exists():
        pytest.fail(f"{kres.LISTING} is missing: build() saves it with the kernels' object")
    return kres.parse(kres.LISTING)


def test_rule_bands():
    assert kres.waves_by_sgprs(80) == 8
    assert kres.waves_by_sgprs(82) == 7
    assert kres.waves_by_sgprs(96) == 7
    assert kres.waves_by_sgprs(98) == 6
    assert kres.waves_by_sgprs(106) == 6
    assert kres.waves_per_simd(70, 64) == 8
    assert kres.waves_per_simd(70, 72) == 7
    # 512-thread blocks take 2 waves a SIMD: 4 a CU at 8 waves, 3 at 6 or 7
    assert kres.blocks_per_cu(512, 80, 64, 2400) == 4
    assert kres.blocks_per_cu(512, 96, 59, 2400) == 3
    assert kres.blocks_per_cu(512, 106, 59, 2400) == 3
    assert kres.blocks_per_cu(256, 60, 54, 1040) == 8


def test_propagate_of_the_1m_run_is_resident_in_one_round(res):
    r = kres.find(res, PROP_1M)
    assert r["sgprs"] <= 80
    assert r["vgprs"] + r["agprs"] <= 64
    assert r["scratch"] == 0
    blocks = -(-1_000_000 // 1024)
    assert blocks == 977
    assert blocks <= CUS * kres.blocks_per_cu(512, r["sgprs"], r["vgprs"] + r["agprs"], r["lds"])


def test_traceback_of_the_1m_run_is_resident_in_one_round(res):
    r = kres.find(res, FINAL_1M)
    assert r["scratch"] == 0
    blocks = -(-(1_000_000 // 2) // 256)
    assert blocks == 1954
    assert blocks <= CUS * kres.blocks_per_cu(256, r["sgprs"], r["vgprs"] + r["agprs"], r["lds"])


@pytest.mark.parametrize("name", FILLS)
def test_fill_uses_no_scratch(res, name):
    assert kres.find(res, name)["scratch"] == 0
