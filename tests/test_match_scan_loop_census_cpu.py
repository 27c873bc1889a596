"""What the match scan's chunk loop executes besides its MFMAs (tools/scan_loop_census.py), checked in the assembly
without a GPU.

The scan is bound by vector issue: per 128 MFMAs - one 128-row chunk of Y against a wave's eight
X tiles - the top-2 arithmetic is 152 vector instructions, and whatever else the compiler leaves on the vector pipe in
that loop is paid for at the same rate.  The loop once carried 21 such instructions per chunk (LDS read addresses
formed per step, 64-bit global addresses of the DMA pieces, wave-uniform predicates kept in a VGPR) and one change of
the surrounding code put an `s_waitcnt vmcnt(0)` in front of an LDS read in every step (profiles/boundary/README.md
section 1).  Both come back silently; this test fails first.  The bounds are what the kernel reaches: three v_add_u32
per chunk move the three LDS read bases to the next ring buffer."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    from pycolmap_amd import build
    import scan_loop_census as slc
    try:
        build._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("census") / "match_mfma.s"
    slc.compile_to_asm(out)
    return slc.census(out.read_text())


@pytest.mark.parametrize("mode", [0, 1])
def test_the_chunk_loop_carries_the_top2_work_and_three_address_ops(census, mode):
    import scan_loop_census as slc
    assert mode in census, "match_mfma_kernel<%d> not found in the assembly" % mode
    k = census[mode]
    loops = k["loops"]
    steady = [lp for lp in loops if lp["kind"] == "steady"]
    assert len(steady) == 1, "one loop holds MFMAs and the Y stream's DMA: %r" % [lp["kind"] for lp in loops]
    for lp in loops:  # the steady loop and the drain of the last chunks
        assert lp["mfma"] > 0 and lp["mfma"] % 128 == 0
        p = slc.per_chunk(lp)
        assert p["top2"] == 152, p["top2_by_op"]
        assert p["other_valu"] <= 3, p["other_valu_by_op"]
        assert not [op for op in lp["other_valu_by_op"] if op.startswith(("v_cndmask", "v_cmp"))]
        assert p["ds_read"] == 24
    p = slc.per_chunk(steady[0])
    assert p["dma"] == 5 and p["s_barrier"] == 1   # a wave's four pieces and wave 0's rs128 block; one crossing
    assert not [w for w in steady[0]["waits"] if "vmcnt(0)" in w], steady[0]["waits"]
    assert k["vgprs"] <= 256 and k["scratch_bytes"] == 0 and k["lds_bytes"] <= 81920


SNIPPET = """
_ZN3amc17match_mfma_kernelILi0EEEvPKNS_7SegDescE:
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v9, 0
.LBB0_1:                                ; =>This Loop Header: Depth=1
	s_add_i32 s2, s2, 1
.LBB0_2:                                ;   Parent Loop BB0_1 Depth=1
	s_add_i32 m0, s7, 0x810
	global_load_lds_dwordx4 v1, s[0:1]
	v_lshl_add_u64 v[2:3], s[0:1], 0, v[4:5]
	;;#ASMSTART
	v_mfma_i32_16x16x64_i8 v[10:13], v[20:23], v[30:33], v[40:43]
	;;#ASMEND
	;;#ASMSTART
	v_mfma_i32_16x16x64_i8 v[10:13], v[24:27], v[34:37], v[10:13]
	;;#ASMEND
	s_cmp_lg_u32 s3, 0
	s_cbranch_scc1 .LBB0_4
; %bb.3:                                ;   in Loop: Header=BB0_2 Depth=2
	v_and_b32_e32 v6, 0x7f, v7
	v_or_b32_e32 v7, 0x7f, v7
	v_or_b32_e32 v8, 0x7f, v8
	v_or_b32_e32 v9, 0x7f, v9
	v_or_b32_e32 v10, 0x7f, v10
	v_cndmask_b32_e32 v6, v6, v7, vcc
.LBB0_4:                                ;   in Loop: Header=BB0_2 Depth=2
	;;#ASMSTART
	v_max3_i32 v50, v10, v11, v12
	v_max_i32 v51, v50, v13
	;;#ASMEND
	s_nop 0
	ds_read_b128 v[20:23], v60 offset:32
	s_waitcnt vmcnt(8)
	s_barrier
	v_cndmask_b32_e64 v61, 0, 1, s[8:9]
	s_cmp_lt_i32 s2, s6
	s_cbranch_scc1 .LBB0_2
; %bb.5:
	v_mov_b32_e32 v0, 0
	s_cmp_lt_i32 s2, s9
	s_cbranch_scc1 .LBB0_1
	s_endpgm
.Lfunc_end0:
amdhsa.kernels:
  - .agpr_count:     0
    .group_segment_fixed_size: 67600
    .name:           _ZN3amc17match_mfma_kernelILi0EEEvPKNS_7SegDescE
    .private_segment_fixed_size: 0
    .vgpr_count:     222
  - .agpr_count:     0
    .group_segment_fixed_size: 16
    .name:           _ZN3amc16seg_count_kernelEi
    .private_segment_fixed_size: 8
    .vgpr_count:     20
"""


def test_the_census_counts_a_hand_written_loop():
    import scan_loop_census as slc
    res = slc.census(SNIPPET)
    assert list(res) == [0]
    k = res[0]
    assert (k["vgprs"], k["scratch_bytes"], k["lds_bytes"]) == (222, 0, 67600)
    assert len(k["loops"]) == 1   # the inner loop; the outer one holds it and is not counted twice
    lp = k["loops"][0]
    assert lp["kind"] == "steady" and lp["mfma"] == 2 and lp["dma"] == 1
    assert lp["top2"] == 2 and lp["top2_by_op"] == {"v_max3_i32": 1, "v_max_i32": 1}
    # outside the flush block: the 64-bit address add and the predicate carried in a VGPR
    assert lp["other_valu_by_op"] == {"v_cndmask_b32": 1, "v_lshl_add_u64": 1}
    assert lp["flush"]["other_valu"] == 6
    assert (lp["salu"], lp["branches"], lp["s_nop"], lp["ds_read"], lp["s_barrier"]) == (3, 2, 1, 1, 1)
    assert lp["waits"] == ["vmcnt(8)"]
    assert slc.per_chunk(lp)["other_valu"] == 128
