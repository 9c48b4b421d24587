"""attn_fwd_persistent_quad_kernel against the toolchain, as tests/test_isa_pins.py holds the kernel it walks next to (no GPU
needed: the gfx950 code object in csrc/t2s_attn.o is read through tools/isa_report.py).

The quad kernel hides its LDS-DMA from hipcc (glds16_asm) and waits with ONE hand-counted `s_waitcnt vmcnt(2)` per key block
(derived at wait_ring in csrc/t2s_attn.hip: every wave issues one or two pieces per block, three blocks ahead; its two
youngest operations are never pieces of the block the barrier hands over).  That holds whatever else is in flight -- a
younger operation only makes the wait stricter -- but a vector load the compiler put INSIDE a block loop, or a scratch
reload, would drain the ring at every block; the only plain loads of the walk, the next pass's Q, are requested between two
runs of blocks and show in the loops as the compiler's own waits for them (vmcnt 7, 5, 4, 3, 1, 0 on the block-11 branch).

Pinned: VGPRs within two waves per SIMD, no scratch, only the f32 MFMA, and every streaming loop (tools/isa_report.py:
innermost backward-branch ranges that hold LDS-DMA and MFMAs) as (MFMAs, LDS-DMAs, other vector loads, vector stores, scratch
ops, vmcnt waits in program order).  The MFMA counts are those of the four pass forms (16 per tile for scores, 16 for PV, 16
for a re-reference where the compiler laid that branch inside the range); one or two LDS-DMA (main ring, second ring).  See
tests/test_isa_pins.py before touching a pin."""
import importlib.util
import os
import shutil
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_report", os.path.join(REPO, "tools", "isa_report.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)

pytestmark = pytest.mark.skipif(not (os.path.exists(os.path.join(isa.LLVM, "llvm-objdump")) and
                                     os.path.exists(os.path.join(REPO, "t2ms_amd", "csrc", "t2s_attn.o"))),
                                reason="needs the ROCm LLVM tools and the built objects (__graft_entry__.build())")

QUAD = "_ZN3t2s31attn_fwd_persistent_quad_kernelEPKfS1_S1_Pfi"
Q_WAITS = (7, 5, 4, 3, 1, 0)     # the compiler's waits for the eight Q loads of the next pass (block 11 only)
# Per range: (MFMAs, LDS-DMAs, loads, stores, scratch ops, vmcnt waits).  Scores 16 and PV 16 MFMAs per tile, a re-reference 16
# more per tile where the compiler laid that branch inside the range; two LDS-DMA: this wave's piece for the main and for the
# second ring; the one counted wait, vmcnt(2), behind the Q waits where the range holds the block-11 branch.
LOOPS = [(48, 2, 0, 0, 0, (2,)), (32, 2, 0, 0, 0, Q_WAITS + (2,)), (96, 2, 0, 0, 0, (2,)), (64, 2, 0, 0, 0, Q_WAITS),
         (96, 2, 0, 0, 0, (2,)), (96, 2, 0, 0, 0, (2,)), (32, 2, 0, 0, 0, Q_WAITS + (2,)), (96, 2, 0, 0, 0, (2,))]


@pytest.fixture(scope="module")
def quad():
    wd = tempfile.mkdtemp(prefix="t2s_isa_quad_")
    try:
        rep = isa.report("t2s_attn", wd)
        co = isa.extract_code_object(os.path.join(REPO, "t2ms_amd", "csrc", "t2s_attn.o"), wd)
        dis = isa.disassemble(co)
        assert QUAD in rep, f"{QUAD} is not in the gfx950 code object (renamed? then rename the pin)"
        yield rep[QUAD], dis[QUAD]
    finally:
        shutil.rmtree(wd, ignore_errors=True)


def test_quad_kernel_fits_two_waves_per_simd_without_scratch(quad):
    r, insts = quad
    m = r["meta"]
    assert m["vgpr_count"] + m.get("agpr_count", 0) <= 256, m
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert r["scratch"] == 0 and not any(mn.startswith("scratch_") for _, mn, _ in insts)
    assert m["wavefront_size"] == 64


def test_quad_kernel_uses_the_f32_matrix_instruction_only(quad):
    kinds = {mn for _, mn, _ in quad[1] if mn.startswith("v_mfma")}
    assert kinds == {"v_mfma_f32_32x32x2_f32"}, kinds


def test_quad_kernel_block_loops_hold_no_vector_load_and_one_counted_wait(quad):
    r, _ = quad
    got = isa.streaming_loops(r)
    assert got, "no streaming loop found"
    for mfma, dma, loads, stores, scratch, waits in got:
        assert loads == 0 and stores == 0 and scratch == 0, got
        assert dma in (1, 2), got
        assert waits in ((2,), Q_WAITS, Q_WAITS + (2,)), got   # nothing but the Q waits and the counted wait, in that order
    for lp in r["loops"]:
        if lp["lds_dma"]:
            assert lp["scratch"] == 0, lp
    assert got == LOOPS, f"the LDS-DMA loops changed shape\n  pinned {LOOPS}\n  now    {got}"
