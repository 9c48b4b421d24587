"""The wide bf16x3 / bf16 kernels against the toolchain, as tests/test_wide_isa_pins.py holds the wide f32 ones (no GPU needed:
the gfx950 code objects in csrc/*.o are read through tools/isa_report.py).

attn_fwd_x3_wide_kernel / attn_fwd_bf16p_wide_kernel: every wave issues its own LDS-DMA pieces of a key block (NPW per block:
bf16x3 waves 0-3 two, waves 4-7 one; one plane waves 0-3 one, waves 4-7 none) and waits `s_waitcnt vmcnt(NPW)` in front of
the block's barrier -- correct only while the key-block loop holds exactly those DMAs, that one counted wait, one barrier and
no vector-memory instruction of the compiler's own.  dit_rows_x3_wide_kernel / dit_rows_bf16p_wide_kernel: the streaming
loops of their 480-token counterparts.  This is about the wait structure only; see tests/test_isa_pins.py before touching a
pin."""
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
                                     os.path.exists(os.path.join(REPO, "t2ms_amd", "csrc", "t2s_attn_x3.o"))),
                                reason="needs the ROCm LLVM tools and the built objects (__graft_entry__.build())")

NS = "_ZN3t2s"
# kernel -> {LDS-DMAs per key-block loop: MFMAs of that loop}: one loop form per wave group (2 tiles x (QK + PV) per block)
ATTN = {
    NS + "12_GLOBAL__N_123attn_fwd_x3_wide_kernelEPKfPKDF16bS4_Pfii": {2: 72, 1: 72},      # 48 in the block loop + 24: its re-reference
    NS + "12_GLOBAL__N_126attn_fwd_bf16p_wide_kernelEPKfPKDF16bS4_Pfii": {1: 12, 0: 12},   # 8 + 4
}
ROWS = [(NS + f"{len(wide)}{wide}ILb{a}ELb{b}EEEvNS_9RowArgsX3E", NS + f"{len(base)}{base}ILb{a}ELb{b}EEEvNS_9RowArgsX3E")
        for wide, base in (("dit_rows_x3_wide_kernel", "dit_rows_x3_kernel"), ("dit_rows_bf16p_wide_kernel", "dit_rows_bf16p_kernel"))
        for a, b in ((0, 1), (1, 1), (1, 0))]


@pytest.fixture(scope="module")
def reports():
    wd = tempfile.mkdtemp(prefix="t2s_isa_wide_math_")
    try:
        out = {}
        for stem in ("t2s_attn_x3", "t2s_dit"):
            out.update(isa.report(stem, wd))
        yield out
    finally:
        shutil.rmtree(wd, ignore_errors=True)


@pytest.mark.parametrize("kernel", sorted(ATTN))
def test_wide_attention_block_loops_hold_one_counted_wait_per_barrier(reports, kernel):
    assert kernel in reports, f"{kernel} is not in the gfx950 code objects (renamed? then rename the pin)"
    r, m, name = reports[kernel], reports[kernel]["meta"], isa.demangled(kernel)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert r["scratch"] == 0 and m["vgpr_count"] <= 256 and m["wavefront_size"] == 64, (name, m)
    # the key-block loops in their plainest form: one barrier, no store, no load of the compiler's own (the forms that also
    # hold the Q prefetch or an item's O stores are the same loops seen through an enclosing branch)
    block = [lp for lp in r["loops"] if lp["barriers"] == 1 and lp["vmem_stores"] == 0 and lp["vmem_loads"] == 0 and lp["mfma"]]
    assert block, name
    seen = {}
    for lp in block:
        npw = lp["lds_dma"]
        assert lp["scratch"] == 0 and lp["vmcnt_waits"] == ([npw] if npw else []), (name, lp)
        seen[npw] = lp["mfma"]
    assert seen == ATTN[kernel], f"{name}: pieces per wave and block -> MFMAs\n  pinned {ATTN[kernel]}\n  now    {seen}"
    # and in EVERY loop around a barrier the DMAs of a block are that wave's pieces, never more
    for lp in r["loops"]:
        if lp["barriers"] == 1:
            assert lp["lds_dma"] in ATTN[kernel], (name, lp)


@pytest.mark.parametrize("wide,base", ROWS)
def test_wide_bf16_row_kernels_keep_the_streaming_loops_of_their_480_counterparts(reports, wide, base):
    assert wide in reports and base in reports, (wide, base)
    rw, rb = reports[wide], reports[base]
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        assert rw["meta"][key] == rb["meta"][key], (isa.demangled(wide), key)
    assert rw["scratch"] == rb["scratch"] and rw["mfma"] == rb["mfma"]
    assert rw["meta"]["vgpr_count"] <= 256
    assert isa.streaming_loops(rw) == isa.streaming_loops(rb), isa.demangled(wide)
