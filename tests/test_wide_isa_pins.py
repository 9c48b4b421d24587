"""The wide-latent kernels against the toolchain, as tests/test_isa_pins.py holds the 480-token ones (no GPU needed: the gfx950
code objects in csrc/*.o are read through tools/isa_report.py).

attn_fwd_packed_wide_kernel<25 | 32> and dit_rows[16]_wide_kernel<..> are further instantiations of the bodies behind
attn_fwd_packed_kernel<2> and dit_rows[16]_kernel<..>: the same LDS rings, the same hand-counted `s_waitcnt vmcnt(N)`.  What
is pinned per wide kernel is what the build produces: no scratch, VGPRs within the budget of its 480-token counterpart, and
streaming loops of the counterpart's shape -- (MFMAs, LDS-DMAs, other vector loads, vector stores, scratch ops, vmcnt waits in
program order), both as written down here and as found in the counterpart of the same build.  This is about the wait
structure only; see tests/test_isa_pins.py before touching a pin."""
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

NS = "_ZN3t2s"
ATT480 = NS + "22attn_fwd_packed_kernelILi2EEEvPKfS2_S2_Pfi"
# wide kernel -> (its 480-token counterpart, VGPR budget, [(mfma, lds_dma, loads, stores, scratch ops, vmcnt waits)] streaming loops)
PINS = {
    NS + "27attn_fwd_packed_wide_kernelILi25EEEvPKfS2_S2_Pfi": (ATT480, 256, [(32, 2, 0, 0, 0, (4,)), (64, 2, 0, 0, 0, (4,))]),
    NS + "27attn_fwd_packed_wide_kernelILi32EEEvPKfS2_S2_Pfi": (ATT480, 256, [(32, 2, 0, 0, 0, (4,)), (64, 2, 0, 0, 0, (4,))]),
    NS + "20dit_rows_wide_kernelILb0ELb1EEEvNS_7RowArgsE": (NS + "15dit_rows_kernelILb0ELb1EEEvNS_7RowArgsE", 256, [(128, 4, 0, 6, 0, ())]),
    NS + "20dit_rows_wide_kernelILb1ELb1EEEvNS_7RowArgsE": (NS + "15dit_rows_kernelILb1ELb1EEEvNS_7RowArgsE", 256,
                                                            [(128, 8, 0, 0, 0, (4, 4)), (128, 4, 0, 6, 0, ())]),
    NS + "20dit_rows_wide_kernelILb1ELb0EEEvNS_7RowArgsE": (NS + "15dit_rows_kernelILb1ELb0EEEvNS_7RowArgsE", 256, [(128, 8, 0, 0, 0, (0, 4, 0))]),
    NS + "22dit_rows16_wide_kernelILb0ELb1EEEvNS_7RowArgsE": (NS + "17dit_rows16_kernelILb0ELb1EEEvNS_7RowArgsE", 256, [(128, 4, 0, 4, 0, (0,))]),
    NS + "22dit_rows16_wide_kernelILb1ELb1EEEvNS_7RowArgsE": (NS + "17dit_rows16_kernelILb1ELb1EEEvNS_7RowArgsE", 256,
                                                              [(128, 8, 0, 0, 0, (4, 4)), (128, 4, 0, 4, 0, (0,))]),
    NS + "22dit_rows16_wide_kernelILb1ELb0EEEvNS_7RowArgsE": (NS + "17dit_rows16_kernelILb1ELb0EEEvNS_7RowArgsE", 256, [(128, 8, 0, 0, 0, (0, 4, 0))]),
}


@pytest.fixture(scope="module")
def reports():
    wd = tempfile.mkdtemp(prefix="t2s_isa_wide_")
    try:
        out = {}
        for stem in ("t2s_attn", "t2s_dit"):
            out.update(isa.report(stem, wd))
        yield out
    finally:
        shutil.rmtree(wd, ignore_errors=True)


@pytest.mark.parametrize("kernel", sorted(PINS))
def test_wide_kernel_keeps_the_counted_wait_structure_of_its_480_counterpart(reports, kernel):
    counterpart, vgpr_budget, loops = PINS[kernel]
    assert kernel in reports, f"{kernel} is not in the gfx950 code objects (renamed? then rename the pin)"
    assert counterpart in reports, counterpart
    r, m, name = reports[kernel], reports[kernel]["meta"], isa.demangled(kernel)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert r["scratch"] == 0, f"{name}: {r['scratch']} scratch_* instructions (every reload is a vmcnt(0) inside a counted ring)"
    assert m["vgpr_count"] <= vgpr_budget, f"{name}: {m['vgpr_count']} VGPRs, two waves per SIMD need <= {vgpr_budget}"
    assert m["wavefront_size"] == 64
    got = isa.streaming_loops(r)
    assert got == loops, f"{name}: the LDS-DMA loops changed shape\n  pinned {loops}\n  now    {got}"
    assert got == isa.streaming_loops(reports[counterpart]), f"{name}: differs from {isa.demangled(counterpart)}"
    for mfma, dma, loads, stores, scratch, waits in got:
        assert loads == 0 and scratch == 0, (name, got)
