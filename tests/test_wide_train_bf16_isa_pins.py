"""The wide bf16 training kernels against the toolchain, in the manner of tests/test_wide_isa_pins.py (no GPU needed: the gfx950
code objects in csrc/*.o are read through tools/isa_report.py).

attn16_fwd_kernel<0, ..>, attn16_bwd_dq_kernel<0, ..> and attn16_bwd_dkv_kernel<0, ..> are the run-time forms of the 480-token
kernels: two whole bf16 images of 800 / 1024 rows in dynamic LDS, filled by LDS-DMA (global_load_lds_dwordx4) and waited for
with ONE s_waitcnt vmcnt(0) in front of the first barrier.  bgemm_kernel<.., 0> and final_bwd_kernel<true, .., 0> are the
run-time forms of the step's GEMMs and fused final layer.  Pinned per kernel, from the code object's metadata and its
`s_waitcnt` pattern: no scratch (private segment 0, no spills, no scratch_* instruction); an LDS request within 163,840 B;
and for the attention kernels the DMA staging as written -- DMA loops free of other vector-memory instructions, the images
never staged through registers (no 8- or 16-byte LDS store), DMA loops of the shape of the 480-token counterpart of the
same build.  Nothing else is pinned."""
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
                                     os.path.exists(os.path.join(REPO, "t2ms_amd", "csrc", "t2s_attn_bf16.o"))),
                                reason="needs the ROCm LLVM tools and the built objects (__graft_entry__.build())")

LDS_BYTES = 163840
ATTN = {"attn16_fwd_kernel": 0, "attn16_bwd_dq_kernel": 0, "attn16_bwd_dkv_kernel": 2 * 1024 * 4}   # name -> bytes beside the two images
BG_STAGE_BYTES = 32 * 144


def _wide_attention_request(extra):
    return 2 * 1024 * 64 + extra                   # attn16_lds(1024, ..) of t2s_attn_bf16.hip: the larger of the two token counts


def _bgemm_request(K, N, EPI):
    waves = 8 if EPI == 3 else 12                  # launch_bgemm's `lds` (t2s_bf16.h)
    return N * K * 2 + N * 4 + waves * BG_STAGE_BYTES + (waves * 1024 if EPI == 3 else 0)


@pytest.fixture(scope="module")
def objects():
    wd = tempfile.mkdtemp(prefix="t2s_isa_wide_bf16_")
    try:
        out = {}
        for stem in ("t2s_attn_bf16", "t2s_train"):
            co = isa.extract_code_object(os.path.join(REPO, "t2ms_amd", "csrc", stem + ".o"), wd)
            out[stem] = {"report": isa.report(stem, wd), "dis": isa.disassemble(co)}
        yield out
    finally:
        shutil.rmtree(wd, ignore_errors=True)


def _no_scratch(name, r):
    m = r["meta"]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert r["scratch"] == 0, f"{name}: {r['scratch']} scratch_* instructions"


def _dma_loops(r):
    return [(lp["lds_dma"], lp["vmem_loads"], lp["vmem_stores"], lp["scratch"], lp["mfma"], tuple(lp["vmcnt_waits"]))
            for lp in sorted(r["loops"], key=lambda lp: (lp["first"], lp["last"])) if lp["lds_dma"]]


@pytest.mark.parametrize("kernel", sorted(ATTN))
def test_wide_bf16_attention_kernel(objects, kernel):
    rep, dis = objects["t2s_attn_bf16"]["report"], objects["t2s_attn_bf16"]["dis"]
    wide = [k for k in rep if kernel + "ILi0E" in k]
    narrow = [k for k in rep if kernel + "ILi480E" in k]
    assert len(wide) == 1 and len(narrow) == 1, (wide, narrow)
    name, r = isa.demangled(wide[0]), rep[wide[0]]
    _no_scratch(name, r)
    assert r["meta"]["wavefront_size"] == 64
    # the LDS request: nothing static beside the launch's dynamic allocation, which is sized for 1024 tokens
    assert r["meta"]["group_segment_fixed_size"] + _wide_attention_request(ATTN[kernel]) <= LDS_BYTES, r["meta"]
    # the staging: DMA loops with nothing else in them, as in the 480-token kernel of the same build
    loops = _dma_loops(r)
    assert loops, f"{name}: no LDS-DMA loop"
    for dma, loads, stores, scratch, mfma, waits in loops:
        assert dma == 1 and loads == 0 and stores == 0 and scratch == 0 and mfma == 0 and waits == (), (name, loops)
    assert set(loops) == set(_dma_loops(rep[narrow[0]])), f"{name}: DMA loops differ from {isa.demangled(narrow[0])}"
    insts = dis[wide[0]]
    mn = [m for _, m, _ in insts]
    assert sum(1 for m in mn if m.startswith("global_load_lds_dwordx4")) >= 1
    wide_lds_stores = [m for m in mn if m.startswith(("ds_write_b64", "ds_write_b128", "ds_write2", "ds_store_b64", "ds_store_b128"))]
    assert not wide_lds_stores, f"{name}: the images are staged through registers ({sorted(set(wide_lds_stores))})"
    # one full wait between the last DMA and the first barrier
    last_dma = max(i for i, m in enumerate(mn) if m.startswith("global_load_lds"))
    barrier = mn.index("s_barrier")
    assert last_dma < barrier
    waits = [o for _, m, o in insts[last_dma:barrier] if m == "s_waitcnt" and "vmcnt" in o]
    assert any("vmcnt(0)" in o for o in waits), (name, waits)


def test_wide_bf16_gemm_and_final_layer_kernels(objects):
    rep = objects["t2s_train"]["report"]
    # (K, N, PRO, EPI) of the instantiations whose tile -> sequence map is taken at run time
    want = {(128, 384, 1, 1), (128, 384, 3, 1), (128, 256, 3, 0), (256, 128, 0, 3), (384, 128, 0, 3)}
    seen = set()
    for k, r in rep.items():
        if "bgemm_kernelILi" in k and k.split("bgemm_kernelI")[1].startswith("Li") and "ELi0EEEvNS_9BGemmArgsE" in k:
            K, N, PRO, EPI, TOK = (int(p) for p in k.split("bgemm_kernelI")[1].split("EEEv")[0].replace("Li", "").split("E"))
            assert TOK == 0
            _no_scratch(isa.demangled(k), r)
            assert r["meta"]["group_segment_fixed_size"] + _bgemm_request(K, N, EPI) <= LDS_BYTES, (k, r["meta"])
            seen.add((K, N, PRO, EPI))
    assert seen == want, seen
    finals = [k for k in rep if "final_bwd_kernelILb1ELi" in k and "ELi0EEEv" in k]      # <true, 160 | 128, 0>
    assert len(finals) == 2, finals
    for k in finals:
        _no_scratch(isa.demangled(k), rep[k])
        assert rep[k]["meta"]["group_segment_fixed_size"] <= LDS_BYTES
