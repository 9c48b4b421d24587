"""The guidance interval on the host (no GPU): guided_steps' exact window arithmetic and refusals, infer.py --cfg_interval and its
directory suffix, and the two C entries in the header and the binding."""
import os
import re
from fractions import Fraction

import pytest

from t2ms_amd import _lib as L
from t2ms_amd.sampler import guided_steps, parse_cfg_interval, resolve_cfg_interval

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- guided_steps
@pytest.mark.parametrize("S", [1, 2, 3, 7, 10, 100, 1000, 99999])
def test_the_whole_interval_is_the_whole_loop(S):
    assert guided_steps((0, 1), S) == (0, S)
    assert guided_steps((0.0, 1.0), S) == (0, S)
    assert guided_steps(("0", "1"), S) == (0, S)


@pytest.mark.parametrize("interval,steps,want", [
    ((0.2, 0.8), 100, (20, 80)),
    ((0.25, 0.75), 50, (13, 38)),           # 12.5 -> 13, 37.5 -> 38: step j is guided iff lo * steps <= j < hi * steps
    ((0.3, 0.7), 1000, (300, 700)),
    ((0.5, 0.5), 10, (5, 5)),
    (("0.3333", 1), 3, (1, 3)),             # 1/3 written with four digits: 0.9999 -> 1
])
def test_guided_steps_table(interval, steps, want):
    assert guided_steps(interval, steps) == want
    # the same values as command-line strings and as Fractions of their decimal text
    as_text = tuple(str(v) for v in interval)
    assert guided_steps(as_text, steps) == want
    assert guided_steps(tuple(Fraction(s) for s in as_text), steps) == want
    assert guided_steps(parse_cfg_interval(",".join(as_text)), steps) == want


def test_the_window_is_the_definition_for_every_step():
    """j0 = ceil(lo S), j1 = ceil(hi S) is `lo S <= j < hi S` step by step, in exact rationals."""
    for S in (1, 3, 7, 10, 50, 1000):
        for lo_s, hi_s in (("0", "0"), ("0", "0.1"), ("0.1", "0.9"), ("0.3", "0.7"), ("0.35", "0.36"), ("0.999", "1"), ("1", "1")):
            lo, hi = Fraction(lo_s), Fraction(hi_s)
            j0, j1 = guided_steps((float(lo_s), float(hi_s)), S)
            assert 0 <= j0 <= j1 <= S
            assert [j for j in range(S) if lo * S <= j < hi * S] == list(range(j0, j1)), (S, lo_s, hi_s)


def test_float_products_are_not_used():
    """Windows a ceil of the float product gets wrong: 0.07 * 100 = 7.000000000000001 -> 8, 0.56 * 25 = 14.000000000000002 -> 15."""
    import math
    assert math.ceil(0.07 * 100) == 8 and math.ceil(0.56 * 25) == 15
    assert guided_steps((0.07, 0.5), 100) == (7, 50)
    assert guided_steps((0.0, 0.56), 25) == (0, 14)
    assert guided_steps((0.3, 0.7), 1000) == (300, 700)


@pytest.mark.parametrize("interval", [(-0.1, 0.5), (0.0, 1.01), (0.6, 0.4), (1.5, 2.0), ("-0", "1.0000001"), (float("nan"), 1.0),
                                      (0.0, float("inf")), ("a", "1"), (0.5,), 0.5, (0.1, 0.2, 0.3), (True, 1), (None, 1)])
def test_guided_steps_refusals(interval):
    with pytest.raises(ValueError):
        guided_steps(interval, 10)


@pytest.mark.parametrize("steps", [0, -3])
def test_guided_steps_refuses_an_empty_loop(steps):
    with pytest.raises(ValueError, match="steps"):
        guided_steps((0, 1), steps)


def test_resolve_cfg_interval_names_the_directory():
    assert resolve_cfg_interval(None, 100) == (None, "")
    assert resolve_cfg_interval("0,1", 100) == ((0, 100), "")            # the whole loop: today's run, today's directory
    assert resolve_cfg_interval("0.2,0.8", 100) == ((20, 80), "_gi20-80")
    assert resolve_cfg_interval(" 0.3 , 0.7 ", 1000) == ((300, 700), "_gi300-700")
    assert resolve_cfg_interval("0.5,0.5", 10) == ((5, 5), "_gi5-5")
    for bad in ("0.2", "0.2,0.8,1", "0.2;0.8", "", "lo,hi", "0.8,0.2", "0,1.5"):
        with pytest.raises(ValueError):
            resolve_cfg_interval(bad, 100)


# ---------------------------------------------------------------------------------------------- infer.py
def _infer_args(*argv):
    import infer
    return infer.build_parser().parse_args(list(argv))


def test_infer_without_the_flag_changes_nothing():
    import infer
    a = _infer_args()
    assert a.cfg_interval is None
    cells = infer.parse_cells(a)
    assert a.guide_steps is None
    assert [c.path for c in cells] == [os.path.join("./results/denoiser_results", "generation", "flowmatching_DiT_exchangerate_24_7_100")]
    a = _infer_args("--backbone", "ddpm", "--total_step", "1000", "--solver", "dpmpp2m", "--sample_steps", "50")
    assert os.path.basename(infer.parse_cells(a)[0].path) == "ddpm_DiT_exchangerate_24_7_1000_dpmpp2m50" and a.guide_steps is None


def test_infer_cfg_interval_window_and_suffix():
    import infer
    a = _infer_args("--cfg_interval", "0.2,0.8")
    cells = infer.parse_cells(a)
    assert a.guide_steps == (20, 80)
    assert os.path.basename(cells[0].path) == "flowmatching_DiT_exchangerate_24_7_100_gi20-80"
    # the whole loop keeps today's directory, and the sampler gets the whole window
    a = _infer_args("--cfg_interval", "0,1")
    assert os.path.basename(infer.parse_cells(a)[0].path) == "flowmatching_DiT_exchangerate_24_7_100" and a.guide_steps == (0, 100)
    # every cell of a grid job, after the solver suffix, in loop indices of the solver's S
    a = _infer_args("--backbone", "ddpm", "--total_step", "1000", "--solver", "dpmpp2m", "--sample_steps", "50",
                    "--dataset_name", "ETTh1_24,ETTh1_96", "--cfg_scale", "5,9", "--cfg_interval", "0.25,0.75")
    paths = [os.path.basename(c.path) for c in infer.parse_cells(a)]
    assert a.guide_steps == (13, 38)
    assert paths == ["ddpm_DiT_ETTh1_24_5.0_1000_dpmpp2m50_gi13-38", "ddpm_DiT_ETTh1_24_9.0_1000_dpmpp2m50_gi13-38",
                     "ddpm_DiT_ETTh1_96_5.0_1000_dpmpp2m50_gi13-38", "ddpm_DiT_ETTh1_96_9.0_1000_dpmpp2m50_gi13-38"]
    units = infer.grid_units(infer.parse_cells(a), 11, 3)
    assert units[1].path.endswith(os.path.join("ddpm_DiT_ETTh1_24_5.0_1000_dpmpp2m50_gi13-38", "run_0"))
    # ancestral DDPM at 1000 steps: the row a float product gets wrong
    a = _infer_args("--backbone", "ddpm", "--total_step", "1000", "--cfg_interval", "0.3,0.7")
    assert os.path.basename(infer.parse_cells(a)[0].path) == "ddpm_DiT_exchangerate_24_7_1000_gi300-700"
    # ddim without --sample_steps runs --total_step evaluations
    a = _infer_args("--backbone", "ddpm", "--total_step", "40", "--solver", "ddim", "--cfg_interval", "0.5,1")
    assert os.path.basename(infer.parse_cells(a)[0].path) == "ddpm_DiT_exchangerate_24_7_40_ddim40_gi20-40"


@pytest.mark.parametrize("argv,word", [
    (("--cfg_interval", "0.2,0.8", "--denoiser", "MLP", "--backbone", "ddpm"), "MLP"),
    (("--cfg_interval", "0,1", "--denoiser", "MLP", "--backbone", "ddpm"), "MLP"),
    (("--cfg_interval", "0.8,0.2"), "lo"),
    (("--cfg_interval", "0.2,1.2"), "hi"),
    (("--cfg_interval=-0.2,1",), "lo"),
    (("--cfg_interval", "0.5"), "LO,HI"),
    (("--cfg_interval", "x,1"), "not a number")])
def test_infer_refuses_with_a_message(argv, word):
    import infer
    with pytest.raises(ValueError, match=word):
        infer.parse_cells(_infer_args(*argv))
    with pytest.raises(SystemExit) as e:                   # main() exits with that message before it looks for a GPU
        infer.main(list(argv))
    assert isinstance(e.value.code, str) and word in e.value.code


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_the_two_entries_and_the_binding_lists_them():
    txt = open(os.path.join(REPO, "include", "t2s.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+t2s_sampler_set_guided_steps\s*\(\s*t2s_sampler\s*\*\s*s\s*,\s*int\s+first\s*,\s*int\s+end\s*\)\s*;", code)
    assert re.search(r"\bint\s+t2s_sampler_guided_steps\s*\(\s*const\s+t2s_sampler\s*\*\s*s\s*,\s*int\s*\*\s*first\s*,\s*int\s*\*\s*end\s*\)\s*;", code)
    import ctypes as C
    assert L.SYMBOLS["t2s_sampler_set_guided_steps"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int])
    res, args = L.SYMBOLS["t2s_sampler_guided_steps"]
    assert res is C.c_int and args[0] is C.c_void_p and args[1] is C.POINTER(C.c_int) and args[2] is C.POINTER(C.c_int)
    assert C.sizeof(L.SampleConfig) == 56                  # the window did not grow t2s_sample_config
    lib = L.lib()                                          # the built library exports them (AttributeError otherwise)
    assert hasattr(lib, "t2s_sampler_set_guided_steps") and hasattr(lib, "t2s_sampler_guided_steps")
    assert b"t2s 0.7 " in lib.t2s_version()
