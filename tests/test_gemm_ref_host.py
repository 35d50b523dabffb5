"""CPU checks of tests/helpers/gemm_ref.py: the case table of tests/test_gpu_gemm.py reaches every branch of the el_gemm_f32 dispatch
on a 256-CU device, its integer cases keep every partial sum below 2^24 and its k_gemm_b3 cases are large enough to reach that kernel."""
import numpy as np
import pytest

from tests.helpers import gemm_ref as gr

CUS = 256
CASES = gr.exact_cases()


def test_case_table_reaches_every_branch_at_256_cus():
    assert len(set(gr.REQUIRED)) == len(gr.REQUIRED) == 44
    assert gr.missing(CUS, CASES) == []
    assert len({c.name for c in CASES}) == len(CASES)


def test_a_table_without_a_branch_is_named():
    """The coverage check can fail: without the long-K stream-K cases the eight-at-a-time loop of k_gemm_sk_fix is reported, and with a
    CU count that splits K another way the plain-grid split of k_gemm_b3 is."""
    assert gr.missing(CUS, [c for c in CASES if c.K != 2052]) == ["fix:gt10"]
    assert "b3:split:plain" in gr.missing(64, CASES)


def test_every_exact_case_keeps_partial_sums_below_2_to_24():
    for c in CASES:
        assert gr.exact_bound(c) < gr.EXACT, c.name
        A, B = gr.int_operands(c)
        assert float(np.abs(A).max()) <= c.amax and float(np.abs(B).max()) <= c.bmax
        assert np.array_equal(A, np.rint(A)) and np.array_equal(B, np.rint(B))
        # integers this small sit in the bf16 planes without a remainder: one plane up to 255, two below 65536
        assert gr.planes_needed(c.amax) <= 2 and gr.planes_needed(c.bmax) <= 2


def test_every_b3_case_is_at_or_above_2_gflop_and_planned_on_b3():
    b3 = [c for c in CASES if c.name.startswith("b3-")]
    assert len(b3) >= 8
    for c in b3:
        assert 2.0 * c.M * c.N * c.K >= gr.FLOP_B3, c.name
        assert gr.case_plan(CUS, c).family == "b3", c.name
    for c in CASES:
        if not c.name.startswith("b3-"):
            assert gr.case_plan(CUS, c).family != "b3", c.name


def test_plan_restates_the_documented_shapes():
    """Shapes whose schedule the kernel file's comments state."""
    al = lambda M, N, K, tA=False, tB=False: gr.align(M if tA else K, K if tB else N, N)
    need = gr.ws_bytes(CUS, 512, 600, 26744)
    assert gr.gemm_splits(CUS, 512, 600, 26744) == 24                      # 20 tiles: 512 / 20 = 25 -> a multiple of 8
    p = gr.plan(CUS, 512, 600, 26744, False, True, al(512, 600, 26744, False, True), need)
    assert (p.family, p.splits, p.grp_mode, p.reduce) == ("b3", 24, 3, True)
    p = gr.plan(CUS, 512, 26744, 600, False, False, al(512, 26744, 600), gr.ws_bytes(CUS, 512, 26744, 600))
    assert (p.family, p.splits, p.grp_mode, p.ngroups_mod8) == ("b3", 1, 1, 209 % 8)
    p = gr.plan(CUS, 512, 400, 600, False, False, al(512, 400, 600), gr.ws_bytes(CUS, 512, 400, 600))
    assert (p.family, p.tm, p.tn, p.whole_tiles, p.sk_fix) == ("v", 1, 1, 1, False)       # the latency-bound class: whole 64 x 64 tiles
    p = gr.plan(CUS, 512, 26744, 600, False, False, al(512, 26744, 600), gr.ws_bytes(CUS, 512, 26744, 600), split_on=False)
    assert (p.family, p.tm, p.tn, p.whole_tiles) == ("v", 2, 2, 0)            # 26 744 = 209 x 128 - 8: nothing to gain from 64-wide tiles
    assert gr.ws_bytes(CUS, 128, 128, 64) == 2 * CUS * 2 * 128 * 128 * 4


@pytest.mark.parametrize("ws,family,splits", [("need", "v", 1), (None, "generic", 1), (100, "generic", 1)])
def test_plan_falls_back_without_workspace(ws, family, splits):
    c = gr.case("x", 128, 196, 2052)
    p = gr.case_plan(CUS, c, ws_bytes_=ws)
    assert (p.family, p.splits) == (family, splits)


def test_plan_names_the_store_epilogue():
    for c_off, pad_c, ep in ((0, 4, "float4"), (2, 4, "float2"), (0, 6, "float2"), (1, 4, "scalar"), (0, 5, "scalar"), (3, 4, "scalar")):
        assert gr.case_plan(CUS, gr.case("x", 128, 196, 68, c_off=c_off, pad_c=pad_c)).epilogue == ep, (c_off, pad_c)
    assert gr.case_plan(CUS, gr.case("x", 128, 196, 68, False, True)).epilogue == "scalar_layout"
    assert gr.case_plan(CUS, gr.case("x", 516, 7940, 248), bias_off=1).family == "v"
    assert gr.case_plan(CUS, gr.case("x", 516, 7940, 248), bias_off=0).family == "b3"
    assert gr.case_plan(CUS, gr.case("x", 516, 7940, 248, c_off=2)).family == "v"
