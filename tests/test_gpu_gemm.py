"""GPU edges of the fp32 GEMM family (elliot_amd/csrc/el_gemm.hip): the generic k_gemm_f32 with split K and k_gemm_reduce, the aligned
persistent k_gemm_f32_v in its 16 instantiations with k_gemm_sk_fix behind it, the three-plane bf16 k_gemm_b3 in its four XCD orders
and the masked column-sum epilogue of el_gemm_f32_x.

Which form a call takes is decided on the host; tests/helpers/gemm_ref.py restates that decision (plan) and holds the case table.
test_case_table_reaches_every_branch_on_this_device asserts, with the device's own CU count, that the table reaches every branch in
gemm_ref.REQUIRED -- on a device with another CU count it fails and names the branch, it does not pass on fewer branches.  Where
kernel names can tell, every exact case checks the plan against the device (ctx.timing): k_gemm_b3 or k_gemm_f32 ran, and k_gemm_reduce
(the name k_gemm_sk_fix is timed under as well) exactly when the plan says so.  The names cannot tell the tile shape (tm, tn), the
schedule or the store epilogue of k_gemm_f32_v apart: that part rests on the restatement alone.

Exact cases: integer operands with every partial sum below 2^24 -- every correct summation order on every family gives the same bits,
so the result must EQUAL the exact product: a product dropped or counted twice at a tile edge, a k tail, a cut tile or a split shows
whatever the size of the entry it lands on.  Operands are views with leading dimensions above the extent into NaN-filled buffers
(a read of the padding that reaches a product poisons the result), C is a view into a buffer of sentinels that must survive around
it, the workspace has sentinel bands on both sides, and every case runs twice for the same bits.

Rounding cases, measured on an MI355X (256 CUs).  e = |got - fp64| / (|A| @ |B|) entry-wise; the ratios are the device's e over that of
NumPy's float32 product of the same operands, (max ratio, rms ratio), the larger of the N(0,1) and the 12-decade data:
    generic k_gemm_f32          one K range (1.000, 1.000)   8 K splits + k_gemm_reduce (0.645, 0.695)
    k_gemm_f32_v                whole 64 x 64 tiles (1.000, 1.001)   stream-K, 17 partial tiles per tile (0.527, 0.698)
                                2052 x 2052 x 256, tiles cut once or twice (0.843, 0.729)
    k_gemm_b3, no K split       516 x 7940 x 248 (1.093, 1.273)   7940 x 516 x 248 transposed (1.340, 1.275)
    k_gemm_b3, K split          64 splits (1.112, 1.309)   61 splits, plain grid (1.180, 1.314)
The largest is 1.340, so M_MARGIN = 4: the smallest power of two that is at least twice it.  (The hard gate (K + 4) 2^-24 |A| @ |B| is
used to 17 % at most, at K = 36.)
Epilogues, the six places x four activations: the worst |got - act64(ref + bias)| is 0.105 of the allowed bound (pre-activation gate
+ 4 * 2^-24 |out|); no entry needs the 4 * 2^-24 |out| on top of the pre-activation gate, which is why the activation is also
measured ALONE, against the fp64 activation of the device's own fp32 pre-activation: tanhf is within 2.49, the expf sigmoid within
2.19 times 2^-24 |out| in every place -- the allowance of 4 holds with nothing of the product's round-off to hide behind."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from elliot_amd import _lib, ops
from tests.gpu_util import cpu
from tests.helpers import gemm_ref as gr

pytestmark = pytest.mark.gpu

SENT = 0x7FC0BEEF                 # a quiet NaN no kernel produces
BAND = 4096
U24 = 2.0 ** -24
M_MARGIN = 4
CASES = gr.exact_cases()


# ---- buffers -------------------------------------------------------------------------------------------------------------------------
def _guard(ld):
    return (2 * ld + 3) // 4 * 4 + 4


def put(host, ld, off, dev):
    """host [R, ext] as a view with leading dimension ld, `off` floats behind a 16-byte boundary, inside a buffer of NaN."""
    R, ext = host.shape
    start = _guard(ld) + off
    buf = torch.full((start + R * ld + _guard(ld),), float("nan"), dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    if R:
        buf[start:start + R * ld].view(R, ld)[:, :ext].copy_(torch.from_numpy(np.ascontiguousarray(host)))
    return buf, buf.data_ptr() + 4 * start


class Out:
    """C [M, N] with leading dimension ldc inside a buffer of sentinels: two rows' worth in front and behind, the row padding between."""

    def __init__(self, M, N, ldc, off, dev):
        self.M, self.N, self.ldc = M, N, ldc
        self.start = _guard(ldc) + off
        self.buf = torch.full((self.start + M * ldc + _guard(ldc),), SENT, dtype=torch.int32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + 4 * self.start

    def inner(self):
        return self.buf[self.start:self.start + self.M * self.ldc].view(self.M, self.ldc)

    def result(self):
        return self.inner()[:, :self.N].contiguous().view(torch.float32)

    def assert_surroundings_intact(self, what):
        assert bool((self.buf[:self.start] == SENT).all()), f"{what}: written in front of C"
        assert bool((self.buf[self.start + self.M * self.ldc:] == SENT).all()), f"{what}: written behind C"
        if self.M:
            assert bool((self.inner()[:, self.N:] == SENT).all()), f"{what}: written into the padding of C's rows"

    def assert_untouched(self, what):
        assert bool((self.buf == SENT).all()), f"{what}: C was written"


class Ws:
    """`nbytes` of workspace between two bands of 0xA5 (tests/test_gpu_workspace_guard.py)."""

    def __init__(self, nbytes, dev):
        self.n = int(nbytes)
        self.raw = torch.full((self.n + 2 * BAND,), 0xA5, dtype=torch.uint8, device=dev)
        self.ptr = self.raw.data_ptr() + BAND

    def assert_bands_intact(self, what):
        assert bool((self.raw[:BAND] == 0xA5).all()), f"{what}: written in front of the workspace"
        assert bool((self.raw[BAND + self.n:] == 0xA5).all()), f"{what}: written behind the workspace ({self.n} bytes)"


def gemm_raw(ctx, tA, tB, M, N, K, a_ptr, lda, b_ptr, ldb, c_ptr, ldc, bias_ptr=None, act=0, ws_ptr=None, ws_bytes=0):
    """el_gemm_f32 as the library exports it: explicit leading dimensions, base addresses and workspace (ops.gemm takes contiguous
    tensors only).  Returns the status."""
    vp = lambda x: None if x is None else C.c_void_p(int(x))
    return ctx.lib.el_gemm_f32(ctx.handle, ctx.stream(), int(tA), int(tB), int(M), int(N), int(K), vp(a_ptr), int(lda), vp(b_ptr), int(ldb),
                               vp(c_ptr), int(ldc), vp(bias_ptr), int(act), vp(ws_ptr), int(ws_bytes))


def launch(ctx, c, A, B, bias=None, bias_off=0, act="none", ws="need", timed=False):
    """One call of case c (gemm_ref.case) on host operands in storage shape; ws: "need" (el_gemm_ws_bytes), a byte count, or None."""
    dev = ctx.device
    lda, ldb, ldc = gr.lds(c)
    abuf, a_ptr = put(A, lda, c.a_off, dev)
    bbuf, b_ptr = put(B, ldb, c.b_off, dev)
    out = Out(c.M, c.N, ldc, c.c_off, dev)
    bias_ptr = None
    if bias is not None:
        biasbuf, bias_ptr = put(bias.reshape(1, -1), c.N + 4, bias_off, dev)
    need = int(ctx.lib.el_gemm_ws_bytes(ctx.handle, c.M, c.N, c.K))
    assert need == gr.ws_bytes(ctx.cus, c.M, c.N, c.K)
    nbytes = need if ws == "need" else ws
    wsg = Ws(nbytes, dev) if nbytes is not None else None
    names = None
    if timed:
        ctx.timing(True)
        ctx.timing_report()
    try:
        rc = gemm_raw(ctx, c.tA, c.tB, c.M, c.N, c.K, a_ptr, lda, b_ptr, ldb, out.ptr, ldc, bias_ptr, gr.ACTS[act],
                      wsg.ptr if wsg else None, wsg.n if wsg else 0)
        torch.cuda.synchronize()
        if timed:
            names = ctx.timing_report()
    finally:
        if timed:
            ctx.timing(False)
    _lib.check(rc, "el_gemm_f32")
    out.assert_surroundings_intact(c.name)
    if wsg:
        wsg.assert_bands_intact(c.name)
    return SimpleNamespace(got=out.result(), out=out, names=names)


def assert_names_match_plan(names, p, what):
    other = "k_gemm_f32" if p.kernel == "k_gemm_b3" else "k_gemm_b3"
    assert p.kernel in names and other not in names, (what, p.kernel, sorted(names))
    assert ("k_gemm_reduce" in names) == bool(p.reduce), (what, "k_gemm_reduce", p.reduce, sorted(names))


def set_options(lib_option, c):
    lib_option("gemm_split", c.split)
    lib_option("gemm_xcd", c.xcd)


def bits(t):
    return t.view(torch.int32)


# ---- 1. the table reaches every branch -----------------------------------------------------------------------------------------------
def test_case_table_reaches_every_branch_on_this_device(ctx):
    missing = gr.missing(ctx.cus, CASES)
    assert not missing, f"with {ctx.cus} CUs the case table no longer reaches: {missing}"


# ---- 2. exact cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_integer_product_is_exact(ctx, lib_option, c):
    set_options(lib_option, c)
    p = gr.case_plan(ctx.cus, c)
    A, B = gr.int_operands(c)
    assert gr.exact_bound(c) < gr.EXACT
    ref = torch.from_numpy(gr.exact_product(A, B, c.tA, c.tB, f32=c.M * c.N > (1 << 24))).to(ctx.device)   # (asserts the 2^24 precondition)
    r1 = launch(ctx, c, A, B, timed=True)
    assert_names_match_plan(r1.names, p, c.name)
    if not torch.equal(r1.got, ref):
        bad = (r1.got != ref) | torch.isnan(r1.got)
        rows, cols = torch.nonzero(bad, as_tuple=True)
        raise AssertionError(f"{c.name} ({p.family}): {int(bad.sum())} of {c.M * c.N} entries differ from the exact product; first at "
                             f"({int(rows[0])}, {int(cols[0])}): got {float(r1.got[rows[0], cols[0]])}, exact {float(ref[rows[0], cols[0]])}; "
                             f"rows {int(rows.min())}..{int(rows.max())}, columns {int(cols.min())}..{int(cols.max())}")
    r2 = launch(ctx, c, A, B)
    assert torch.equal(bits(r1.got), bits(r2.got)), c.name


# ---- 3. rounding cases ---------------------------------------------------------------------------------------------------------------
ROUND = [gr.case("round-generic-split8", 70, 45, 1000, pad_a=1, pad_b=3), gr.case("round-generic", 5, 1030, 77, True, True, pad_a=3, pad_b=3),
         gr.case("round-v-whole64", 260, 260, 36, False, True), gr.case("round-v-fix17", 200, 132, 2052, True, False),
         gr.case("round-v-big", 2052, 2052, 256, split=0), gr.case("round-b3", 516, 7940, 248), gr.case("round-b3-TT", 7940, 516, 248, True, True),
         gr.case("round-b3-split64", 132, 260, 30716, False, True), gr.case("round-b3-split61", 132, 260, 29140, True, False)]
ROUND_FAMILY = {"round-generic-split8": "generic", "round-generic": "generic", "round-v-whole64": "v", "round-v-fix17": "v", "round-v-big": "v",
                "round-b3": "b3", "round-b3-TT": "b3", "round-b3-split64": "b3", "round-b3-split61": "b3"}


def float_operands(c, dist, scale=1.0):
    rs = np.random.RandomState(c.M + 3 * c.N + 5 * c.K + (17 if dist == "spread" else 0))
    sa, sb = ((c.K, c.M) if c.tA else (c.M, c.K)), ((c.N, c.K) if c.tB else (c.K, c.N))
    if dist == "spread":
        return gr.spread_operands(sa, sb, rs)
    return (rs.normal(size=sa) * scale).astype(np.float32), (rs.normal(size=sb) * scale).astype(np.float32)


@pytest.mark.parametrize("dist", ["normal", "spread"])
@pytest.mark.parametrize("c", ROUND, ids=[c.name for c in ROUND])
def test_rounding_is_fp32_grade(ctx, lib_option, c, dist):
    """Hard gate: |got - ref| <= (K + 4) 2^-24 (|A| @ |B|) entry-wise -- the forward bound of any fp32 fma dot product plus the three
    plane terms k_gemm_b3 leaves out.  Relative gate: the error is within M_MARGIN of that of NumPy's float32 product of the same
    operands (another correct fp32 order), max and rms."""
    set_options(lib_option, c)
    p = gr.case_plan(ctx.cus, c)
    assert p.family == ROUND_FAMILY[c.name], (c.name, p.family)
    A, B = float_operands(c, dist)
    a64, b64 = gr.op(A, c.tA).astype(np.float64), gr.op(B, c.tB).astype(np.float64)
    ref, mag = a64 @ b64, np.abs(a64) @ np.abs(b64)
    got = cpu(launch(ctx, c, A, B).got).astype(np.float64)
    err = np.abs(got - ref)
    e_gpu, e_np = err / mag, np.abs((gr.op(A, c.tA) @ gr.op(B, c.tB)).astype(np.float64) - ref) / mag
    rms = lambda e: float(np.sqrt((e ** 2).mean()))
    print(f"RATIO {c.name} {p.family} {dist}: max {e_gpu.max() / e_np.max():.3f} rms {rms(e_gpu) / rms(e_np):.3f} "
          f"(e_gpu max {e_gpu.max() / U24:.2f} ulp, e_np max {e_np.max() / U24:.2f} ulp, hard {float((err / ((c.K + 4) * U24 * mag)).max()):.4f})")
    assert bool((err <= (c.K + 4) * U24 * mag).all()), (c.name, dist, float((err / ((c.K + 4) * U24 * mag)).max()))
    assert e_gpu.max() <= max(M_MARGIN * e_np.max(), 4 * U24), (c.name, dist, float(e_gpu.max()), float(e_np.max()))
    assert rms(e_gpu) <= M_MARGIN * rms(e_np), (c.name, dist, rms(e_gpu), rms(e_np))


# ---- 4. bias + activation in the six places an epilogue lives -------------------------------------------------------------------------
# (place, case, bias offset in floats, family, what the plan must say)
PLACES = [
    ("v-float4", gr.case("ep-v-float4", 128, 196, 68), 1, lambda p: p.family == "v" and p.epilogue == "float4" and not p.sk_fix),
    ("v-float2", gr.case("ep-v-float2", 128, 196, 68, c_off=2), 1, lambda p: p.family == "v" and p.epilogue == "float2" and not p.sk_fix),
    ("v-scalar", gr.case("ep-v-scalar", 128, 196, 68, c_off=1), 1, lambda p: p.family == "v" and p.epilogue == "scalar" and not p.sk_fix),
    ("v-scalar-layout", gr.case("ep-v-scalar-NT", 260, 260, 36, False, True), 1, lambda p: p.family == "v" and p.epilogue == "scalar_layout"),
    ("sk-fix", gr.case("ep-sk-fix", 128, 196, 2052), 1, lambda p: p.family == "v" and p.sk_fix and p.finished_in_v == 0),
    ("sk-fix-scalar", gr.case("ep-sk-fix-scalar", 132, 200, 2052, True, True, c_off=1), 1, lambda p: p.family == "v" and p.sk_fix and p.finished_in_v == 0),
    ("reduce", gr.case("ep-reduce", 70, 45, 1000, pad_a=1, pad_b=3), 1, lambda p: p.family == "generic" and p.splits == 8),
    ("generic", gr.case("ep-generic", 70, 45, 33, pad_a=3, pad_b=3), 0, lambda p: p.family == "generic" and p.splits == 1),
    ("b3", gr.case("ep-b3", 516, 7940, 248), 0, lambda p: p.family == "b3" and p.splits == 1),
    ("b3-reduce", gr.case("ep-b3-reduce", 132, 260, 30716, False, True), 0, lambda p: p.family == "b3" and p.splits == 64),
    ("b3-falls-to-v", gr.case("ep-b3-bias-off1", 516, 7940, 248), 1, lambda p: p.family == "v" and p.sk_fix),
]


@pytest.mark.parametrize("place,c,bias_off,expect", PLACES, ids=[x[0] for x in PLACES])
def test_bias_and_activation_in_every_epilogue(ctx, lib_option, place, c, bias_off, expect):
    """act(ref + bias) in fp64 against the device, pre-activations O(1): the pre-activation gate of the rounding cases plus 4 ulp of the
    output for tanhf / expf (all three derivatives are at most 1)."""
    set_options(lib_option, c)
    p = gr.case_plan(ctx.cus, c, bias_off=bias_off)
    assert expect(p), (place, vars(p))
    A, B = float_operands(c, "normal", scale=float(c.K) ** -0.25)
    bias = np.random.RandomState(c.N).normal(size=c.N).astype(np.float32)
    a64, b64 = gr.op(A, c.tA).astype(np.float64), gr.op(B, c.tB).astype(np.float64)
    z, mag = a64 @ b64 + bias.astype(np.float64), np.abs(a64) @ np.abs(b64)
    pre = None
    for act in ("none", "tanh", "relu", "sigmoid"):
        r = launch(ctx, c, A, B, bias=bias, bias_off=bias_off, act=act, timed=(act == "none"))
        if act == "none":
            assert_names_match_plan(r.names, p, place)
            pre = cpu(r.got)
        else:
            # the activation alone: the runs repeat their bits, so `pre` is the very fp32 value the epilogue activates -- nothing of
            # the product's round-off hides an error of tanhf / expf here
            own = gr.act64(pre.astype(np.float64), act)
            if act == "relu":
                assert np.array_equal(cpu(r.got), own.astype(np.float32)), (place, act)
            else:
                ulp = np.abs(cpu(r.got).astype(np.float64) - own) / (U24 * np.abs(own))
                print(f"ACTIVATION {place} {act}: {float(ulp.max()):.3f} x 2^-24 |out| from the fp64 activation of the device's pre-activation")
                assert float(ulp.max()) <= 4.0, (place, act, float(ulp.max()))
        exp = gr.act64(z, act)
        bound = (c.K + 4) * U24 * mag + 4 * U24 * np.abs(exp)
        err = np.abs(cpu(r.got).astype(np.float64) - exp)
        print(f"EPILOGUE {place} {act}: worst error / bound {float((err / bound).max()):.4f}, "
              f"beyond the pre-activation gate {float(((err - (c.K + 4) * U24 * mag) / (U24 * np.abs(exp) + 1e-300)).max()):.2f} ulp of the output")
        assert bool((err <= bound).all()), (place, act, float((err / bound).max()))
        if act == "relu":
            assert bool((cpu(r.got) >= 0).all())


# ---- 5. degenerate calls and the workspace ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tA,tB", gr.TRANSPOSES, ids=[gr.tname(*t) for t in gr.TRANSPOSES])
@pytest.mark.parametrize("act", ["none", "tanh", "relu", "sigmoid"])
def test_k_zero_gives_the_activated_bias(ctx, tA, tB, act):
    c = gr.case("k0", 37, 52, 0, tA, tB)
    A, B = np.zeros((0, 37) if tA else (37, 0), np.float32), np.zeros((52, 0) if tB else (0, 52), np.float32)
    bias = np.linspace(-3, 3, 52).astype(np.float32)
    got = cpu(launch(ctx, c, A, B, bias=bias, act=act).got)
    exp = np.broadcast_to(gr.act64(bias.astype(np.float64), act), (37, 52))
    if act in ("none", "relu"):
        assert np.array_equal(got, exp.astype(np.float32))
    else:
        assert bool((np.abs(got - exp) <= 4 * U24 * np.abs(exp)).all())
    got = cpu(launch(ctx, c, A, B, act=act).got)
    assert np.array_equal(got, np.full((37, 52), gr.act64(np.float64(0.0), act), np.float32))


@pytest.mark.parametrize("M,N", [(0, 44), (44, 0), (0, 0)])
def test_an_empty_result_is_no_call(ctx, M, N):
    c = gr.case("empty", M, N, 36)
    A, B = np.ones((M, 36), np.float32), np.ones((36, N), np.float32)
    r = launch(ctx, c, A, B)                                   # (status 0: launch checks it)
    r.out.assert_untouched(f"M = {M}, N = {N}")


@pytest.mark.parametrize("tA,tB", gr.TRANSPOSES, ids=[gr.tname(*t) for t in gr.TRANSPOSES])
@pytest.mark.parametrize("M,N,K", [(1, 1, 36), (1, 44, 36), (44, 1, 36), (1, 1, 1), (1, 132, 2052), (4, 4, 4)])
def test_single_rows_and_columns(ctx, tA, tB, M, N, K):
    c = gr.case(f"thin-{M}-{N}-{K}", M, N, K, tA, tB, pad_a=4 - ((M if tA else K) % 4), pad_b=4 - ((K if tB else N) % 4))
    p = gr.case_plan(ctx.cus, c)
    A, B = gr.int_operands(c)
    ref = torch.from_numpy(gr.exact_product(A, B, tA, tB)).to(ctx.device)
    r = launch(ctx, c, A, B, timed=True)
    assert_names_match_plan(r.names, p, c.name)
    assert torch.equal(r.got, ref), (c.name, p.family)


def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    dev = ctx.device
    M, N, K = 40, 44, 36
    abuf, a_ptr = put(np.ones((M, K), np.float32), K, 0, dev)
    bbuf, b_ptr = put(np.ones((K, N), np.float32), N, 0, dev)
    ws = Ws(int(ctx.lib.el_gemm_ws_bytes(ctx.handle, M, N, K)), dev)
    out = Out(M, N, N, 0, dev)

    def refused(what, *args, **kw):
        rc = gemm_raw(ctx, *args, **kw, ws_ptr=ws.ptr, ws_bytes=ws.n)
        torch.cuda.synchronize()
        assert rc != 0, what
        with pytest.raises(_lib.ElliotHipError):
            _lib.check(rc, what)
        out.assert_untouched(what)

    refused("lda below K", False, False, M, N, K, a_ptr, K - 1, b_ptr, N, out.ptr, N)
    refused("lda below M (transposed)", True, False, K + 1, N, M, a_ptr, K, b_ptr, N, out.ptr, N)
    refused("ldb below N", False, False, M, N, K, a_ptr, K, b_ptr, N - 1, out.ptr, N)
    refused("ldb below K (transposed)", False, True, M, K, N + 1, a_ptr, N + 1, b_ptr, N, out.ptr, K)
    refused("ldc below N", False, False, M, N, K, a_ptr, K, b_ptr, N, out.ptr, N - 1)
    refused("activation 4", False, False, M, N, K, a_ptr, K, b_ptr, N, out.ptr, N, act=4)
    refused("activation -1", False, False, M, N, K, a_ptr, K, b_ptr, N, out.ptr, N, act=-1)
    refused("null A", False, False, M, N, K, None, K, b_ptr, N, out.ptr, N)
    refused("null B", False, False, M, N, K, a_ptr, K, None, N, out.ptr, N)
    refused("negative K", False, False, M, N, -1, a_ptr, K, b_ptr, N, out.ptr, N)
    assert gemm_raw(ctx, False, False, M, N, K, a_ptr, K, b_ptr, N, None, N, ws_ptr=ws.ptr, ws_bytes=ws.n) != 0, "null C"
    ws.assert_bands_intact("refused calls")
    assert gemm_raw(ctx, False, False, M, N, K, a_ptr, K, b_ptr, N, out.ptr, N, ws_ptr=ws.ptr, ws_bytes=ws.n) == 0
    torch.cuda.synchronize()
    assert bool((out.result() == float(K)).all())


WS_CASES = [("stream-k", gr.case("ws-stream-k", 128, 196, 2052)), ("generic-split", gr.case("ws-generic-split", 70, 45, 1000, pad_a=1, pad_b=3)),
            ("b3-split", gr.case("ws-b3-split", 132, 260, 30716, False, True))]


def ws_requirement(cus, c):
    """Bytes the form planned with a full workspace actually uses (el_gemm_ws_bytes is an upper bound of it)."""
    p = gr.case_plan(cus, c)
    if p.family == "v":
        pl = gr.gemm_plan(cus, c.M, c.N, c.K)
        return 2 * pl.P * (64 * pl.tm) * (64 * pl.tn) * 4
    return gr.gemm_splits(cus, c.M, c.N, c.K) * c.M * c.N * 4


@pytest.mark.parametrize("kind,c", WS_CASES, ids=[k for k, _ in WS_CASES])
@pytest.mark.parametrize("ws", ["need", "need-4", "use", "use-4", None])
def test_workspace_is_respected_and_a_short_one_falls_back(ctx, lib_option, kind, c, ws):
    """A workspace of exactly el_gemm_ws_bytes between sentinel bands stays inside them (launch checks the bands); four bytes fewer than
    the query names, four fewer than the chosen form uses, or none at all: the plan predicts the fallback -- k_gemm_b3 and the generic
    kernel without a K split, k_gemm_f32_v gives way to the generic kernel -- and the product of the integer operands stays exact."""
    set_options(lib_option, c)
    need, use = gr.ws_bytes(ctx.cus, c.M, c.N, c.K), ws_requirement(ctx.cus, c)
    assert use <= need
    have = {"need": need, "need-4": need - 4, "use": use, "use-4": use - 4, None: None}[ws]
    full, p = gr.case_plan(ctx.cus, c), gr.case_plan(ctx.cus, c, ws_bytes_=have)
    assert (full.family, full.reduce) == ({"stream-k": "v", "generic-split": "generic", "b3-split": "b3"}[kind], True)
    if ws in ("use-4", None):
        if kind == "stream-k":
            assert p.family == "generic" and (ws is not None or p.splits == 1), vars(p)
        else:
            assert p.family == full.family and p.splits == 1 and not p.reduce, vars(p)
    elif ws == "use" or use <= need - 4:
        assert (p.family, p.reduce, p.splits) == (full.family, True, full.splits)
    A, B = gr.int_operands(c)
    ref = torch.from_numpy(gr.exact_product(A, B, c.tA, c.tB)).to(ctx.device)
    r = launch(ctx, c, A, B, ws=have, timed=True)
    assert_names_match_plan(r.names, p, (kind, ws))
    assert torch.equal(r.got, ref), (kind, ws, p.family, p.splits)


@pytest.mark.parametrize("split", [1, 0])
def test_an_infinite_operand_is_nan_on_the_three_plane_kernel_and_infinite_on_the_fp32_one(ctx, lib_option, split):
    """A documented limit, pinned: the three-way split forms a1 = a - a0, which is inf - inf = NaN for an infinite a, so
    k_gemm_b3 turns the row of C that an infinite entry of A feeds into NaN; the fp32 matrix instruction (gemm_split = 0) gives the
    infinity of IEEE arithmetic.  Every other row stays the exact product on both."""
    c = gr.case("inf", 516, 7940, 248, split=split)
    lib_option("gemm_split", split)
    assert gr.case_plan(ctx.cus, c).family == ("b3" if split else "v")
    A, B = gr.int_operands(c)
    B = np.abs(B) + 1.0                                                    # every product with the infinity has its sign
    A[3, 5], A[130, 247] = 0.0, 0.0
    ref = torch.from_numpy(gr.exact_product(A, B, False, False)).to(ctx.device)
    A[3, 5], A[130, 247] = np.inf, -np.inf
    got = launch(ctx, c, A, B).got
    finite = torch.ones(c.M, dtype=torch.bool, device=ctx.device)
    finite[3] = finite[130] = False
    assert torch.equal(got[finite], ref[finite])
    if split:
        assert bool(torch.isnan(got[3]).all()) and bool(torch.isnan(got[130]).all())
    else:
        assert bool((got[3] == float("inf")).all()) and bool((got[130] == float("-inf")).all())


# ---- 6. the masked column-sum epilogue on ragged tiles --------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [1, 0])
def test_masked_colsum_epilogue_on_ragged_tiles(ctx, lib_option, split):
    """el_gemm_f32_x through NmfDeviceState.grads (tests/test_gpu_neumf.py: test_neumf_step_at_d128_matches_oracle, its gates unchanged):
    one batch of n = 7601 rows (59 row tiles and one of 49 rows), no dropout, a tower (516, 256, 64): the input gradient of the layer
    with 256 units is a [7601, 516] x K = 256 product (four column tiles and one of 4 columns) of 2.008 GFLOP -- with gemm_split = 1
    it runs on k_gemm_b3 with the ReLU mask of the layer below and that layer's bias gradient in its epilogue, with 0 on k_gemm_f32_v
    followed by k_relu_bwd_colsum.  Checked against the fp64 oracle under the device's ReLU pattern: every gradient tensor -- the
    lower layer's gb and gW and the embedding gradients fed through din among them; the run repeats its bits."""
    from oracle import neumf as on
    from tests.test_gpu_neumf import _relu_branch_audit
    lib_option("gemm_split", split)
    U, I, F, n = 300, 200, 16, 7601
    units = [516, 256, 64]
    assert 2.0 * n * units[0] * units[1] >= gr.FLOP_B3 and n % 128 == 49 and units[0] % 128 == 4
    p = gr.plan(ctx.cus, n, units[0], units[1], False, True, gr.align(units[1], units[1], units[0]), 1 << 40, bool(split))
    assert p.family == ("b3" if split else "v") and p.splits == 1
    w0 = on.init_neumf(U, I, F, 3, units=units)
    rs = np.random.RandomState(5)
    for l in range(3):
        w0["b"][l] = rs.normal(scale=0.05, size=units[l]).astype(np.float32)
    u = rs.randint(0, U, n).astype(np.int32)
    i = (rs.zipf(1.2, n) % I).astype(np.int32)
    y = rs.randint(0, 2, n).astype(np.float32)
    d = ctx.device
    names = ["Umf", "Imf", "Umlp", "Imlp"]

    def run(timed=False):
        st = ops.NmfDeviceState(ctx, w0, max_batch=n)
        rep = None
        if timed:
            ctx.timing(True)
            ctx.timing_report()
        try:
            st.grads(torch.from_numpy(u).to(d), torch.from_numpy(i).to(d), torch.from_numpy(y).to(d))
            loss = st.pop_loss()
            torch.cuda.synchronize()
            if timed:
                rep = ctx.timing_report()
        finally:
            if timed:
                ctx.timing(False)
        g = {k: cpu(t) for k, t in zip(names, st.gtab)}
        g.update({"hw": cpu(st.ghw), "hb": cpu(st.ghb)})
        for l in range(3):
            g["W", l], g["b", l] = cpu(st.gW[l]), cpu(st.gb[l])
        return st, loss, g, rep

    st, got_loss, got, _ = run()
    u64, i64 = u.astype(np.int64), i.astype(np.int64)
    masks, flips = _relu_branch_audit(st, w0, n)
    for (l, z, bound) in flips:
        assert z <= bound, (l, z, bound)
    assert len(flips) <= 24, [(l, z) for l, z, _ in flips]
    c64 = on.forward(w0, u64, i64, dtype=np.float64)
    exp_loss = float(on.bce(c64["p"], y.astype(np.float64)))
    assert abs(got_loss - exp_loss) <= 1e-4 * abs(exp_loss), (got_loss, exp_loss)
    g64 = on.gradients(w0, c64, u64, i64, y.astype(np.float64), relu_masks=masks)
    g32 = on.gradients(w0, on.forward(w0, u64, i64), u64, i64, y, relu_masks=masks)

    def close(a, b32, b64, what):
        b64 = np.asarray(b64, np.float64).reshape(a.shape)
        scale = float(np.abs(b64).max())
        own = float(np.sqrt(np.mean((np.asarray(b32, np.float64).reshape(a.shape) - b64) ** 2))) / scale
        tol = max(2e-5, 64 * own) * scale
        err = np.abs(a - b64)
        assert float((err > tol).mean()) <= 1e-3 and float(err.max()) <= 0.05 * scale, \
            (split, what, float((err > tol).mean()), float(err.max()), tol, scale, len(flips))

    for k in names + ["hw", "hb"]:
        close(got[k], g32[k], g64[k], k)
    for l in range(3):
        close(got["W", l], g32["W"][l], g64["W"][l], ("W", l))
        close(got["b", l], g32["b"][l], g64["b"][l], ("b", l))
    # the same bits again; and, on one stream so that every launch is timed in order, the kernels the plan names
    _, loss2, again, _ = run()
    for k, v in got.items():
        assert np.array_equal(v.view(np.uint32), again[k].view(np.uint32)), (split, k)
    lib_option("nmf_side", 0)
    _, _, one_stream, rep = run(timed=True)
    assert ("k_gemm_b3" in rep) == bool(split), sorted(rep)
    assert rep["k_relu_bwd_colsum"][0] == (1 if split else 2), rep.get("k_relu_bwd_colsum")
    for k in (("b", 0), ("W", 0), ("W", 1), "Umlp", "Imlp"):
        close(one_stream[k], g32[k[0]][k[1]] if isinstance(k, tuple) else g32[k], g64[k[0]][k[1]] if isinstance(k, tuple) else g64[k], k)
