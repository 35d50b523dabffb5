"""The host dispatch of el_gemm_f32 (elliot_amd/csrc/el_gemm.hip: gemm_splits, gemm_plan, el_gemm_ws_bytes and the branch in
el_gemm_f32_x) restated in Python, the case table of tests/test_gpu_gemm.py and the coverage it has to prove.

plan() tells, for a call, which kernel family runs and in which form -- the tile shape of k_gemm_f32_v, its schedule, whether
k_gemm_sk_fix follows and how many partial tiles the busiest cut tile adds, the K splits of the generic kernel and of k_gemm_b3, the
XCD order of the latter, which store epilogue of k_gemm_f32_v a finished tile takes.  coverage() turns the plans of a case list into
branch labels; REQUIRED lists the labels the case table must reach.  The CPU test checks that for 256 CUs, the GPU module for the
device's own CU count: on a device where a shape no longer reaches its branch the assertion names the branch.

No device, no torch: NumPy only."""
from types import SimpleNamespace

import numpy as np

GBM = GBN = 128
GBK = KB = B3_BK = 32
FLOP_B3 = 2.0e9                # products at or above this run on k_gemm_b3 (option gemm_split)
EXACT = 2 ** 24

ACTS = {"none": 0, "tanh": 1, "relu": 2, "sigmoid": 3}
TRANSPOSES = ((False, False), (False, True), (True, False), (True, True))


def tname(tA, tB):
    return ("T" if tA else "N") + ("T" if tB else "N")


def cdiv(a, b):
    return (a + b - 1) // b


def gemm_splits(cus, M, N, K):
    tiles = cdiv(M, GBM) * cdiv(N, GBN)
    target = cus * 2
    if tiles >= target // 2 or K < 4 * GBK:
        return 1
    s = min(target // tiles, K // (2 * GBK), 64)
    if s >= 8:
        s &= ~7
    return max(s, 1)


def gemm_plan(cus, M, N, K):
    def waste(X, b):
        return float(cdiv(X, b) * b) / float(X)
    tm = 1 if waste(M, 128) > 1.12 * waste(M, 64) else 2
    tn = 1 if waste(N, 128) > 1.12 * waste(N, 64) else 2
    mode = -1
    if 2.0 * M * N * K < FLOP_B3 and cdiv(M, 64) * cdiv(N, 64) >= 16:
        tm = tn = 1
        mode = 1
    bm, bn = 64 * tm, 64 * tn
    nkt = max(cdiv(K, KB), 1)
    tiles_n = cdiv(N, bn)
    tiles = cdiv(M, bm) * tiles_n
    units = tiles * nkt
    P = cus * 2
    whole = mode if mode >= 0 else (1 if tiles >= 8 * P else 0)
    if whole:
        P = min(P, tiles)
    else:
        P = min(P, cdiv(units, 4))
    P = max(P, 1)
    return SimpleNamespace(tm=tm, tn=tn, P=P, whole_tiles=whole, nkt=nkt, tiles_n=tiles_n, tiles=tiles, units=units)


def ws_bytes(cus, M, N, K):
    s1 = gemm_splits(cus, M, N, K)
    generic = s1 * M * N * 4 if s1 > 1 else 0
    return max(generic, 2 * cus * 2 * 128 * 128 * 4)


def contributors(pl):
    """Stream-K: per output tile, the number of persistent workgroups whose unit range holds a part of its k tiles (1: finished in
    k_gemm_f32_v itself; more: one partial tile each, added by k_gemm_sk_fix)."""
    out = []
    for t in range(pl.tiles):
        ua, ub = t * pl.nkt, t * pl.nkt + pl.nkt - 1
        wa, wb = ((ua + 1) * pl.P - 1) // pl.units, ((ub + 1) * pl.P - 1) // pl.units
        out.append(wb - wa + 1)
    return out


def align(lda, ldb, ldc, a_off=0, b_off=0, c_off=0, bias_off=None):
    """Leading dimensions and the offsets (in floats) of each base from a 16-byte boundary; bias_off None: no bias."""
    return SimpleNamespace(lda=lda, ldb=ldb, ldc=ldc, a_off=a_off, b_off=b_off, c_off=c_off, bias_off=bias_off)


def plan(cus, M, N, K, tA, tB, alignments, ws_bytes, split_on=True, xcd_on=True):
    """What el_gemm_f32 does with this call (M, N >= 1).  ws_bytes None: no workspace."""
    al = alignments
    extA, extB = (M if tA else K), (K if tB else N)
    vecA = al.a_off % 4 == 0 and al.lda % 4 == 0
    vecB = al.b_off % 4 == 0 and al.ldb % 4 == 0
    fast0 = vecA and vecB and K >= 1 and extA % 4 == 0 and extB % 4 == 0
    pl = gemm_plan(cus, M, N, K)
    have = -1 if ws_bytes is None else ws_bytes
    fast = fast0 and have >= 2 * pl.P * (64 * pl.tm) * (64 * pl.tn) * 4
    outvec = N % 4 == 0 and al.ldc % 4 == 0 and al.c_off % 4 == 0 and (al.bias_off is None or al.bias_off % 4 == 0)
    out = SimpleNamespace(family=None, kernel="k_gemm_f32", tm=None, tn=None, whole_tiles=None, sk_fix=False, max_contrib=1,
                          min_cut_contrib=None, finished_in_v=0, splits=1, kchunk=None, last_chunk=None, grp_mode=None,
                          ngroups_mod8=None, grid=None, epilogue=None, reduce=False, tA=tA, tB=tB, M=M, N=N, K=K, fast0=fast0)

    def split_k(bk):
        s = gemm_splits(cus, M, N, K)
        if s > 1 and have < s * M * N * 4:
            s = 1
        kchunk = max(cdiv(cdiv(K, s), bk) * bk, bk)
        s = max(cdiv(K, kchunk), 1)
        out.splits, out.kchunk = s, kchunk
        out.last_chunk = K - (s - 1) * kchunk
        out.reduce = s > 1

    if split_on and fast0 and outvec and 2.0 * M * N * K >= FLOP_B3:
        out.family, out.kernel = "b3", "k_gemm_b3"
        split_k(B3_BK)
        gx, gy, gz = cdiv(N, 128), cdiv(M, 128), out.splits
        out.grid = (gx, gy, gz)
        out.grp_mode = 0
        if xcd_on and gx * gy * gz >= 16:
            ngroups = 0
            if gz > 1:
                if gz % 8 == 0 and gx * gy <= 64:
                    out.grp_mode, ngroups = 3, gz
            elif gy <= gx and gy <= 64:
                out.grp_mode, ngroups = 1, gx * gz
            elif gx <= 64:
                out.grp_mode, ngroups = 2, gy * gz
            if out.grp_mode:
                out.ngroups_mod8 = ngroups % 8
    elif fast:
        out.family = "v"
        out.tm, out.tn, out.whole_tiles = pl.tm, pl.tn, pl.whole_tiles
        per = contributors(pl) if not pl.whole_tiles else [1] * pl.tiles
        out.sk_fix = (not pl.whole_tiles) and (pl.units % pl.P != 0 or (pl.units // pl.P) % pl.nkt != 0)
        cut = [c for c in per if c > 1]
        assert out.sk_fix or not cut
        out.max_contrib = max(per)
        out.min_cut_contrib = min(cut) if cut else None
        out.finished_in_v = sum(1 for c in per if c == 1)
        out.reduce = out.sk_fix                          # (k_gemm_sk_fix is timed under the name k_gemm_reduce)
        if out.finished_in_v:
            wide = (not tB) and pl.tn == 2               # a lane holds two adjacent columns
            if wide and al.ldc % 4 == 0 and al.c_off % 4 == 0:
                out.epilogue = "float4"
            elif wide and al.ldc % 2 == 0 and al.c_off % 2 == 0:
                out.epilogue = "float2"
            else:
                out.epilogue = "scalar" if wide else "scalar_layout"
    else:
        out.family = "generic"
        split_k(GBK)
    return out


# ---- the case table ----------------------------------------------------------------------------------------------------------------
# One row: shape, transposes, the library options, how the three matrices sit in their buffers and what the integer operands may hold.
#   pad_a / pad_b / pad_c   floats added to the extent for the leading dimension (the padding holds NaN / the sentinel)
#   a_off / b_off / c_off   floats between a 16-byte boundary and the base
#   amax, bmax              |a| <= amax, |b| <= bmax, integers: K amax bmax < 2^24, so every partial sum is exact in fp32; on k_gemm_b3
#                           |v| <= 255 lives in the first bf16 plane alone, |v| < 4096 in the first two
def case(name, M, N, K, tA=False, tB=False, split=1, xcd=1, pad_a=4, pad_b=8, pad_c=4, a_off=0, b_off=0, c_off=0, amax=63, bmax=8):
    return SimpleNamespace(name=name, M=M, N=N, K=K, tA=tA, tB=tB, split=split, xcd=xcd, pad_a=pad_a, pad_b=pad_b, pad_c=pad_c,
                           a_off=a_off, b_off=b_off, c_off=c_off, amax=amax, bmax=bmax)


def lds(c):
    extA, extB = (c.M if c.tA else c.K), (c.K if c.tB else c.N)
    return extA + c.pad_a, extB + c.pad_b, c.N + c.pad_c


def case_plan(cus, c, bias_off=None, ws_bytes_="need"):
    lda, ldb, ldc = lds(c)
    have = ws_bytes(cus, c.M, c.N, c.K) if ws_bytes_ == "need" else ws_bytes_
    return plan(cus, c.M, c.N, c.K, c.tA, c.tB, align(lda, ldb, ldc, c.a_off, c.b_off, c.c_off, bias_off), have, bool(c.split), bool(c.xcd))


SK_SHAPES = {(2, 1): (200, 132), (1, 2): (132, 200), (2, 2): (128, 196), (1, 1): (132, 132)}


def exact_cases():
    cs = []
    for tA, tB in TRANSPOSES:
        t = tname(tA, tB)
        # generic family, each cause of leaving the fast path alone; with and without a K split
        cs.append(case(f"generic-odd-lda-{t}", 72, 44, 36, tA, tB, pad_a=1))
        cs.append(case(f"generic-extent-{t}", 70, 45, 33, tA, tB, pad_a=(2 if tA else 3), pad_b=3))
        cs.append(case(f"generic-base-{t}", 72, 44, 36, tA, tB, a_off=1))
        cs.append(case(f"generic-wide-{t}", 5, 1030, 77, tA, tB, pad_a=3, pad_b=(3 if tB else 2)))
        cs.append(case(f"generic-split8-{t}", 70, 45, 1000, tA, tB, pad_a=(2 if tA else 1), pad_b=(0 if tB else 3)))
        # k_gemm_f32_v: 64 x 64 whole tiles; the four tile shapes on the stream-K schedule, short K (a tile has one or two
        # contributors) and long K (many)
        cs.append(case(f"v-whole64-{t}", 260, 260, 36, tA, tB))
        for (tm, tn), (M, N) in SK_SHAPES.items():
            cs.append(case(f"v-sk{tm}{tn}-k68-{t}", M, N, 68, tA, tB))
            cs.append(case(f"v-sk{tm}{tn}-k2052-{t}", M, N, 2052, tA, tB))
    # the three store epilogues of k_gemm_f32_v (B stored [K, N], 128-wide tiles) and the two of k_gemm_sk_fix
    cs.append(case("v-ep-float2-c2", 128, 196, 68, c_off=2))
    cs.append(case("v-ep-scalar-c1", 128, 196, 68, c_off=1))
    cs.append(case("v-ep-scalar-oddldc", 128, 196, 68, pad_c=5))
    cs.append(case("v-ep-float2-ldc2", 132, 200, 68, pad_c=6))
    cs.append(case("v-fix-scalar-c1", 128, 196, 2052, c_off=1))
    cs.append(case("v-fix-scalar-oddldc", 132, 200, 2052, pad_c=3))
    # >= 2 GFLOP on the fp32 instruction: every 128 x 128 tile cut once or twice
    cs.append(case("v-big-cut12", 2052, 2052, 256, split=0, amax=4095, bmax=15))
    # whole 128 x 128 tiles by count (>= 8 per persistent workgroup)
    cs.append(case("v-whole128", 8196, 8196, 16, split=0, amax=4095, bmax=15))
    # k_gemm_b3: the four XCD orders, the four storage orders, K splits, a ragged last K chunk; a second plane on either side
    cs.append(case("b3-grp1-NN", 516, 7940, 248, amax=4095, bmax=15))
    cs.append(case("b3-grp1-NT", 516, 7940, 248, False, True, amax=15, bmax=4095))
    cs.append(case("b3-grp2-TN", 7940, 516, 248, True, False, amax=15, bmax=4095))
    cs.append(case("b3-grp2-TT", 7940, 516, 248, True, True, amax=4095, bmax=15))
    cs.append(case("b3-grp3-NT", 132, 260, 30716, False, True))
    cs.append(case("b3-grp3-TN", 132, 260, 30716, True, False))
    cs.append(case("b3-split61-TT", 132, 260, 29140, True, True))
    cs.append(case("b3-split61-NN", 132, 260, 29140))
    cs.append(case("b3-grp0-size", 8196, 8196, 16, amax=4095, bmax=15))
    cs.append(case("b3-noxcd", 516, 7940, 248, xcd=0, amax=255, bmax=15))
    return cs


V_LABELS = [f"v:{tname(tA, tB)}:{tm}{tn}" for tA, tB in TRANSPOSES for tm in (1, 2) for tn in (1, 2)]
REQUIRED = (
    [f"generic:{tname(*t)}" for t in TRANSPOSES] + ["generic:cause:odd-lda", "generic:cause:extent", "generic:cause:base",
                                                    "generic:split", "generic:nosplit"]
    + V_LABELS + ["v:whole-tiles", "v:stream-k", "fix:short", "fix:le2", "fix:gt10", "ep:float4", "ep:float2", "ep:scalar:c-off1",
                  "ep:scalar:odd-ldc"]
    + [f"b3:{tname(*t)}" for t in TRANSPOSES] + ["b3:grp1:ragged", "b3:grp2:ragged", "b3:grp3", "b3:grp0:size", "b3:split:plain",
                                                 "b3:ktail"])


def labels(c, p):
    """Branch labels one case reaches under plan p."""
    out = set()
    t = tname(c.tA, c.tB)
    lda, ldb, ldc = lds(c)
    if p.family == "generic":
        out.add(f"generic:{t}")
        out.add("generic:split" if p.splits > 1 else "generic:nosplit")
        extA, extB = (c.M if c.tA else c.K), (c.K if c.tB else c.N)
        causes = []
        if lda % 4 or ldb % 4:
            causes.append("odd-lda")
        if extA % 4 or extB % 4:
            causes.append("extent")
        if c.a_off % 4 or c.b_off % 4:
            causes.append("base")
        if len(causes) == 1:
            out.add("generic:cause:" + causes[0])
    elif p.family == "v":
        out.add(f"v:{t}:{p.tm}{p.tn}")
        out.add("v:whole-tiles" if p.whole_tiles else "v:stream-k")
        if p.sk_fix:
            if p.max_contrib <= 3:
                out.add("fix:short")                    # k_gemm_sk_fix: wb - wa <= 2, the one-at-a-time loop
            if p.max_contrib <= 2:
                out.add("fix:le2")
            if p.max_contrib > 10:
                out.add("fix:gt10")                     # the eight-at-a-time loop, more than one round of it
        if p.epilogue in ("float4", "float2"):
            out.add("ep:" + p.epilogue)
        elif p.epilogue == "scalar":
            out.add("ep:scalar:odd-ldc" if ldc % 2 else "ep:scalar:c-off1")
    else:
        out.add(f"b3:{t}")
        if p.grp_mode in (1, 2) and p.ngroups_mod8 != 0:
            out.add(f"b3:grp{p.grp_mode}:ragged")
        if p.grp_mode == 3:
            out.add("b3:grp3")                          # (ngroups = the split count, a multiple of 8 by construction)
        if p.grp_mode == 0 and p.splits == 1 and c.xcd and p.grid[0] > 64 and p.grid[1] > 64:
            out.add("b3:grp0:size")
        if p.grp_mode == 0 and p.splits > 1 and p.splits % 8 != 0 and c.xcd:
            out.add("b3:split:plain")
        if p.last_chunk % B3_BK != 0:
            out.add("b3:ktail")
    return out


def coverage(cus, cases):
    got = set()
    for c in cases:
        got |= labels(c, case_plan(cus, c))
    return got


def missing(cus, cases):
    got = coverage(cus, cases)
    return [r for r in REQUIRED if r not in got]


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def int_operands(c, seed=0):
    """Integer-valued fp32 operands in their STORAGE shapes ([K, M] if tA else [M, K]; [N, K] if tB else [K, N])."""
    rs = np.random.RandomState(seed + c.M * 7 + c.N * 3 + c.K)
    A = rs.randint(-c.amax, c.amax + 1, size=(c.K, c.M) if c.tA else (c.M, c.K)).astype(np.float32)
    B = rs.randint(-c.bmax, c.bmax + 1, size=(c.N, c.K) if c.tB else (c.K, c.N)).astype(np.float32)
    return A, B


def exact_bound(c):
    """An upper bound of (|A| @ |B|).max() that needs no product: K amax bmax."""
    return c.K * c.amax * c.bmax


def planes_needed(vmax):
    """bf16 planes an integer of magnitude <= vmax occupies in the three-way split (8 significant bits each)."""
    return 1 if vmax <= 255 else (2 if vmax <= 65535 else 3)


def op(X, t):
    return X.T if t else X


def exact_product(A, B, tA, tB, f32=False):
    """op(A) op(B) of integer operands under the 2^24 precondition: exact in float64 BLAS, and in float32 BLAS as well (every partial
    sum of every order is an integer below 2^24) -- f32 spares the float64 copies of a large case."""
    a, b = op(A, tA), op(B, tB)
    mag_max = float((np.abs(a).astype(np.float64).sum(1).max()) * np.abs(b).max())      # >= (|A| @ |B|).max(), cheap
    if mag_max >= EXACT:
        mag_max = float((np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)).max())
    assert mag_max < EXACT, mag_max
    if f32:
        return a @ b
    return (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)


def spread_operands(shape_a, shape_b, rs):
    """Entries spread over 12 decades, signs at random: sums that cancel (the data of test_gemm_three_way_split_is_fp32_grade)."""
    A = (rs.normal(size=shape_a) * 10.0 ** rs.uniform(-6, 6, size=shape_a)).astype(np.float32)
    B = (rs.normal(size=shape_b) * 10.0 ** rs.uniform(-6, 6, size=shape_b)).astype(np.float32)
    return A, B


def act64(z, act):
    if act == "tanh":
        return np.tanh(z)
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    return z
