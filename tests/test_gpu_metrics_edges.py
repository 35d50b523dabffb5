"""el_rec_metrics and its column-sum tree (csrc/el_metrics.hip, el_metrics_tree.h) at their edges, every per-user row and every sum
against tests/helpers/metrics_ref.py (plain Python, correctly rounded sums); el_topk_fragile on crafted lists against NumPy.

Tolerances (u = 2^-53, the unit roundoff of fp64; c = cutoff).  They follow from the arithmetic, none is fitted to the device:

  Precision, Recall, HR, MRR, valid   one IEEE division of two small integers (or a constant): the same bits on both sides.
  F1      2 * p * r / (p + r): four operations on bit-equal p, r, no a * b + c for the compiler to contract.  2 ulp.
  DCG, IDCG, MAP sum   sums of at most c non-negative terms.  Summing t non-negative terms in any order (lane-strided, then a
          butterfly) is within (t - 1) u, relative, of their exact sum, and the reference's fsum within u.  Each DCG / IDCG term is a
          product gain x discount, rounded once on both sides (the library is built with contraction off): + u.  The gain is
          exp2(x) - 1 with x >= 1: the device exp2 is good to a few ulp for fractional x and the subtraction at most doubles that
          relative error, since exp2(x) >= 2.
  nDCG    DCG / IDCG: (c + few) u for each sum and u for the division: rel <= (2 c + 16) u.
  MAP     the terms hits / rank are single divisions, bit-equal; c - 1 additions, the reference's rounding and the division by c:
          rel <= (c + 4) u.
  sums    m valid rows of non-negative values through the partial / final tree: (m - 1) u for the order, u for the reference:
          rel <= (m + 8) u, plus the row tolerance where the rows themselves may differ (nDCG, MAP, F1).  HR and valid are
          integers below 2^53: exact.  A non-zero start of `sums` is one more term.

Every test prints the largest error it saw as a fraction of its bound (pytest -s shows them)."""
import numpy as np
import pytest
import torch

from elliot_amd import ops
from tests.helpers import metrics_ref as mr

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
EXACT = (1, 2, 3, 5, 7)


def row_rel(cutoff):
    """the relative bound of the columns that are not bit-equal (F1: the relative size of its 2 ulp, for the sums)"""
    return {0: (2 * cutoff + 16) * U53, 4: (cutoff + 4) * U53, 6: 2 * 2.0 ** -52}


def device(ctx, recs, test, thr, cutoff, u_start=0, sums=None, per_user=True):
    rec = torch.from_numpy(np.ascontiguousarray(recs, dtype=np.int32)).to(ctx.device)
    if sums is not None:
        sums = torch.from_numpy(np.asarray(sums, np.float64).copy()).to(ctx.device)
    out = ops.rec_metrics(ctx, rec, test, thr, cutoff, u_start=u_start, sums=sums, per_user=per_user)
    torch.cuda.synchronize()
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if per_user else (out.cpu().numpy(), None)


def check_rows(got, ref, cutoff, what):
    """All eight columns, user by user; returns the worst error / bound of the toleranced columns."""
    assert got.shape == ref.shape
    for m in EXACT:
        bad = np.flatnonzero(got[:, m].view(np.uint64) != ref[:, m].view(np.uint64))
        assert bad.size == 0, (what, "column", m, "user", int(bad[0]), got[bad[0]], ref[bad[0]])
    worst = {}
    for m, rel in row_rel(cutoff).items():
        tol = 2 * np.spacing(ref[:, m]) if m == 6 else rel * ref[:, m]
        err = np.abs(got[:, m] - ref[:, m])
        bad = np.flatnonzero(~(err <= tol))
        assert bad.size == 0, (what, "column", m, "user", int(bad[0]), got[bad[0], m], ref[bad[0], m], err[bad[0]] / tol[bad[0]])
        nz = tol > 0
        worst[m] = float(np.max(err[nz] / tol[nz])) if nz.any() else 0.0
    return worst


def check_sums(got, ref_rows, cutoff, what, start=None):
    valid = ref_rows[ref_rows[:, 7] != 0]
    m = valid.shape[0]
    start = np.zeros(8) if start is None else np.asarray(start, np.float64)
    ref = mr.sums(np.vstack([valid, np.concatenate([start[:7], [1.0]])[None]]))
    ref[7] = m + start[7]
    rr = row_rel(cutoff)
    worst = {}
    for c in range(8):
        if c in (3, 7):
            assert got[c] == ref[c], (what, "sum", c, got[c], ref[c])
            continue
        tol = ((m + 8) * U53 + rr.get(c, 0.0)) * ref[c]
        err = abs(got[c] - ref[c])
        assert err <= tol, (what, "sum", c, got[c], ref[c], err / tol if tol else np.inf)
        worst[c] = err / tol if tol else 0.0
    return worst


def check(ctx, recs, ip, items, ratings, thr, cutoff, what, ref=None, u_start=0, start=None, test=None):
    test = test or ops.DeviceTestSet(ip, items, ratings, ctx.device)
    if ref is None:
        ref = mr.rows(recs, ip, items, ratings, thr, cutoff, u_start=u_start)
    sums, rows = device(ctx, recs, test, thr, cutoff, u_start=u_start, sums=start)
    wr = check_rows(rows, ref, cutoff, what)
    ws = check_sums(sums, ref, cutoff, what, start=start)
    print(f"\n{what}: rows err/bound nDCG {wr[0]:.3f} MAP {wr[4]:.3f} F1 {wr[6]:.3f}; sums err/bound max {max(ws.values()):.3f}")
    return sums, rows, ref


# ---- 1. cutoffs, hit ranks and list shapes over the 64-lane chunks ---------------------------------------------------------
LANE_RANKS = (1, 2, 63, 64, 65, 128, 129)       # + the cutoff itself


def lanes_case(cutoff, ld):
    """13 users, thr 2: 0..7 a single hit at rank LANE_RANKS / cutoff (beyond the cutoff, where the list is that long, it must not
    count), 8 every slot a hit, 9 no hit, 10 all -1, 11 hits only beyond the cutoff, 12 one relevant item recommended twice.
    The slots without a hit hold items outside the row and test items below the threshold."""
    rs = np.random.RandomState(1000 * cutoff + ld)
    U, I, thr = 13, 6000, 2.0
    deg = rs.randint(6, 40, size=U)
    deg[8] = 900
    ip = np.zeros(U + 1, np.int64)
    ip[1:] = np.cumsum(deg)
    items = np.concatenate([np.sort(rs.choice(I, size=d, replace=False)) for d in deg]).astype(np.int32)
    ratings = rs.uniform(0.5, 5.0, size=ip[-1]).astype(np.float32)
    for u in range(U):
        ratings[ip[u]:ip[u] + 4] = (4.25, 1.0, 3.5, 2.0)                  # three relevant (one exactly at thr), one not
    r8 = np.concatenate([rs.uniform(2.0, 5.0, size=600), rs.uniform(0.5, 1.99, size=300)]).astype(np.float32)
    ratings[ip[8]:ip[9]] = rs.permutation(r8)
    recs = np.empty((U, ld), np.int32)
    ranks = LANE_RANKS + (cutoff,)
    for u in range(U):
        row, rr = items[ip[u]:ip[u + 1]], ratings[ip[u]:ip[u + 1]]
        relv, nonrel = row[rr >= thr], row[rr < thr]
        fill = rs.choice(np.setdiff1d(np.arange(I), row), size=ld, replace=False).astype(np.int32)
        slots = rs.choice(ld, size=min(len(nonrel), ld // 2), replace=False)
        fill[slots] = nonrel[:len(slots)]
        recs[u] = fill
        if u < 8:
            if ranks[u] <= ld:
                recs[u, ranks[u] - 1] = relv[0]
        elif u == 8:
            recs[u] = rs.permutation(relv)[:ld]
        elif u == 10:
            recs[u] = -1
        elif u == 11:
            recs[u, ::3] = -1
            recs[u, cutoff:] = relv[:ld - cutoff]
        elif u == 12:
            recs[u, 0] = relv[1]
            recs[u, min(ld, max(cutoff, 2)) - 1] = relv[1]
    return recs, ip, items, ratings, thr


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("cutoff", [1, 63, 64, 65, 128, 511, 512])
def test_lane_grid(ctx, cutoff, extra):
    ld = cutoff + extra
    recs, ip, items, ratings, thr = lanes_case(cutoff, ld)
    _, _, ref = check(ctx, recs, ip, items, ratings, thr, cutoff, f"lanes c={cutoff} ld={ld}")
    # the case holds what it says (reference side)
    for u, r in enumerate(LANE_RANKS + (cutoff,)):
        assert ref[u, 5] == (1.0 / r if r <= cutoff else 0.0) and ref[u, 1] == (1.0 / cutoff if r <= cutoff else 0.0)
    assert ref[8, 1] == 1.0 and ref[8, 5] == 1.0
    assert not ref[9:12, :7].any() and ref[:, 7].all()
    assert ref[12, 1] == (2.0 if cutoff >= 2 else 1.0) / cutoff


def test_refused_cutoffs(ctx):
    recs, ip, items, ratings, thr = lanes_case(64, 64)
    test = ops.DeviceTestSet(ip, items, ratings, ctx.device)
    rec = torch.from_numpy(recs).to(ctx.device)
    with pytest.raises(ops._lib.ElliotHipError):
        ops.rec_metrics(ctx, rec, test, thr, 65)                             # cutoff > ld
    wide = torch.full((13, 520), -1, dtype=torch.int32, device=ctx.device)
    with pytest.raises(ops._lib.ElliotHipError):
        ops.rec_metrics(ctx, wide, test, thr, 513)                           # cutoff > 512
    torch.cuda.synchronize()


# ---- 2. the IDCG selection at the edges of its gain buffer -----------------------------------------------------------------
@pytest.fixture(scope="module")
def idcg_refs():
    out = {}
    for cutoff in (1, 64, 512):
        case = mr.idcg_case(cutoff)
        out[cutoff] = case + (mr.rows(*case[:4], case[4], cutoff),)
    return out


@pytest.mark.parametrize("cutoff", [1, 64, 512])
def test_idcg_buffer_edges(ctx, idcg_refs, cutoff):
    recs, ip, items, ratings, thr, ref = idcg_refs[cutoff]
    hitters = ref[2::2] if cutoff == 1 else ref[1:]             # cutoff 1 recommends the largest gain to every other user
    assert hitters[:, 0].all() and ref[1:, 7].all() and ref[0, 7] == 0          # their nDCG exercises the IDCG
    sums, rows, _ = check(ctx, recs, ip, items, ratings, thr, cutoff, f"idcg c={cutoff}", ref=ref)
    # 6. the same bytes from a second run
    sums2, rows2 = device(ctx, recs, ops.DeviceTestSet(ip, items, ratings, ctx.device), thr, cutoff)
    assert sums.tobytes() == sums2.tobytes() and rows.tobytes() == rows2.tobytes()


# ---- 3. the threshold --------------------------------------------------------------------------------------------------
def thr_case():
    rs = np.random.RandomState(5)
    deg = np.array([0, 1, 3, 8, 2, 5, 7])
    ip = np.zeros(len(deg) + 1, np.int64)
    ip[1:] = np.cumsum(deg)
    items = np.concatenate([np.sort(rs.choice(50, size=d, replace=False)) for d in deg]).astype(np.int32)
    recs = np.stack([rs.choice(50, size=5, replace=False) for _ in deg]).astype(np.int32)
    for u, d in enumerate(deg):
        if d:
            recs[u, u % 5] = items[ip[u]]
            recs[u, (u + 2) % 5] = items[ip[u + 1] - 1]
    return recs, ip, items


THR = 2.5
BELOW = np.nextafter(np.float32(THR), np.float32(-np.inf))
START = np.array([0.125, 3.5, 7.0, 2.0, 1e-3, 0.3, 11.0, 5.0])


@pytest.mark.parametrize("kind", ["at", "below", "at_below", "plus30_at", "implicit"])
def test_threshold_edge(ctx, kind):
    recs, ip, items = thr_case()
    nnz = int(ip[-1])
    alt = np.arange(nnz) % 2 == 0
    ratings = {"at": np.full(nnz, THR), "below": np.full(nnz, BELOW), "at_below": np.where(alt, THR, BELOW),
               "plus30_at": np.where(alt, THR + 30, THR), "implicit": None}[kind]
    thr = 1.0 if kind == "implicit" else THR
    if ratings is not None:
        ratings = ratings.astype(np.float32)
    sums, rows, ref = check(ctx, recs, ip, items, ratings, thr, 5, f"threshold {kind}", start=START)
    if kind == "below":
        assert not rows.any() and sums.tobytes() == START.tobytes()
    else:
        assert ref[1:, 7].all() and ref[:, 3].sum() >= 3 and ref[0, 7] == 0
    if kind == "plus30_at":
        assert 2.0 ** 31 - 1 == 2.0 ** (np.float32(THR + 30) - THR + 1) - 1


@pytest.mark.parametrize("kind", ["implicit_thr_above_1", "no_entries", "no_entries_with_ratings"])
def test_nobody_valid_leaves_sums_untouched(ctx, kind):
    recs, ip, items = thr_case()
    ratings = None
    if kind != "implicit_thr_above_1":
        ip, items = np.zeros_like(ip), np.zeros(0, np.int32)
        ratings = np.zeros(0, np.float32) if kind.endswith("ratings") else None
    for per_user in (True, False):
        sums, rows = device(ctx, recs, ops.DeviceTestSet(ip, items, ratings, ctx.device), 1.5, 5, sums=START, per_user=per_user)
        assert sums.tobytes() == START.tobytes()
        assert rows is None or not rows.any()
    assert not mr.rows(recs, ip, items, ratings, 1.5, 5).any()


# ---- 4. user counts around the workgroup and the tree groups, user offsets ------------------------------------------------
TAIL_N = (1, 2, 3, 5, 4095, 4096, 4097, 8193, 12289)
OFF = 129


@pytest.fixture(scope="module")
def tail():
    """12289 users, degrees 0..12, fractional ratings, thr 2.5, cutoff 10; the last user of every block the tests cut is valid, so
    a block that loses its last user loses a count."""
    rs = np.random.RandomState(4)
    N, I, k, thr = max(TAIL_N), 500, 10, 2.5
    deg = rs.randint(0, 13, size=N)
    ends = [n - 1 for n in TAIL_N] + [OFF - 1, OFF, OFF + 4097 - 1, 4097 + 3 - 1, 4097 + 3]
    deg[ends] = np.maximum(deg[ends], 1)
    ip = np.zeros(N + 1, np.int64)
    ip[1:] = np.cumsum(deg)
    items = np.concatenate([np.sort(rs.choice(I, size=d, replace=False)) for d in deg]).astype(np.int32)
    ratings = rs.uniform(0.5, 5.0, size=ip[-1]).astype(np.float32)
    ratings[ip[ends]] = 5.0
    recs = rs.randint(0, I, size=(N, k)).astype(np.int32)
    for u in range(0, N, 2):
        if deg[u]:
            recs[u, rs.randint(k)] = items[ip[u] + rs.randint(deg[u])]
    recs[rs.rand(N, k) < 0.05] = -1
    ref = mr.rows(recs, ip, items, ratings, thr, k)
    assert ref[ends, 7].all() and 0.5 * N < ref[:, 7].sum() < N and 0.2 * N < ref[:, 3].sum()
    return dict(recs=recs, ip=ip, items=items, ratings=ratings, thr=thr, k=k, ref=ref)


@pytest.fixture(scope="module")
def tail_test(ctx, tail):
    return ops.DeviceTestSet(tail["ip"], tail["items"], tail["ratings"], ctx.device)


def check_block(ctx, tail, tail_test, lo, n, what, start=None):
    return check(ctx, tail["recs"][lo:lo + n], tail["ip"], tail["items"], tail["ratings"], tail["thr"], tail["k"], what,
                 ref=tail["ref"][lo:lo + n], u_start=lo, start=start, test=tail_test)


@pytest.mark.parametrize("n", TAIL_N)
def test_user_count_tail(ctx, tail, tail_test, n):
    check_block(ctx, tail, tail_test, 0, n, f"tail n={n}")


def test_user_block_at_an_offset(ctx, tail, tail_test):
    check_block(ctx, tail, tail_test, OFF, 4097, f"tail n=4097 u_start={OFF}", start=START)


def test_blocks_accumulate_into_one_sums(ctx, tail, tail_test):
    n = 4097 + 3 + 1
    single, _, _ = check_block(ctx, tail, tail_test, 0, n, f"tail n={n}", start=START)
    acc, lo = START, 0
    for b in (4097, 3, 1):                                      # u_start 0, 4097, 4100
        acc, _ = device(ctx, tail["recs"][lo:lo + b], tail_test, tail["thr"], tail["k"], u_start=lo, sums=acc, per_user=False)
        lo += b
    ws = check_sums(acc, tail["ref"][:n], tail["k"], "blocks 4097 + 3 + 1", start=START)
    print(f"\nblocks 4097 + 3 + 1: sums err/bound max {max(ws.values()):.3f}")
    assert acc[3] == single[3] and acc[7] == single[7]


def test_small_call_after_a_large_one(ctx, tail, tail_test):
    """the workspace keeps the rows of the 12289-user call: a 3-user call must not read past its own"""
    big, _ = device(ctx, tail["recs"], tail_test, tail["thr"], tail["k"], per_user=False)
    check_sums(big, tail["ref"], tail["k"], "n=12289 without per-user rows")
    small, _ = device(ctx, tail["recs"][:3], tail_test, tail["thr"], tail["k"], per_user=False)
    check_sums(small, tail["ref"][:3], tail["k"], "n=3 after n=12289")


# ---- el_topk_fragile on crafted lists ------------------------------------------------------------------------------------
def fragile_device(ctx, c, rows=slice(None), **kw):
    d = ctx.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    lo = c["u_start"] + (rows.start or 0)
    out = ops.topk_fragile(ctx, t(c["Gu"]), t(c["Gi"]), t(c["idx"][rows]), t(c["val"][rows]), c["k"], u_start=lo,
                           item_offset=c["item_offset"], **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("F", mr.FRAGILE_F)
@pytest.mark.parametrize("n", mr.FRAGILE_N)
def test_fragile_crafted_lists(ctx, F, n):
    """u_start = 37 into a larger Gu, item_offset = 1000 with Gi holding rows 1000 onward; from 5 users on, rows 0..2 are the three
    kinds of short list (flag 0, one count each in counts[1]) and row 3 an exact tie (fragile)."""
    c = mr.fragile_case(F, n, mr.fragile_seed(F, n))
    assert c["margin"] > mr.FRAGILE_MARGIN                      # no user's flag hangs on the summation order
    counts, flags = fragile_device(ctx, c, flags=True)
    got = flags.cpu().numpy().astype(bool)
    assert np.array_equal(got, c["flags"]), np.flatnonzero(got != c["flags"])
    assert tuple(counts.cpu().tolist()) == c["counts"]
    if n >= 5:
        assert got[3] and not got[:3].any() and c["counts"][1] == 3
    # a second call adds to the same counts; without flags
    again = fragile_device(ctx, c, counts=counts)
    assert again is counts and tuple(counts.cpu().tolist()) == (2 * c["counts"][0], 2 * c["counts"][1])


@pytest.mark.parametrize("F", [1, 65])
def test_fragile_single_user_kinds(ctx, F):
    """n = 1 for each kind of row: the three short lists, the tie, a plain row; one counts tensor through all five calls."""
    c = mr.fragile_case(F, 5, mr.fragile_seed(F, 5))
    assert c["margin"] > mr.FRAGILE_MARGIN
    counts = torch.zeros(2, dtype=torch.int64, device=ctx.device)
    exp = [0, 0]
    for r in range(5):
        _, fl = fragile_device(ctx, c, rows=slice(r, r + 1), flags=True, counts=counts)
        assert bool(fl.cpu().numpy()[0]) == bool(c["flags"][r]), r
        exp[0] += int(c["flags"][r])
        exp[1] += int(r < 3)
        assert counts.cpu().tolist() == exp, r


def test_fragile_no_offsets_matches_offsets(ctx):
    """the same lists with u_start = 0 and item_offset = 0 (Gu, Gi cut to the block; ids shifted) give the same flags"""
    c = mr.fragile_case(63, 701, mr.fragile_seed(63, 701))
    z = dict(c, Gu=c["Gu"][c["u_start"]:], idx=np.where(c["idx"] >= 0, c["idx"] - c["item_offset"], -1).astype(np.int32), u_start=0,
             item_offset=0)
    counts, flags = fragile_device(ctx, z, flags=True)
    assert np.array_equal(flags.cpu().numpy().astype(bool), c["flags"]) and tuple(counts.cpu().tolist()) == c["counts"]


# ---- 5. the capped tree: more than 4096 * 1024 users (keep this test last: it grows the metric workspace to 0.27 GB) --------
def test_capped_tree_exact_counts(ctx):
    n = 4096 * 1024 + 5
    u = np.arange(n, dtype=np.int64)
    hit = u % 3 == 0
    items = (u % 1000).astype(np.int32)
    recs = np.where(hit, items, -1).astype(np.int32)[:, None]
    test = ops.DeviceTestSet(np.arange(n + 1, dtype=np.int64), items, None, ctx.device)
    try:
        sums, _ = device(ctx, recs, test, 1.0, 1, per_user=False)
    finally:
        ctx._metrics_ws = None                                   # hand the 0.27 GB back
    exp = np.full(8, float(np.count_nonzero(hit)))
    exp[7] = float(n)
    assert np.array_equal(sums, exp), (sums, exp)
