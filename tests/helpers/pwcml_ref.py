"""What tests/test_gpu_pointwise_edges.py and tests/test_gpu_cml_edges.py hold the point-wise factor models (elliot_amd/csrc/el_pwmf.hip)
and Collaborative Metric Learning (el_cml.hip, the cml branches of el_bpr_sorted.hip, el_segcombine.h) to, in NumPy fp64:
  pick_lpt / lanes      el_pick_lpt restated: lanes per row and chunks per lane of a factor count
  Plan / make_batch / assert_layout
                        batches whose sorted segments sit at prescribed positions against the chunk borders of the segment pass
  pw_ref                loss and gradient sums of MF / FunkSVD / PMF / LogisticMF with the batch mean over n_global samples, for one side or both
  cml_*                 D, E, regulariser, brute-force counts and hinge share, row gradients
  pw_budget / cml_budget
                        the EXACT cases: every input sits on a dyadic grid, so every product and every partial sum of the kernels is a
                        multiple of one quantum q; while sum |terms| < 2^24 q, every fp32 partial sum is representable whatever the order
                        of summation (sorted segments, pieces, float atomics, wave shuffles) and the device must give the fp64 bits
  pw_bound / pw_emulate_f32
                        the BOUNDED cases (sigmoid / softplus links), see pw_bound
  the case tables       shared with tests/test_pwcml_ref_host.py, which checks budgets, bounds and layouts without a GPU

Error bound of the bounded cases (pw_bound), forward error analysis against fp64, first order, u = 2^-24 per fp32 operation and
(len + 1) u sum|terms| for a sum of len terms:
  x = <gu, gi> + Bu + Bi        |dx| <= (F + 3) u (sum_f |gu_f gi_f| + |Bu| + |Bi|)
  e = expf(-x)                  relative error |dx| + 2 ULP u          (ULP units in the last place = 2 ULP u relative)
  o = 1 / (1 + e)               do/de = -o^2, one add, one divide:     |do| <= o (1 - o) (|dx| + 2 ULP u) + 2 u o
  PMF    r = o - y              |dr| <= |do| + u |r|;   1 - o: |do| + u (1 - o)
         c = 2 r inv_n o (1-o)  |dc| <= 2 inv_n (|dr| o (1-o) + |r| |do| (1-o) + |r| o (|do| + u (1-o))) + 4 u |c|     (three products, inv_n)
         loss term r^2 inv_n    <= 2 |r| |dr| inv_n + 3 u r^2 inv_n
  LogisticMF  w = 1 + alpha y (exact for the alpha used),  c = w o - alpha y:   |dc| <= w |do| + u w o + u |c|
         softplus(x) = log1pf(expf(x)) (x <= 15; x + expf(-x) above):  |dsp| <= o (|dx| + 2 ULP u) + 2 ULP u sp + u (sp + |x|)
         loss term w sp - alpha y x + l_w sq / 2:   w |dsp| + alpha y |dx| + (2 F + 3) u l_w sq / 2 + 4 u (w sp + alpha y |x| + l_w sq / 2)
  g[row, f] = sum_b c_b v_bf (+ cnt l_w own_f, added once per piece of a cut row): T = len + pieces terms, two roundings for the L2 term
         |dg| <= sum_b |dc_b| |v_bf| + (T + 3) u (sum_b |c_b v_bf| + cnt l_w |own_f|)
  bias   |dgb| <= sum_b |dc_b| + (len + pieces + 1) u sum_b |c_b|
ULP: no copy of ROCm's accuracy tables is at hand, so expf and log1pf are ASSUMED to be within 2 units in the last place (LIBM_ULP); for that
assumption the whole bound carries the factor LIBM_SLACK = 2 and nothing else.  Nothing here was fitted to a device result:
tests/test_pwcml_ref_host.py holds an fp32 NumPy emulation in two summation orders to the bound and shows that a dropped, doubled or
misplaced sample of any covered row (<= COVERED_LEN samples) breaks it.
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import cml as oc
from oracle import pointwise_mf as pw

f32, f64 = np.float32, np.float64
U_RND = 2.0 ** -24               # unit round-off of fp32
BUDGET = 1 << 24                 # quanta an fp32 partial sum can hold exactly
USER_CHUNK, ITEM_CHUNK = 4, 16   # el_pwmf.hip user_chunk(n) for n < 5 * 65536, item_chunk(n) for n < 17 * 16384 (sorted positions per lane group)
CML_ITEM_CHUNK = 16              # el_bpr_sorted.hip item_chunk_for(B, I) for 2 B < 17 * 8192, over the 2 B positions of (i, j)
CML_SORTED_FROM = 2048           # el_cml.hip cml_grads: the sorted-segment path from this many triplets, float atomics below
LIBM_ULP = 2.0                   # ASSUMED accuracy of the device's expf / log1pf (see above)
LIBM_SLACK = 2.0
COVERED_LEN = 64                 # rows of at most this many samples are under the no-hiding guarantee
QT = 0.25                        # grid of the tables, biases and labels of the exact cases


# ---- el_pick_lpt (el_bpr.hip) ----------------------------------------------------------------------------------------------------------
def pick_lpt(F, vw):
    """-> (lanes per row, chunks per lane), or (None, None) where the library refuses the size (more than 4 chunks per lane)."""
    groups = (F + vw - 1) // vw
    lpt = 8
    while lpt < groups and lpt < 64:
        lpt *= 2
    cpl = 1
    while cpl < (groups + lpt - 1) // lpt:
        cpl *= 2
    return (lpt, cpl) if cpl <= 4 else (None, None)


def lanes(F):
    """(VW, lpt, CPL) of F-wide fp32 rows on 16-byte aligned tables."""
    vw = 4 if F % 4 == 0 else 1
    return (vw,) + pick_lpt(F, vw)


# ---- batches with prescribed segment positions -------------------------------------------------------------------------------------------
def conts_of(start, end, chunk):
    """Lane groups after the one that holds `start` whose chunk still begins inside [start, end): the chunk borders in (start, end)."""
    return (np.asarray(end) - 1) // chunk - np.asarray(start) // chunk


class Plan:
    """Sample counts of one side's rows in ascending row id = the sorted segments in order.  `conts` given to row() is asserted as the plan is
    built; names[...] remembers the rows a docstring speaks of."""

    def __init__(self, chunk):
        self.c, self.counts, self.pos, self.names = int(chunk), [], 0, {}

    def row(self, length, conts=None, name=None):
        assert length >= 1
        k = int(conts_of(self.pos, self.pos + length, self.c))
        assert conts is None or k == conts, (name, self.pos, length, k, conts)
        self.counts.append(int(length))
        self.pos += int(length)
        if name:
            self.names[name] = len(self.counts) - 1
        return len(self.counts) - 1

    def row_conts(self, k, tail=1, name=None):
        """A row from here that continues into k following chunks and ends `tail` positions into the last of them."""
        assert 1 <= tail <= self.c and k >= 1
        return self.row((self.pos // self.c + k) * self.c + tail - self.pos, conts=k, name=name)

    def fill_to(self, rem):
        """Plain one-sample rows up to the next position = rem (mod chunk)."""
        while self.pos % self.c != rem % self.c:
            self.row(1, conts=0)

    def fill_until(self, pos):
        """Plain rows up to `pos`: alternately one that ends on the next chunk border and a single sample."""
        assert pos >= self.pos
        t = 0
        while self.pos < pos:
            room = min(self.c - self.pos % self.c, pos - self.pos)
            self.row(room if t % 2 == 0 else 1, conts=0)
            t += 1

    def finish(self, n):
        """... and a last row that starts on the last position of a chunk and ends with the data, n no multiple of the chunk."""
        assert n % self.c != 0
        s = (n // self.c) * self.c - 1
        if s < self.pos:                     # n < chunk (one lane group) or nothing left to cut: plain rows to the end
            if self.pos < n:
                self.fill_until(n)
            return self
        self.fill_until(s)
        self.row(n - s, conts=1, name="last_cut")
        return self

    def expect(self):
        cnt = np.asarray(self.counts, np.int64)
        end = np.cumsum(cnt)
        start = end - cnt
        return start, end, conts_of(start, end, self.c)


def layout_of(ids, chunk):
    """From the batch itself: the rows present, the [start, end) of each one's sorted segment and its number of continuations."""
    s = np.sort(np.asarray(ids, np.int64), kind="stable")
    rows, start = np.unique(s, return_index=True)
    end = np.r_[start[1:], len(s)]
    return rows, start, end, conts_of(start, end, chunk)


def assert_layout(ids, plan):
    rows, start, end, conts = layout_of(ids, plan.c)
    estart, eend, econts = plan.expect()
    assert np.array_equal(rows, np.arange(len(plan.counts))), "rows of the plan missing from the batch"
    assert np.array_equal(start, estart) and np.array_equal(end, eend) and np.array_equal(conts, econts), "segments are not where the plan put them"
    return conts


def make_batch(rs, plan_u, plan_i):
    """u, i in a shuffled batch order with plan_u's counts per user and plan_i's per item (the pairing is random)."""
    n = plan_u.pos
    assert plan_i.pos == n, (n, plan_i.pos)
    u = np.repeat(np.arange(len(plan_u.counts)), plan_u.counts)
    i = np.repeat(np.arange(len(plan_i.counts)), plan_i.counts)
    rs.shuffle(i)
    perm = rs.permutation(n)
    return u[perm].astype(np.int64), i[perm].astype(np.int64)


def _small_body(p, L):
    """The short layouts of el_segcombine.h's decisions, c = chunk, L = lanes per row."""
    c = p.c
    p.row(c + 1, conts=1, name="first_cut")                       # the first row of the sort (pos == 0) is cut
    p.fill_to(c - 2)
    p.row(2, conts=0, name="ends_on_border")                      # ends exactly on a chunk border ...
    p.row(2, conts=0, name="starts_on_border")                    # ... the next starts on it: both plain stores
    p.fill_to(c - 1)
    p.row(2, conts=1, name="two_positions")                       # head piece of 1, tail piece of 1
    p.fill_to(0)
    p.row(3 * c, conts=2, name="three_chunks")                    # head, middle piece, last piece that ends on a border
    p.fill_to(c - 2)
    p.row(3, conts=1, name="adjacent_a")                          # its tail and the next row's head share a chunk: slots 2 g and 2 g + 1
    p.row(c, conts=1, name="adjacent_b")
    for t, k in enumerate((L - 2, L - 1, L, L + 1)):              # k_seg_combine's last sizes, the long list's first
        p.fill_to(t % 2)
        p.row_conts(k, tail=1 + t % 3, name="conts_%d" % k)
    p.row_conts(L + 3, tail=c, name="long_b")                     # with conts_L, conts_L+1: more than three long-list rows in one batch
    p.row_conts(2 * L, tail=2, name="long_c")


def _round_n(n, slack=40):
    n += slack
    return n + (5 - n % 16) % 16                                  # n = 5 (mod 16): no multiple of either chunk


LAYOUTS = ("small", "long_a", "long_b", "long_c", "long_d", "tiny", "one")


@functools.lru_cache(maxsize=None)
def layout_plans(name, L=8):
    """-> (plan of the user side, plan of the item side) with equal n.
      small    every short layout on both sides
      long_a   users: 255, 256, 257, 513 continuations (first, second, third pass of the long kernel's 256-wide search); items: 255
      long_b   items: 256          long_c   items: 257          long_d   items: 513 (one item of about 8200 samples); users: 513, 257
      tiny     n = 3 < chunk (one lane group)                   one      n = 1"""
    pu, pi = Plan(USER_CHUNK), Plan(ITEM_CHUNK)
    if name == "tiny":
        pu.row(2), pu.row(1), pi.row(1), pi.row(2)
        return pu, pi
    if name == "one":
        pu.row(1), pi.row(1)
        return pu, pi
    if name == "small":
        _small_body(pu, L), _small_body(pi, L)
    else:
        ku, ki = {"long_a": ((255, 256, 257, 513), 255), "long_b": ((L, 3), 256), "long_c": ((1, 2 * L), 257), "long_d": ((513, 257), 513)}[name]
        pu.row(2)
        for t, k in enumerate(ku):
            pu.fill_to(t)
            pu.row_conts(k, tail=1 + t % 4, name="conts_%d" % k)
        pi.row(3)
        pi.fill_to(5)
        pi.row_conts(ki, tail=7, name="conts_%d" % ki)
    n = _round_n(max(pu.pos, pi.pos))
    return pu.finish(n), pi.finish(n)


@functools.lru_cache(maxsize=None)
def class_plans(F):
    """One compact batch per lane class: plain rows, a short cut row and a long-list row (lpt continuations) on each side."""
    L = lanes(F)[1]
    pu, pi = Plan(USER_CHUNK), Plan(ITEM_CHUNK)
    for p in (pu, pi):
        p.row(3, conts=0)
        p.fill_to(p.c - 1)
        p.row(2, conts=1, name="short_cut")
        p.row(2, conts=0)
        p.row_conts(L, tail=1, name="long")
        p.row_conts(2, tail=3, name="three_pieces")
    n = _round_n(max(pu.pos, pi.pos), slack=24)
    return pu.finish(n), pi.finish(n)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def dyadic(rs, shape):
    """Multiples of 1/4 in [-1, 1]; the first element of every row is not zero, so that no row is all zero."""
    a = rs.randint(-4, 5, size=shape)
    nz = rs.choice(np.array([-4, -3, -2, -1, 1, 2, 3, 4]), size=a.shape[0])
    if a.ndim == 2:
        a[:, 0] = nz
    else:
        a[:] = np.where(a == 0, nz, a)
    return a * QT


def pw_exact_inputs(seed, plan_u, plan_i, F, bias):
    """Dyadic tables and a batch of the plans; labels in {0, 1}, re-drawn (flipped) where the sample's coefficient would be exactly 0."""
    rs = np.random.RandomState(seed)
    U, I = len(plan_u.counts), len(plan_i.counts)
    w = {"Gu": dyadic(rs, (U, F)), "Gi": dyadic(rs, (I, F))}
    if bias:
        w["Bu"], w["Bi"] = dyadic(rs, (U,)), dyadic(rs, (I,))
    u, i = make_batch(rs, plan_u, plan_i)
    y = rs.randint(0, 2, len(u)).astype(f64)
    x = pw.raw_score(w, u, i, f64)
    y = np.where(x == y, 1.0 - y, y)
    n_global = 2 << int(np.ceil(np.log2(max(len(u), 2))))          # a power of two above n: inv_n exact, the mean runs over more than the batch
    return w, u, i, y, n_global


def pw_bounded_inputs(seed, plan_u, plan_i, F, bias):
    """Scores of moderate size (|x| about 1) for the kinds with a sigmoid / softplus link."""
    rs = np.random.RandomState(seed)
    U, I = len(plan_u.counts), len(plan_i.counts)
    s = 0.9 * F ** -0.25
    w = {"Gu": rs.normal(scale=s, size=(U, F)).astype(f32).astype(f64), "Gi": rs.normal(scale=s, size=(I, F)).astype(f32).astype(f64)}
    if bias:
        w["Bu"], w["Bi"] = (rs.normal(scale=0.2, size=k).astype(f32).astype(f64) for k in (U, I))
    u, i = make_batch(rs, plan_u, plan_i)
    y = rs.randint(0, 2, len(u)).astype(f64)
    return w, u, i, y, len(u) + 37


# ---- point-wise reference ----------------------------------------------------------------------------------------------------------------
def pw_coef(w, kind, u, i, y, n_global, alpha=0.0):
    """x, per-sample loss terms (l2 term apart) and c_b = dloss/dx in fp64, from oracle/pointwise_mf.py's raw_score, sigmoid and softplus."""
    y = np.asarray(y, f64)
    x = pw.raw_score(w, u, i, f64)
    if kind == "logistic":
        wgt = 1 + alpha * y
        return x, wgt * pw.softplus(x) - alpha * y * x, wgt * pw.sigmoid(x) - alpha * y
    o = pw.sigmoid(x) if kind == "mse_sigmoid" else x
    c = 2 * (o - y) / n_global
    if kind == "mse_sigmoid":
        c = c * o * (1 - o)
    return x, (o - y) ** 2 / n_global, c


def pw_ref(w, kind, u, i, y, n_global=None, side="both", alpha=0.0, l_w=0.0, skip=None, twice=None, move=None):
    """-> (loss, {name: dense fp64 gradient}) of oracle.pointwise_mf.loss_and_grads(dtype=float64), with the batch mean of the mean-squared
    kinds over n_global >= n samples and only the accumulators of `side` filled (the others stay zero, as on the device).
    Mutations for the no-hiding check: sample `skip` left out of the sums, sample `twice` counted twice, move = (b, row): user-side sample
    b credited to another user row."""
    w = {k: np.asarray(v, f64) for k, v in w.items()}
    n = len(y)
    n_global = n if n_global is None else n_global
    x, terms, c = pw_coef(w, kind, u, i, y, n_global, alpha)
    Gu, Gi = w["Gu"], w["Gi"]
    l2 = 0.5 * l_w * (np.sum(Gu[u] ** 2, -1) + np.sum(Gi[i] ** 2, -1)) if kind == "logistic" and l_w else np.zeros(n)
    m = np.ones(n)
    if skip is not None:
        m[skip] = 0
    if twice is not None:
        m[twice] = 2
    uu = np.array(u)
    if move is not None:
        uu[move[0]] = move[1]
    loss = float(np.sum(terms + l2))
    cm = c * m
    lw = m * (l_w if kind == "logistic" else 0.0)
    g = {k: np.zeros_like(v) for k, v in w.items()}
    if side != "items":
        np.add.at(g["Gu"], uu, cm[:, None] * Gi[i] + lw[:, None] * Gu[u])
        if "Bu" in w:
            np.add.at(g["Bu"], uu, cm)
    if side != "users":
        np.add.at(g["Gi"], i, cm[:, None] * Gu[u] + lw[:, None] * Gi[i])
        if "Bi" in w:
            np.add.at(g["Bi"], i, cm)
    return loss, g


def _on_grid(a, q, what):
    v = np.asarray(a, f64) / q
    assert np.array_equal(v, np.round(v)), what + " is off the grid"


def pw_budget(w, u, i, y, n_global):
    """The exactness budget of a mean-squared case with dyadic inputs; -> the largest sum |terms| met, in quanta (< 2^24).
    Also: no coefficient is 0 and no gathered row is all zero (a dropped sample would be invisible)."""
    for k, v in w.items():
        _on_grid(v, QT, k)
    _on_grid(y, 1.0, "labels")
    assert n_global >= len(y) and n_global & (n_global - 1) == 0, "inv_n must be exact"
    Gu, Gi = w["Gu"], w["Gi"]
    qd = QT * QT                                                   # products of two table entries, and the score
    sx = np.sum(np.abs(Gu[u] * Gi[i]), -1) + np.abs(y)
    if "Bu" in w:
        sx = sx + np.abs(w["Bu"][u]) + np.abs(w["Bi"][i])
    r = pw.raw_score(w, u, i, f64) - y
    c = 2 * r / n_global
    qc = 2 * qd / n_global
    assert (c != 0).all(), "a coefficient is exactly 0"
    assert Gu[u].any(1).all() and Gi[i].any(1).all(), "a gathered row is all zero"
    worst = [sx.max() / qd, (r * r).max() / (qd * qd)]
    for tab, own, oth in (("Gu", u, Gi[i]), ("Gi", i, Gu[u])):
        s = np.zeros_like(w[tab])
        np.add.at(s, own, np.abs(c)[:, None] * np.abs(oth))
        worst.append(s.max() / (qc * QT))
        worst.append(np.bincount(own, np.abs(c)).max() / qc)
    assert max(worst) < BUDGET, worst
    return max(worst)


def pw_emulate_f32(w, kind, u, i, y, n_global, side="both", alpha=0.0, l_w=0.0, reverse=False):
    """The step in fp32 NumPy, one rounding per operation, samples and factors taken in batch order or reversed."""
    W = {k: np.asarray(v, f32) for k, v in w.items()}
    u, i, y = (np.asarray(a)[::-1] if reverse else np.asarray(a) for a in (u, i, y))
    y = y.astype(f32)
    Gu, Gi = W["Gu"], W["Gi"]
    F = Gu.shape[1]
    a, b = Gu[u], Gi[i]
    x, sq = np.zeros(len(y), f32), np.zeros(len(y), f32)
    for f in (range(F - 1, -1, -1) if reverse else range(F)):
        x = x + a[:, f] * b[:, f]
        sq = sq + (a[:, f] * a[:, f] + b[:, f] * b[:, f])
    if "Bu" in W:
        x = x + (W["Bu"][u] + W["Bi"][i])
    sig = lambda t: f32(1) / (f32(1) + np.exp(-t))
    al, lw = f32(alpha), f32(l_w if kind == "logistic" else 0.0)
    if kind == "logistic":
        wgt = f32(1) + al * y
        sp = np.where(x > 15, x + np.exp(-x), np.log1p(np.exp(np.minimum(x, f32(15))))).astype(f32)
        term = wgt * sp - al * y * x + f32(0.5) * lw * sq
        c = wgt * sig(x) - al * y
    else:
        inv_n = f32(1) / f32(n_global)
        o = sig(x) if kind == "mse_sigmoid" else x
        r = o - y
        term = r * r * inv_n
        c = f32(2) * r * inv_n
        if kind == "mse_sigmoid":
            c = c * o * (f32(1) - o)
    assert term.dtype == f32 and c.dtype == f32
    g = {k: np.zeros_like(v) for k, v in W.items()}
    if side != "items":
        np.add.at(g["Gu"], u, c[:, None] * b + lw * a)
        if "Bu" in W:
            np.add.at(g["Bu"], u, c)
    if side != "users":
        np.add.at(g["Gi"], i, c[:, None] * a + lw * b)
        if "Bi" in W:
            np.add.at(g["Bi"], i, c)
    assert all(v.dtype == f32 for v in g.values())
    return float(np.sum(term.astype(f64))), g


def pw_bound(w, kind, u, i, y, n_global, side="both", alpha=0.0, l_w=0.0):
    """-> (bound on |loss - ref|, {name: element-wise bound on |gradient - ref|}); the derivation is in the module's docstring."""
    assert kind in ("mse_sigmoid", "logistic")
    w = {k: np.asarray(v, f64) for k, v in w.items()}
    y = np.asarray(y, f64)
    Gu, Gi = w["Gu"], w["Gi"]
    F, un, lib = Gu.shape[1], U_RND, 2 * LIBM_ULP * U_RND
    x = pw.raw_score(w, u, i, f64)
    sx = np.sum(np.abs(Gu[u] * Gi[i]), -1)
    if "Bu" in w:
        sx = sx + np.abs(w["Bu"][u]) + np.abs(w["Bi"][i])
    dx = (F + 3) * un * sx
    o = pw.sigmoid(x)
    do = o * (1 - o) * (dx + lib) + 2 * un * o
    if kind == "mse_sigmoid":
        inv_n = 1.0 / n_global
        r = o - y
        dr = do + un * np.abs(r)
        c = 2 * r * inv_n * o * (1 - o)
        dc = 2 * inv_n * (dr * o * (1 - o) + np.abs(r) * do * (1 - o) + np.abs(r) * o * (do + un * (1 - o))) + 4 * un * np.abs(c)
        dterm = 2 * np.abs(r) * dr * inv_n + 3 * un * r * r * inv_n
        lw = 0.0
    else:
        wgt = 1 + alpha * y
        c = wgt * o - alpha * y
        dc = wgt * do + un * wgt * o + un * np.abs(c)
        sp = pw.softplus(x)
        dsp = o * (dx + lib) + lib * sp + un * (sp + np.abs(x))
        sq = np.sum(Gu[u] ** 2, -1) + np.sum(Gi[i] ** 2, -1)
        dterm = wgt * dsp + alpha * y * dx + (2 * F + 3) * un * 0.5 * l_w * sq + 4 * un * (wgt * sp + alpha * y * np.abs(x) + 0.5 * l_w * sq)
        lw = l_w
    bound = {k: np.zeros_like(v) for k, v in w.items()}
    for tab, bias, own, oth, chunk, on in (("Gu", "Bu", u, Gi[i], USER_CHUNK, side != "items"), ("Gi", "Bi", i, Gu[u], ITEM_CHUNK, side != "users")):
        if not on:
            continue
        rows, _, _, conts = layout_of(own, chunk)
        cnt = np.bincount(own, minlength=len(w[tab])).astype(f64)
        terms = np.zeros(len(w[tab]))
        terms[rows] = cnt[rows] + conts + 1                        # len + pieces
        s_abs, s_err = np.zeros_like(w[tab]), np.zeros_like(w[tab])
        np.add.at(s_abs, own, np.abs(c)[:, None] * np.abs(oth))
        np.add.at(s_err, own, dc[:, None] * np.abs(oth))
        s_abs += (cnt * lw)[:, None] * np.abs(w[tab])
        bound[tab] = LIBM_SLACK * (s_err + (terms[:, None] + 3) * un * s_abs)
        if bias in w:
            bound[bias] = LIBM_SLACK * (np.bincount(own, dc, minlength=len(cnt)) + (terms + 1) * un * np.bincount(own, np.abs(c), minlength=len(cnt)))
    return LIBM_SLACK * float(np.sum(dterm)), bound


def pw_forward_bound(w, kind, u, i):
    """Bound on |forward - ref|: |dx|, through the sigmoid for PMF (the module's docstring)."""
    w = {k: np.asarray(v, f64) for k, v in w.items()}
    sx = np.sum(np.abs(w["Gu"][u] * w["Gi"][i]), -1)
    if "Bu" in w:
        sx = sx + np.abs(w["Bu"][u]) + np.abs(w["Bi"][i])
    dx = (w["Gu"].shape[1] + 3) * U_RND * sx
    if kind != "mse_sigmoid":
        return LIBM_SLACK * dx
    o = pw.sigmoid(pw.raw_score(w, u, i, f64))
    return LIBM_SLACK * (o * (1 - o) * (dx + 2 * LIBM_ULP * U_RND) + 2 * U_RND * o)


def bound_ratio(got, ref, bound):
    """Largest |got - ref| / bound; an element with bound 0 (a row the batch does not touch) must be equal."""
    d = np.abs(np.asarray(got, f64) - ref)
    assert not d[bound == 0].any(), "a row outside the batch was written"
    return float((d[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def pw_hidden_rows(w, kind, u, i, y, n_global, side, alpha, l_w, bound):
    """Covered rows (<= COVERED_LEN samples) in which SOME sample could be dropped, doubled or credited elsewhere without any element leaving
    twice the bound -- {table: row ids}; the bounded cases need this empty.  Removing, doubling or moving sample b changes its row by
    -/+ (c_b v_b + l_w own, c_b), and a kernel that did so would sit within one bound of the changed reference."""
    w = {k: np.asarray(v, f64) for k, v in w.items()}
    _, _, c = pw_coef(w, kind, u, i, y, n_global, alpha)
    lw = l_w if kind == "logistic" else 0.0
    out = {}
    for tab, bias, own, oth, on in (("Gu", "Bu", u, w["Gi"][i], side != "items"), ("Gi", "Bi", i, w["Gu"][u], side != "users")):
        if not on:
            continue
        delta = np.abs(c[:, None] * oth + lw * w[tab][own])
        seen = (delta > 2 * bound[tab][own]).any(1)
        if bias in w:
            seen |= np.abs(c) > 2 * bound[bias][own]
        cnt = np.bincount(own, minlength=len(w[tab]))
        hidden = np.unique(np.asarray(own)[~seen & (cnt[own] <= COVERED_LEN)])
        out[tab] = hidden.tolist()
    return out


# ---- CML ----------------------------------------------------------------------------------------------------------------------------------
def cml_forward_ref(Gu, Gi, Bi, u, i, j, l_w, l_b):
    """D, E and the regulariser of the triplets in fp64 (oracle.cml.distances / regulariser)."""
    Gu, Gi, Bi = (np.asarray(a, f64) for a in (Gu, Gi, Bi))
    D, E = oc.distances(Gu, Gi, Bi, u, i, j, dtype=f64)
    return D, E, oc.regulariser(Gu, Gi, Bi, u, i, j, l_w, l_b)


def cml_counts(D, E, D_all, E_all, margin):
    """Brute force over the [B, B_all] and [B_all, B] blocks of the pair matrix diff[a, b] = D_a + E_b:
    n_a = #{b : -80 <= diff <= margin} (equality counts: active), low_a = #{b : diff < -80}, m_b = #{a : -80 <= D_a + E_b <= margin}."""
    D, E, D_all, E_all = (np.asarray(a, f64) for a in (D, E, D_all, E_all))
    d1 = D[:, None] + E_all[None, :]
    n_a = ((d1 >= -80.0) & (d1 <= margin)).sum(1)
    low_a = (d1 < -80.0).sum(1)
    d2 = D_all[:, None] + E[None, :]
    m_b = ((d2 >= -80.0) & (d2 <= margin)).sum(0)
    return n_a, m_b, low_a


def cml_hinge_share(D, E, D_all, E_all, margin):
    """The local triplets' share of the hinge sum as the device splits it between ranks: the D part and the clipped constants of the pairs
    (a local, b global), the E part of the pairs (a global, b local).  For B_all = B this is sum max(margin - clip(D_a + E_b, -80, 1e8), 0)."""
    D, E, D_all, E_all = (np.asarray(a, f64) for a in (D, E, D_all, E_all))
    d1 = D[:, None] + E_all[None, :]
    act1 = (d1 >= -80.0) & (d1 <= margin)
    d2 = D_all[:, None] + E[None, :]
    act2 = (d2 >= -80.0) & (d2 <= margin)
    return float(np.sum(act1 * (margin - D)[:, None]) + np.sum(d1 < -80.0) * (margin + 80.0) - np.sum(act2 * E[None, :]))


def cml_hinge_full(D, E, margin):
    d = np.clip(np.asarray(D, f64)[:, None] + np.asarray(E, f64)[None, :], -80.0, 1e8)
    return float(np.maximum(margin - d, 0).sum())


def cml_grads_ref(Gu, Gi, Bi, u, i, j, D, E, D_all, E_all, l_w, l_b, margin):
    """-> (hinge share, dGu, dGi, dBi, (n_a, m_b, low_a)) in fp64: brute-force counts, oracle.cml.row_gradients."""
    n_a, m_b, low_a = cml_counts(D, E, D_all, E_all, margin)
    dGu, dGi, dBi = oc.row_gradients(Gu, Gi, Bi, u, i, j, -n_a.astype(f64), -m_b.astype(f64), l_w, l_b, dtype=f64)
    return cml_hinge_share(D, E, D_all, E_all, margin), dGu, dGi, dBi, (n_a, m_b, low_a)


def cml_tables(seed, U, I, F):
    rs = np.random.RandomState(seed)
    return dyadic(rs, (U, F)), dyadic(rs, (I, F)), dyadic(rs, (I,))


def cml_triplets(rs, Gi, U, B, hot=None, hot_count=0):
    """B triplets whose positive and negative rows differ (a coefficient on gi - gj = 0 would be invisible); `hot_count` of the positives are
    item `hot`."""
    I = Gi.shape[0]
    u, i, j = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, I, B)
    if hot is not None:
        i[rs.permutation(B)[:hot_count]] = hot
    for _ in range(100):
        same = ~(Gi[i] != Gi[j]).any(1)
        if not same.any():
            return u, i, j
        j[same] = rs.randint(0, I, int(same.sum()))
    raise AssertionError("no negative with another row found")


def cml_forward_budget(Gu, Gi, Bi, u, i, j, l_w):
    """D, E and the l_w part of the regulariser are exact in fp32: -> the largest sum met, in quanta."""
    for a in (Gu, Gi, Bi):
        _on_grid(a, QT, "table")
    _on_grid(np.log2(l_w) if l_w else 0.0, 1.0, "log2 l_w")
    q = QT * QT
    sp = np.sum((Gu[u] - Gi[i]) ** 2, -1) + np.sum((Gu[u] - Gi[j]) ** 2, -1)
    sq = np.sum(Gu[u] ** 2 + Gi[i] ** 2 + Gi[j] ** 2, -1)
    assert Gu[u].any(1).all() and Gi[i].any(1).all() and Gi[j].any(1).all()
    worst = max(sp.max() / q, sq.max() / q)
    assert worst < BUDGET, worst
    return worst


def cml_budget(Gu, Gi, Bi, u, i, j, D, E, D_all, E_all, l_w, margin):
    """The exactness budget of a grads_de case: dyadic tables, D / E on multiples of 1/8, l_w a power of two, l_b = 0.  Terms are taken in
    the expanded form (|c| (|u| + |i|) rather than |c| |u - i|), which covers the atomic kernel's and the sorted segments' order of operations.
    Every sample is visible through its l_w term (no gathered row is all zero) and its coefficient through gi != gj."""
    for a in (Gu, Gi, Bi):
        _on_grid(a, QT, "table")
    for a in (D, E, D_all, E_all, margin):
        _on_grid(a, 0.125, "D / E / margin")
    assert l_w > 0 and np.log2(l_w) == np.round(np.log2(l_w)) and l_w <= 1
    assert max(np.abs(D_all).max(), np.abs(E_all).max()) < 2 ** 20          # margin - D, -80 - D exact on the 1/8 grid
    assert Gu[u].any(1).all() and Gi[i].any(1).all() and Gi[j].any(1).all() and (Gi[i] != Gi[j]).any(1).all()
    n_a, m_b, _ = cml_counts(D, E, D_all, E_all, margin)
    q = QT * l_w
    c2 = 2.0 * n_a
    aGu, aGi, aGj = np.abs(Gu[u]), np.abs(Gi[i]), np.abs(Gi[j])
    sU, sI = np.zeros_like(Gu), np.zeros_like(Gi)
    np.add.at(sU, u, c2[:, None] * (aGi + aGj) + l_w * aGu)
    np.add.at(sI, i, c2[:, None] * (aGu + aGi) + l_w * aGi)
    np.add.at(sI, j, c2[:, None] * (aGu + aGj) + l_w * aGj)
    sB = np.bincount(i, m_b, minlength=len(Bi)) + np.bincount(j, m_b, minlength=len(Bi))
    worst = max(sU.max() / q, sI.max() / q, sB.max())
    assert worst < BUDGET, worst
    return worst


def cml_de(seed, B, B_all=None, lo=0, kind="ties"):
    """D, E of B local triplets and the gathered D_all, E_all (the local ones at [lo, lo + B)), all on multiples of 1/8, margin 0.5.
      ties     most E far above the hinge (inactive pairs, so the counts stay small), and planted: pairs with D_a + E_b = margin, margin -+ 1/8,
               -80, -80 -+ 1/8; a run of equal E values on the hinge and a run of equal D values
      clipped  every pair below the clip      inactive  no pair active"""
    rs = np.random.RandomState(seed)
    B_all = B if B_all is None else B_all
    D_all = rs.randint(-32, 33, B_all) / 8.0
    if kind == "clipped":
        E_all = -1000.0 - rs.randint(0, 64, B_all) / 8.0
    else:
        E_all = 1000.0 + rs.randint(0, 64, B_all) / 8.0
    if kind == "ties" and B_all >= 48:
        k = min(B_all // 4, 60)
        sel = rs.permutation(B_all)
        D_all[sel[:k // 2]] = 3.0                                  # a run of equal D values ...
        pick = rs.permutation(B_all)[:k]
        off = np.array([0.5, 0.5 - 0.125, 0.5 + 0.125, -80.0, -80.0 - 0.125, -80.0 + 0.125])
        E_all[pick] = off[np.arange(k) % 6] - D_all[sel[np.arange(k) % max(k // 2 + 3, 1)]]
        run = rs.permutation(B_all)[:min(B_all // 8, 40)]
        E_all[run] = 0.5 - 3.0                                     # ... against a run of equal E values exactly on the hinge
    elif kind == "ties":
        E_all[:] = np.array([0.5, 0.375, 0.625, -80.0, -80.125, -79.875, 0.5, -80.0])[np.arange(B_all) % 8] - D_all
    return D_all[lo:lo + B].copy(), E_all[lo:lo + B].copy(), D_all, E_all


def rescore_bound(Gu_rows, Gi_rows, Bi_vals, F):
    """|val - ref| of -sum (u - i)^2 + b_i in fp32: each difference rounds (2 u on its square), a sum of F terms, the final subtraction."""
    return (F + 4) * U_RND * (np.sum((Gu_rows - Gi_rows) ** 2, -1) + np.abs(Bi_vals))


def item_side_bound(Gi, Bi):
    F = Gi.shape[1]
    return (F + 2) * U_RND * (np.sum(Gi * Gi, -1) + np.abs(Bi))


def cml_reg_bound(Gu, Gi, Bi, u, i, j, l_w, l_b):
    """Regulariser with l_b != 0 on dyadic tables: the /10 and the two additions round, per triplet, before the fp64 sum."""
    per = 0.5 * l_w * np.sum(Gu[u] ** 2 + Gi[i] ** 2 + Gi[j] ** 2, -1) + 0.5 * l_b * Bi[i] ** 2 + 0.05 * l_b * Bi[j] ** 2
    return float(np.sum(6 * U_RND * per))


# ---- the cases of the GPU files ---------------------------------------------------------------------------------------------------------
PW_LAYOUT_F = (8, 7)                                               # vector and scalar path at lpt = 8
PW_CLASS_F = (4, 32, 36, 256, 260, 512, 516, 1024, 1, 9, 63, 65, 127, 129, 255)
PW_REFUSED_F = (257, 1028)
PW_BOUNDED_F = (8, 65, 260, 516)
PW_BOUNDED_KINDS = {"PMF": ("mse_sigmoid", False, 0.0, 0.0, ("both",)), "LogisticMF": ("logistic", True, 0.5, 2.0 ** -5, ("items", "users"))}
CML_FORWARD_F = (4, 32, 36, 256, 260, 516, 1024, 1, 9, 65, 129, 255)
CML_GRADS_F = (8, 7, 260, 65, 516)
CML_L_W = 2.0 ** -3
CML_MARGIN = 0.5
CML_TIE_SUMS = (0.5, 0.5 - 0.125, 0.5 + 0.125, -80.0, -80.0 - 0.125, -80.0 + 0.125)     # D_a + E_b planted by cml_de("ties")
LPT_TABLE = {(4, 4): (8, 1), (36, 4): (16, 1), (256, 4): (64, 1), (260, 4): (64, 2), (516, 4): (64, 4), (1024, 4): (64, 4), (65, 1): (64, 2),
             (129, 1): (64, 4), (257, 1): (None, None), (1028, 4): (None, None)}


def pw_exact_case(layout, F, bias):
    """-> namespace(w, u, i, y, n_global, plans, budget) of an exact point-wise case; layout: a name of LAYOUTS or "class"."""
    return _pw_exact_case(layout, F, bool(bias))


@functools.lru_cache(maxsize=None)
def _pw_exact_case(layout, F, bias):
    pu, pi = class_plans(F) if layout == "class" else layout_plans(layout, lanes(F)[1])
    w, u, i, y, n_global = pw_exact_inputs(1000 + F + 7 * len(layout) + bias, pu, pi, F, bias)
    assert_layout(u, pu), assert_layout(i, pi)
    return SimpleNamespace(w=w, u=u, i=i, y=y, n_global=n_global, plans=(pu, pi), budget=pw_budget(w, u, i, y, n_global))


@functools.lru_cache(maxsize=None)
def pw_bounded_case(layout, F, model):
    kind, bias, alpha, l_w, sides = PW_BOUNDED_KINDS[model]
    pu, pi = class_plans(F) if layout == "class" else layout_plans(layout, lanes(F)[1])
    w, u, i, y, n_global = pw_bounded_inputs(2000 + F + len(model), pu, pi, F, bias)
    assert_layout(u, pu), assert_layout(i, pi)
    return SimpleNamespace(w=w, u=u, i=i, y=y, n_global=n_global if kind != "logistic" else len(y), plans=(pu, pi), kind=kind, alpha=alpha,
                           l_w=l_w, sides=sides)


def pw_bounded_cases():
    """Every layout of LAYOUTS that cuts a row (F = 8: up to 513 pieces, each adding its cnt l_w own term for LogisticMF), and the lane classes."""
    return [(name, 8) for name in LAYOUTS if name not in ("tiny", "one")] + [("class", F) for F in PW_BOUNDED_F]


@functools.lru_cache(maxsize=None)
def cml_forward_case(F, B=300, U=64, I=48):
    Gu, Gi, Bi = cml_tables(3000 + F, U, I, F)
    u, i, j = cml_triplets(np.random.RandomState(F), Gi, U, B)
    return SimpleNamespace(Gu=Gu, Gi=Gi, Bi=Bi, u=u, i=i, j=j, budget=cml_forward_budget(Gu, Gi, Bi, u, i, j, CML_L_W))


@functools.lru_cache(maxsize=None)
def cml_grads_case(F, B, kind="ties", B_all=None, lo=0, hot=False, U=64, I=48):
    """An exact grads_de case (l_b = 0, l_w = 1/8, margin 0.5) with its fp64 reference.  B = 2047 takes the first 2047 triplets of the
    B = 2048 case.  hot: item 5 is the positive of enough triplets for its segment to be cut over more than lpt chunks of the sorted path."""
    Gu, Gi, Bi = cml_tables(3000 + F, U, I, F)
    gen = 2048 if B == 2047 else B
    lpt = lanes(F)[1]
    hc = min((lpt + 2) * CML_ITEM_CHUNK, gen // 2 + gen // 64) if hot else 0
    u, i, j = (a[:B] for a in cml_triplets(np.random.RandomState(gen + F), Gi, U, gen, hot=5 if hot else None, hot_count=hc))
    if hot and B >= CML_SORTED_FROM:
        rows, _, _, conts = layout_of(np.concatenate([i, j]), CML_ITEM_CHUNK)
        assert conts[rows == 5][0] > lpt, "the hot item is not a long-list row"
    D, E, D_all, E_all = cml_de(7 * B + F, B, B_all, lo, kind)
    if kind == "ties" and len(D_all) >= 48:                        # the planted sums are there, on both blocks of the pair matrix
        for s in CML_TIE_SUMS:
            assert (D[:, None] + E_all[None, :] == s).any() and (D_all[:, None] + E[None, :] == s).any(), ("planted tie lost", s)
    budget = cml_budget(Gu, Gi, Bi, u, i, j, D, E, D_all, E_all, CML_L_W, CML_MARGIN)
    hinge, dGu, dGi, dBi, counts = cml_grads_ref(Gu, Gi, Bi, u, i, j, D, E, D_all, E_all, CML_L_W, 0.0, CML_MARGIN)
    return SimpleNamespace(Gu=Gu, Gi=Gi, Bi=Bi, u=u, i=i, j=j, D=D, E=E, D_all=D_all, E_all=E_all, budget=budget, hinge=hinge, dGu=dGu, dGi=dGi,
                           dBi=dBi, counts=counts)


# (F, B, kind, B_all, lo, hot) of tests/test_gpu_cml_edges.py's grads_de cases
CML_GRADS_CASES = ([(F, B, "ties", None, 0, True) for F in CML_GRADS_F for B in (2047, 2048)] +
                   [(8, 300, "ties", None, 0, False), (8, 300, "clipped", None, 0, False), (8, 300, "inactive", None, 0, False),
                    (8, 300, "ties", 700, 0, False), (7, 300, "ties", 700, 250, False), (8, 2100, "ties", 2600, 250, True),
                    (8, 1, "ties", None, 0, False), (65, 1, "ties", 5, 2, False)])
