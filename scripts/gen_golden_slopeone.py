"""Generate tests/golden/slopeone_ref.npz by RUNNING THE REFERENCE'S OWN SlopeOneModel (build machine only).

TEST INFRASTRUCTURE.  Needs the reference checkout (argument or $ELLIOT_REF); nothing at test time reads it.  slope_one_model.py
is loaded BY FILE PATH (it imports only pickle and numpy, so no stub modules are needed).  In the loaded module's namespace `np`
is replaced by a shim that is numpy with `empty` = numpy.zeros: the reference starts freq and dev from np.empty and relies on
fresh pages being zero; the start is DEFINED as zero here.  The reference file itself is untouched, and its
initialize, predict and get_user_recs run unmodified.  Before anything is written, the vectorised restatement the tests use
(tests/helpers/slopeone_ref.py) must equal the reference's freq, dev, user_mean and every prediction bit for bit.

Cases (240 users x 84 items each, every row stored in a shuffled dict order):
  int          ratings 1..5                                                     + <tag>_pred (the full prediction matrix)
  half         ratings 0.5..5 in half steps                                     + <tag>_pred
  cold_item    ratings, one item nobody rated
  one_rating   ratings, one user with a single rating
  split        two item groups without a common rater: freq == 0 off the diagonal, (user, item) pairs with an empty Ri
Per case: <tag>_indptr / _indices / _ratings / _shape (the dict-order rows), <tag>_freq / _dev / _user_mean, and
<tag>_rec_idx / _rec_val: get_user_recs(u, all-unrated mask, 10) for every user, padded with (-1, -inf).
At most 5 % of a case's users may hold two equal values inside or at the edge of their top 10 (asserted): there the order of
the reference's argpartition is arbitrary and the tests compare values only.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_slopeone.py <reference checkout>
"""
import importlib.util
import os
import sys
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests.helpers import slopeone_ref  # noqa: E402

np = numpy
OUT = os.path.join(REPO, "tests", "golden", "slopeone_ref.npz")
K = 10
U, I = 240, 84
CASES = ("int", "half", "cold_item", "one_rating", "split")
WITH_PRED = ("int", "half")
SPLIT_ITEMS, SPLIT_USERS = 3, 6                 # the small group of the split case: its last items and users


class ZeroedNumpy(object):
    """numpy, except that empty() returns zeros."""

    def __getattr__(self, name):
        return numpy.zeros if name == "empty" else getattr(numpy, name)


def load_reference(ref):
    spec = importlib.util.spec_from_file_location(
        "ref_slope_one_model", os.path.join(ref, "elliot/recommender/algebric/slope_one/slope_one_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.np = ZeroedNumpy()
    return mod


def make_rows(seed, tag):
    """{user: {item: rating}} with every dict in a shuffled order."""
    rs = np.random.RandomState(seed)
    pop = 1.0 / np.arange(1, I + 1) ** 0.6
    p = np.minimum(0.4, 0.18 * pop / pop.mean())
    levels = np.arange(1, 11) * 0.5 if tag == "half" else np.arange(1, 6).astype(float)
    M = (rs.rand(U, I) < p[rs.permutation(I)][None, :]) * levels[rs.randint(0, len(levels), (U, I))]
    M[np.arange(U), rs.randint(0, I, U)] = levels[rs.randint(0, len(levels), U)]          # every user rates something
    if tag == "cold_item":
        M[:, 7] = 0
        M[M.sum(axis=1) == 0, 8] = 3.0
    if tag == "one_rating":
        M[11, :] = 0
        M[11, 30] = 4.0
    if tag == "split":
        M[:U - SPLIT_USERS, I - SPLIT_ITEMS:] = 0
        M[U - SPLIT_USERS:, :I - SPLIT_ITEMS] = 0
        for u in range(U):
            lo, hi = (0, I - SPLIT_ITEMS) if u < U - SPLIT_USERS else (I - SPLIT_ITEMS, I)
            if not M[u, lo:hi].any():
                M[u, rs.randint(lo, hi)] = levels[rs.randint(0, len(levels))]
        M[U - SPLIT_USERS:, I - SPLIT_ITEMS] = np.maximum(M[U - SPLIT_USERS:, I - SPLIT_ITEMS], 1.0)
    rows = {}
    for u in range(U):
        items = np.flatnonzero(M[u])
        rs.shuffle(items)
        rows[u] = {int(i): float(M[u, i]) for i in items}
    return rows


def main(ref):
    mod = load_reference(ref)
    out = {"k": np.int64(K)}
    for seed, tag in enumerate(CASES):
        rows = make_rows(300 + seed, tag)
        data = SimpleNamespace(num_items=I, num_users=U, i_train_dict=rows, public_users={u: u for u in range(U)},
                               private_items={i: i for i in range(I)})
        m = mod.SlopeOneModel(data)
        m.initialize()
        indptr = np.concatenate([[0], np.cumsum([len(rows[u]) for u in range(U)])]).astype(np.int64)
        indices = np.asarray([i for u in range(U) for i in rows[u]], dtype=np.int32)
        ratings = np.asarray([r for u in range(U) for r in rows[u].values()], dtype=np.float64)
        mean = np.asarray(m.user_mean, dtype=np.float64)
        assert m.freq.dtype == np.float64 and m.dev.dtype == np.float64 and all(type(x) is np.float64 for x in m.user_mean)
        pred = np.array([[m.predict(u, i) for i in range(I)] for u in range(U)], dtype=np.float64)
        # the restatement, bit for bit
        freq, dev, mean2 = slopeone_ref.build(indptr, indices, ratings, U, I)
        assert np.array_equal(freq, m.freq), tag
        assert np.array_equal(dev.view(np.uint64), m.dev.view(np.uint64)), tag
        assert np.array_equal(mean2.view(np.uint64), mean.view(np.uint64)), tag
        mine = slopeone_ref.predictions(indptr, indices, freq, dev, mean2)
        assert np.array_equal(mine.view(np.uint64), pred.view(np.uint64)), tag
        # what each case is there for
        off = ~np.eye(I, dtype=bool)
        if tag == "cold_item":
            assert not freq[7].any()
        if tag == "one_rating":
            assert indptr[12] - indptr[11] == 1
        if tag == "split":
            assert (freq[off] == 0).any() and np.signbit(dev[np.tril(freq == 0, -1)]).all()
            assert (pred[:U - SPLIT_USERS, I - 1] == mean[:U - SPLIT_USERS]).all()
        mask = np.ones((U, I), dtype=bool)
        mask[np.repeat(np.arange(U), np.diff(indptr)), indices] = False
        idx = np.full((U, K), -1, np.int32)
        val = np.full((U, K), -np.inf, np.float64)
        ties = 0
        for u in range(U):
            r = m.get_user_recs(u, mask, K)
            idx[u, :len(r)] = [x[0] for x in r]
            val[u, :len(r)] = [x[1] for x in r]
            _, v = slopeone_ref.topk(pred[u], mask[u], K)
            assert np.array_equal(v.view(np.uint64), val[u].view(np.uint64)), (tag, u)
            ties += slopeone_ref.has_tie(pred[u], mask[u], K)
        assert ties <= 0.05 * U, (tag, ties)
        print(f"{tag}: nnz {len(indices)}, users with a tie in or at the edge of the top {K}: {ties} of {U}")
        out.update({f"{tag}_indptr": indptr, f"{tag}_indices": indices, f"{tag}_ratings": ratings,
                    f"{tag}_shape": np.asarray([U, I], np.int64), f"{tag}_freq": m.freq, f"{tag}_dev": m.dev,
                    f"{tag}_user_mean": mean, f"{tag}_rec_idx": idx, f"{tag}_rec_val": val})
        if tag in WITH_PRED:
            out[f"{tag}_pred"] = pred
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["ELLIOT_REF"])
