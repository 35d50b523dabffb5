"""Generate tests/golden/bprslim_ref.npz by RUNNING THE REFERENCE'S OWN BPRSlimModel and sampler (build machine only).

TEST INFRASTRUCTURE.  Needs the reference checkout (argument or $ELLIOT_REF); nothing at test time reads it.  bprslim_model.py and
custom_sampler.py are loaded BY FILE PATH (they import only pickle and numpy, so no stub modules are needed).  In the model
module's namespace `np` is replaced by a shim that is numpy with `empty` = numpy.zeros: the reference starts S from np.empty and
relies on fresh pages being zero; the start is DEFINED as zero here.  The reference files themselves are
untouched, and train_step, predict and get_user_recs run unmodified on the unmodified sampler's [1, 1] batches -- `batch_size: 1`,
the only one the reference's train_step runs with.  Before anything is written, the restatement the tests use
(tests/helpers/bprslim_ref.py) must equal the reference's S, x and predictions bit for bit.

Cases (60 users x 40 items, EPOCHS epochs of `transactions` triplets each, every row stored in a shuffled dict order):
  plain        Zipf-ish popularity, every user rates something, lr 0.05                + plain_pred (the full prediction matrix)
  short_rows   several users with exactly one item (row i's only seen cell is skipped: only row j moves), one item nobody rated
  defaults     the reference's default hyper-parameters (lr 0.001, lj_reg 0.001, li_reg 0.1): the moves are tiny
No user holds every item: the sampler's `lui == n_items` branch recurses without returning.
Per case: <tag>_indptr / _indices / _ratings / _shape (the dict-order rows), _hyper (lr, lj_reg, li_reg), _trip int32 [E, 3, n],
_S float64 [E, I, I] (S after each epoch), _x float64 [E, n], _loss float64 [E] (the reference's running `loss` of each epoch),
_rec_idx / _rec_val (get_user_recs(u, all-unseen mask, 10) for every user, padded with (-1, -inf)), _d_reorder (the largest
difference between the reference's S and that of a twin whose chain is summed with math.fsum, over both epochs) and _fragile
(bool per user: a gap below 1e-9 inside the first eleven ranks, a tie included).  At most 5 % of a case's users may be fragile
(asserted): there the list depends on the last bits of S and the tests compare values only.

Run:  PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_bprslim.py <reference checkout>
"""
import importlib.util
import os
import sys
from types import SimpleNamespace

sys.dont_write_bytecode = True
import numpy
import scipy.sparse as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests.helpers import bprslim_ref  # noqa: E402

np = numpy
OUT = os.path.join(REPO, "tests", "golden", "bprslim_ref.npz")
K = 10
U, I = 60, 40
EPOCHS = {"plain": 2, "short_rows": 2, "defaults": 2}
HYPER = {"plain": (0.05, 0.001, 0.1), "short_rows": (0.05, 0.001, 0.1), "defaults": (0.001, 0.001, 0.1)}    # lr, lj_reg, li_reg
WITH_PRED = ("plain",)
SINGLE_USERS, COLD_ITEM = (3, 17, 18, 41, 59), 7
FRAGILE_GAP = 1e-9


class ZeroedNumpy(object):
    """numpy, except that empty() returns zeros."""

    def __getattr__(self, name):
        return numpy.zeros if name == "empty" else getattr(numpy, name)


def load_by_path(ref, name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_rows(seed, tag):
    """{user: {item: rating}} with every dict in a shuffled order."""
    rs = np.random.RandomState(seed)
    pop = 1.0 / np.arange(1, I + 1) ** 0.8
    p = np.minimum(0.6, 0.16 * pop / pop.mean())
    M = (rs.rand(U, I) < p[rs.permutation(I)][None, :]) * rs.randint(1, 6, (U, I))
    M[np.arange(U), rs.randint(0, I, U)] = rs.randint(1, 6, U)                  # every user rates something
    if tag == "short_rows":
        M[:, COLD_ITEM] = 0
        for u in SINGLE_USERS:
            M[u, :] = 0
            M[u, rs.choice(np.setdiff1d(np.arange(I), [COLD_ITEM]))] = 4
        for u in np.flatnonzero(M.sum(axis=1) == 0):
            M[u, (COLD_ITEM + 1 + u) % I] = 3
    assert (M > 0).sum(axis=1).min() >= 1 and (M > 0).sum(axis=1).max() < I - 1
    rows = {}
    for u in range(U):
        items = np.flatnonzero(M[u])
        rs.shuffle(items)
        rows[u] = {int(i): float(M[u, i]) for i in items}
    return rows


def main(ref):
    model_mod = load_by_path(ref, "ref_bprslim_model", "elliot/recommender/latent_factor_models/BPRSlim/bprslim_model.py")
    model_mod.np = ZeroedNumpy()
    sampler_mod = load_by_path(ref, "ref_custom_sampler", "elliot/dataset/samplers/custom_sampler.py")
    out = {"k": np.int64(K)}
    for seed, tag in enumerate(bprslim_ref.CASES):
        rows = make_rows(500 + seed, tag)
        lr, lj_reg, li_reg = HYPER[tag]
        indptr = np.concatenate([[0], np.cumsum([len(rows[u]) for u in range(U)])]).astype(np.int64)
        indices = np.asarray([i for u in range(U) for i in rows[u]], dtype=np.int32)
        ratings = np.asarray([r for u in range(U) for r in rows[u].values()], dtype=np.float64)
        n = len(indices)
        users = np.repeat(np.arange(U), np.diff(indptr))
        R = sp.csr_matrix((ratings, (users, indices)), dtype="float32", shape=(U, I))          # dataset.py builds it like this
        data = SimpleNamespace(sp_i_train_ratings=R, public_users={u: u for u in range(U)}, public_items={i: i for i in range(I)},
                               items=list(range(I)), transactions=n)
        sampler = sampler_mod.Sampler(rows)
        m = model_mod.BPRSlimModel(data, U, I, lr, lj_reg, li_reg, sampler, random_seed=42)
        assert not m._s_dense.any() and m._s_dense.dtype == np.float64
        sp_indptr, sp_indices = bprslim_ref.sorted_rows(indptr, indices)
        assert np.array_equal(m._mask_indptr, sp_indptr) and np.array_equal(m._mask_indices, sp_indices)   # scipy: rows ascending
        E = EPOCHS[tag]
        trip = np.empty((E, 3, n), dtype=np.int32)
        x_ref = np.empty((E, n), dtype=np.float64)
        S_ref = np.empty((E, I, I), dtype=np.float64)
        loss_ref = np.empty(E, dtype=np.float64)
        S_mine, S_twin = np.zeros((I, I)), np.zeros((I, I))
        d_reorder = 0.0
        for e in range(E):
            loss = 0
            for t, batch in enumerate(sampler.step(n, 1)):                     # bprslim.py:107-115 with batch_size 1
                assert all(b.shape == (1, 1) for b in batch)
                trip[e, :, t] = [int(b[0, 0]) for b in batch]
                before = m._s_dense[batch[1][0, 0], sp_indices[sp_indptr[batch[0][0, 0]]:sp_indptr[batch[0][0, 0] + 1]]] - \
                    m._s_dense[batch[2][0, 0], sp_indices[sp_indptr[batch[0][0, 0]]:sp_indptr[batch[0][0, 0] + 1]]]
                step_loss = m.train_step(batch)
                loss += step_loss
                xs = 0.0
                for v in before.tolist():
                    xs += v
                x_ref[e, t] = xs
                assert float(step_loss) == xs ** 2, (tag, e, t)               # the x the reference's own loss was made of
            S_ref[e] = m._s_dense
            loss_ref[e] = float(loss)
            # the restatement, bit for bit
            x_mine = bprslim_ref.train(S_mine, sp_indptr, sp_indices, trip[e], lr, li_reg, lj_reg)
            assert np.array_equal(S_mine.view(np.uint64), S_ref[e].view(np.uint64)), (tag, e)
            assert np.array_equal(x_mine.view(np.uint64), x_ref[e].view(np.uint64)), (tag, e)
            bprslim_ref.train(S_twin, sp_indptr, sp_indices, trip[e], lr, li_reg, lj_reg, chain="fsum")
            d_reorder = max(d_reorder, float(np.abs(S_twin - S_ref[e]).max()))
        assert not np.diag(m._s_dense).any()                                  # S[i, i] never moves
        lev, _, start = bprslim_ref.levels(trip[0, 1], trip[0, 2], I)
        pred = np.array([[m.predict(u, i) for i in range(I)] for u in range(U)], dtype=np.float64)
        mine = bprslim_ref.predictions(sp_indptr, sp_indices, S_ref[-1])
        assert np.array_equal(mine.view(np.uint64), pred.view(np.uint64)), tag
        # what each case is there for
        if tag == "short_rows":
            assert all(indptr[u + 1] - indptr[u] == 1 for u in SINGLE_USERS) and COLD_ITEM not in indices
            assert any(trip[0, 0, t] in SINGLE_USERS for t in range(n))
        assert not any(trip[e, 2, t] in rows[trip[e, 0, t]] for e in range(E) for t in range(n))      # never a seen j
        mask = np.ones((U, I), dtype=bool)
        mask[users, indices] = False
        idx = np.full((U, K), -1, np.int32)
        val = np.full((U, K), -np.inf, np.float64)
        fragile = np.zeros(U, dtype=bool)
        for u in range(U):
            r = m.get_user_recs(u, mask, K)
            idx[u, :len(r)] = [x[0] for x in r]
            val[u, :len(r)] = [x[1] for x in r]
            _, v = bprslim_ref.topk(pred[u], mask[u], K)
            assert np.array_equal(v.view(np.uint64), val[u].view(np.uint64)), (tag, u)
            fragile[u] = bprslim_ref.min_gap(pred[u], mask[u], K) < FRAGILE_GAP
        assert fragile.sum() <= 0.05 * U, (tag, int(fragile.sum()))
        print(f"{tag}: nnz {n}, {len(start) - 1} levels in epoch 1, d_reorder {d_reorder:.3e}, max |S| {np.abs(S_ref[-1]).max():.3e}, "
              f"losses {loss_ref.tolist()}, fragile users {int(fragile.sum())} of {U}")
        out.update({f"{tag}_indptr": indptr, f"{tag}_indices": indices, f"{tag}_ratings": ratings,
                    f"{tag}_shape": np.asarray([U, I], np.int64), f"{tag}_hyper": np.asarray([lr, lj_reg, li_reg], np.float64),
                    f"{tag}_trip": trip, f"{tag}_S": S_ref, f"{tag}_x": x_ref, f"{tag}_loss": loss_ref,
                    f"{tag}_rec_idx": idx, f"{tag}_rec_val": val, f"{tag}_d_reorder": np.float64(d_reorder),
                    f"{tag}_fragile": fragile})
        if tag in WITH_PRED:
            out[f"{tag}_pred"] = pred
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["ELLIOT_REF"])
