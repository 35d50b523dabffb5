"""Fixtures of the beyond-accuracy metric tests: the golden cases of scripts/gen_golden_metrics_beyond.py as the data object and
the recommendation dicts the stand-alone Evaluator takes, and a random-case generator for the device tests."""
import os
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "metrics_beyond_ref.npz")
INT_METRICS = ("ItemCoverage", "UserCoverage")


def load():
    return np.load(GOLDEN, allow_pickle=False)


class Data:
    """What the Evaluator reads of a DataSet, with identity id maps, from CSR arrays."""

    def __init__(self, U, I, train, test, k, cutoffs, threshold, metrics, val=None, transactions=None):
        qp, qc = train
        self.num_users, self.num_items = int(U), int(I)
        self.sp_i_train = sp.csr_matrix((np.ones(len(qc), np.float32), np.asarray(qc, np.int32), np.asarray(qp, np.int64)), shape=(U, I))
        self.transactions = int(len(qc)) if transactions is None else int(transactions)
        self.private_users = self.public_users = {u: u for u in range(U)}
        self.private_items = self.public_items = {i: i for i in range(I)}
        self._splits = {False: test, True: val}
        ev = SimpleNamespace(simple_metrics=list(metrics), relevance_threshold=threshold, cutoffs=list(cutoffs), paired_ttest=False,
                             complex_metrics=[])
        self.config = SimpleNamespace(top_k=int(k), evaluation=ev, config_test=True)

    def split_csr(self, validation=False):
        s = self._splits[validation]
        if s is None:
            return None
        return np.asarray(s[0], np.int64), np.asarray(s[1], np.int32), np.asarray(s[2], np.float32)

    def _dict(self, validation):
        s = self.split_csr(validation)
        if s is None:
            return None
        tp, tc, tr = s
        return {u: {int(i): float(r) for i, r in zip(tc[tp[u]:tp[u + 1]], tr[tp[u]:tp[u + 1]])} for u in range(self.num_users) if tp[u + 1] > tp[u]}

    def get_test(self):
        return self._dict(False)

    def get_validation(self):
        return self._dict(True)


def golden_case(z, tag, metrics):
    U, I, k = (int(v) for v in z[f"{tag}_shape"])
    data = Data(U, I, (z[f"{tag}_train_indptr"], z[f"{tag}_train_indices"]),
                (z[f"{tag}_test_indptr"], z[f"{tag}_test_indices"], z[f"{tag}_test_ratings"]), k, z[f"{tag}_cutoffs"].tolist(),
                float(z[f"{tag}_threshold"]), metrics, transactions=int(z[f"{tag}_transactions"]))
    return data, z[f"{tag}_lists"].astype(np.int32)


def recs_of(lists):
    k = lists.shape[1]
    return {u: [(int(i), float(k - c)) for c, i in enumerate(row) if i >= 0] for u, row in enumerate(lists)}


def check_against(got, names, ref_values, tol, what):
    """got: {name: value}; ref_values aligned with names.  Integer metrics exactly, the others within tol * max(1, |ref|)."""
    for m, ref in zip(names, ref_values):
        v = got[m]
        if m in INT_METRICS:
            assert isinstance(v, int) and v == int(ref), (what, m, v, ref)
        else:
            err = abs(v - ref)
            print(f"{what} {m}: {v!r} vs {ref!r}, |diff| {err:.3g}")
            assert err <= tol * max(1.0, abs(ref)), (what, m, v, ref, err)


def random_case(U, I, k, seed, big_user=None, empty_user=None):
    """Zipf-ish train rows, held-out rows of 1-6 items rated 1-5 outside them, popularity-biased lists with planted hits and -1 tails."""
    r = np.random.RandomState(seed)
    w = 1.0 / np.arange(1, I + 1) ** 0.8
    w = (w / w.sum())[r.permutation(I)]
    cdf = np.cumsum(w)
    train, test, lists = [], [], np.full((U, k), -1, dtype=np.int32)
    for u in range(U):
        tr_items = np.unique(np.searchsorted(cdf, r.rand(r.randint(3, 40))).clip(0, I - 1))
        rest = np.setdiff1d(np.arange(I), tr_items)
        n_held = 1500 if u == big_user else (0 if u == empty_user or r.randint(9) == 0 else r.randint(1, 7))
        held = np.sort(r.choice(rest, size=min(n_held, rest.shape[0]), replace=False))
        ratings = r.randint(1, 6, size=held.shape[0]).astype(np.float32)
        pool = np.unique(np.searchsorted(cdf, r.rand(4 * k + 8)).clip(0, I - 1))
        pool = np.setdiff1d(pool, tr_items)
        r.shuffle(pool)
        lst = list(pool[:k])
        for i in held[:3]:
            if i not in lst and lst and r.rand() < 0.6:
                lst[r.randint(len(lst))] = i
        n = len(lst) if r.randint(6) else r.randint(0, len(lst) + 1)
        lists[u, :n] = lst[:n]
        train.append(tr_items)
        test.append((held, ratings))
    qp = np.concatenate([[0], np.cumsum([len(t) for t in train])]).astype(np.int64)
    tp = np.concatenate([[0], np.cumsum([len(t[0]) for t in test])]).astype(np.int64)
    return ((qp, np.concatenate(train).astype(np.int32)),
            (tp, np.concatenate([t[0] for t in test]).astype(np.int32), np.concatenate([t[1] for t in test]).astype(np.float32)), lists)
