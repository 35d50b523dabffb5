"""Stand-alone evaluator with the interface of elliot/evaluation/evaluator.py:37-162 for the accuracy
metrics a latent-factor experiment normally asks for (nDCG, Precision, Recall, HR, MAP, MRR, F1) and the
beyond-accuracy metrics of the reference's default configuration (ItemCoverage, UserCoverage, NumRetrieved, Gini,
SEntropy, EFD, EPC, ARP, APLT, ACLT, PopREO, PopRSP: evaluation/beyond.py).

Definitions follow the reference:
  relevance          test items with rating >= relevance_threshold            relevance.py:87-96
  nDCG gain          2**(rating - threshold + 1) - 1, discount ln2/ln(rank+2) relevance.py:49-55,71-82
  IDCG               the user's gains sorted descending, first min(n, cutoff)  ndcg.py:68-79
  Precision / Recall hits / cutoff ; hits / #relevant                         precision.py:66, recall.py:66
  HR, MAP, MRR, F1   hit_rate.py:66, map.py:69-80, mrr.py:63-70, f1.py:56-68
  averaging          over users that have recommendations AND >= 1 relevant test item (ndcg.py:124-125)
Computation is vectorised over an [n_users, k] item matrix instead of per-user Python loops.  The remaining
metrics of the reference (nDCGRendle2020, MAR, DSC, the rating-error metrics, paired tests) are out of scope here; inside an
Elliot process the genuine Evaluator is used instead (recommender/_compat.py).

`evaluation.complex_metrics` holds the fairness family (RSP, REO, BiasDisparityBS / BR / BD, the four MADs: evaluation/fairness.py)
with the reference's keys; their values follow the simple metrics in configuration order under the reference's names.  The
validation metric reads simple_metrics only, as in the reference.

AUC, GAUC and LAUC (evaluation/ranks.py) are accepted only with `evaluation.rank_metrics: True`: they need the position of
every held-out item in the user's complete ranking, which costs one more full-catalogue pass per evaluation (el_rank.hip)
beside the top-k pass.  Full-length lists are never requested: get_needed_recommendations() stays top_k, the positions come
from the models' rank() (eval_device) or from the caller (eval(recs, ranks=...)), never from truncated lists.

The accuracy metrics average over the users with >= 1 relevant held-out item; the beyond-accuracy metrics see every
user whose held-out row is non-empty (evaluator.py:121) and average over either population, as their classes do.
"""
import logging
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from . import beyond, fairness, ranks

ACCURACY = ("nDCG", "Precision", "Recall", "HR", "MAP", "MRR", "F1")
SUPPORTED = ACCURACY + beyond.NAMES


class EvalBlock(namedtuple("EvalBlock", "first idx_val idx_test pos_val pos_test val_val val_test", defaults=(None,) * 4)):
    """One block of eval_device: the [n, k] index tensors of users first ..., optionally the positions of the held-out entries
    (rank metrics) and the fp32 score tensors of the lists (UserMADrating / ItemMADrating)."""
    __slots__ = ()


def _block_fields(block):
    """(first, idx_val, idx_test, pos_val, pos_test, val_val, val_test) of an EvalBlock or of a plain tuple of 3 or 5."""
    if isinstance(block, EvalBlock):
        return tuple(block)
    return tuple(block[:5]) + (None,) * (7 - min(len(block), 5))


def _canon(name, rank_metrics=False):
    for s in SUPPORTED + (ranks.NAMES if rank_metrics else ()):
        if s.lower() == name.lower():
            return s
    hint = ""
    if any(s.lower() == name.lower() for s in ranks.NAMES):
        hint = f"; {ranks.NAMES} need `evaluation.rank_metrics: True` (one more full-catalogue pass per evaluation)"
    raise Exception(f"Metric {name} is not available in the stand-alone evaluator (supported: {SUPPORTED}){hint}")


class _Split:
    """One held-out split ({public_user: {public_item: rating}}) in array form."""

    def __init__(self, test, threshold):
        self.users = [u for u, items in test.items() if any(r >= threshold for r in items.values())]
        self.row = {u: n for n, u in enumerate(self.users)}
        self.rel = [{i: r for i, r in test[u].items() if r >= threshold} for u in self.users]
        self.threshold = threshold


class Evaluator:
    def __init__(self, data, params):
        cfg = data.config
        self._data, self._params = data, params
        self._k = getattr(cfg.evaluation, "cutoffs", [cfg.top_k])
        self._k = self._k if isinstance(self._k, list) else [self._k]
        if any(np.array(self._k) > cfg.top_k):
            raise Exception("Cutoff values must be smaller than recommendation list length (top_k)")
        self._rel_threshold = getattr(cfg.evaluation, "relevance_threshold", 0)
        gate = bool(getattr(cfg.evaluation, "rank_metrics", False))
        self._metrics = [_canon(m, gate) for m in cfg.evaluation.simple_metrics]
        self._rank = [m for m in self._metrics if m in ranks.NAMES]
        self.rank_metrics = bool(self._rank)      # RecMixin: evaluate on the device and hand eval_device positions
        self._accuracy = [m for m in self._metrics if m in ACCURACY]
        self._beyond = [m for m in self._metrics if m in beyond.NAMES]
        complex_metrics = getattr(cfg.evaluation, "complex_metrics", None) or []
        self._fair = fairness.Plan(complex_metrics, data) if complex_metrics else None     # raises on an unknown complex metric
        self.needs_scores = bool(self._fair and self._fair.needs_scores)      # RecMixin: hand eval_device the lists' scores
        self._fair_bs, self._fair_dev, self._fair_warned = {}, None, False
        self._item_tables = None
        self._host_csr = {}
        self._dict_splits = None          # the dict-based form is only built when eval() is handed recommendation dicts
        self._needed_recommendations = cfg.top_k

    def _splits(self):
        if self._dict_splits is None:
            data = self._data
            val = data.get_validation() if hasattr(data, "get_validation") else None
            self._dict_splits = (_Split(data.get_test(), self._rel_threshold), _Split(val, self._rel_threshold) if val else None)
        return self._dict_splits

    @property
    def _test(self):
        return self._splits()[0]

    @property
    def _val(self):
        return self._splits()[1]

    def get_needed_recommendations(self):
        return self._needed_recommendations

    # ---- device path: metrics straight from the [users, k] index tensors --------------------------
    supports_device = True

    def device_sets(self, data, device):
        """Held-out splits as device CSRs in PRIVATE ids (rows = the model's user order).  Test items the model has no
        row for get ids >= num_items: never recommended, but they count as relevant items like in the reference."""
        if getattr(self, "_dev_sets", None) is None:
            from .. import ops
            if hasattr(data, "split_csr"):                 # array data plane: no dicts on the way to the device
                test = data.split_csr(False)
                val = data.split_csr(True)
                self._dev_sets = {"test": ops.DeviceTestSet(*test, device),
                                  "val": ops.DeviceTestSet(*val, device) if val is not None and val[1].shape[0] else None}
                return self._dev_sets
            self._dev_sets = {"test": self._split_to_csr(ops, data, self._test_dict_raw(data, False), device)}
            raw_val = self._test_dict_raw(data, True)
            self._dev_sets["val"] = self._split_to_csr(ops, data, raw_val, device) if raw_val else None
        return self._dev_sets

    @staticmethod
    def _test_dict_raw(data, validation):
        if validation:
            return data.get_validation() if hasattr(data, "get_validation") else None
        return data.get_test()

    @staticmethod
    def _split_arrays(data, split):
        """A {public_user: {public_item: rating}} split as CSR arrays in private ids (what DataSet.split_csr returns)."""
        pu, pi = data.public_users, data.public_items
        U, I = data.num_users, data.num_items
        rows = [[] for _ in range(U)]
        unknown = {}
        for u, items in split.items():
            if u not in pu:
                continue
            r = rows[pu[u]]
            for it, rating in items.items():
                col = pi.get(it)
                if col is None:
                    col = unknown.setdefault(it, I + len(unknown))
                r.append((col, rating))
        indptr = np.zeros(U + 1, dtype=np.int64)
        cols, vals = [], []
        for u, r in enumerate(rows):
            r.sort()
            indptr[u + 1] = indptr[u] + len(r)
            cols.extend(c for c, _ in r)
            vals.extend(v for _, v in r)
        return indptr, np.asarray(cols, dtype=np.int32), np.asarray(vals, dtype=np.float32)

    @classmethod
    def _split_to_csr(cls, ops, data, split, device):
        return ops.DeviceTestSet(*cls._split_arrays(data, split), device)

    def item_tables(self, data):
        """Popularity, short head and the two novelty tables of the data set (beyond.ItemTables), built once."""
        if self._item_tables is None:
            self._item_tables = beyond.ItemTables(data.sp_i_train, data.transactions, data.num_users)
        return self._item_tables

    def eval_device(self, ctx, data, blocks):
        """blocks: iterable of (first_private_user, idx_val, idx_test) with [n, k] int32 device tensors (idx_val may be
        the same tensor), or (first, idx_val, idx_test, pos_val, pos_test) where pos_* are the int32 positions of the block's
        held-out entries (the models' rank() on device_sets()["val" | "test"]; pos_val None without a validation split).
        An EvalBlock carries the same fields by name and, optionally, val_val / val_test: the float score tensors of the lists,
        required when UserMADrating / ItemMADrating are configured.
        Returns the same structure as eval().  AUC and GAUC do not depend on the cutoff; LAUC does.

        With complex_metrics, el_fair_metrics + el_group_sums run per block and (pass, split, cutoff) into integer tables, the
        hit arrays of the held-out entries (8 bytes per entry) and the histogram of the lists of R (4 bytes per item);
        el_fair_item_finish runs after the last block ("Fairness metrics").

        The accuracy kernel runs as before.  When a beyond-accuracy metric is asked for, el_beyond_metrics runs beside it
        into one item histogram (int32[num_items]) and one row of sums per (split, cutoff); the histograms are finished
        after the last block.  SEntropy needs the finished histogram and therefore a second pass over the lists: only when
        it is requested the blocks' index tensors are kept alive until then -- users x top_k x 4 bytes per split (400 MB at
        10 M users x 10)."""
        from .. import ops
        import torch
        sets = self.device_sets(data, ctx.device)
        keys = [(sp, c) for sp in ("val", "test") if sets[sp] is not None for c in self._k]
        acc = {key: torch.zeros(8, dtype=torch.float64, device=ctx.device) for key in keys}
        bey = None
        if self._beyond:
            from ..recommender.masks import device_masks
            train = device_masks(data, ctx).train
            tables = getattr(self, "_dev_tables", None)
            if tables is None or tables.pop.device != ctx.device:
                tables = self._dev_tables = ops.DeviceItemTables(self.item_tables(data), ctx.device)
            bey = {key: (torch.zeros(ops.BEYOND_SUMS, dtype=torch.float64, device=ctx.device),
                         torch.zeros(tables.num_items, dtype=torch.int32, device=ctx.device)) for key in keys}
        rnk = None
        if self._rank:
            from ..recommender.masks import device_masks
            rank_train = device_masks(data, ctx).train
            rnk = {key: torch.zeros(ops.RANK_SUMS, dtype=torch.float64, device=ctx.device) for key in keys}
        kept = {"val": [], "test": []} if "SEntropy" in self._beyond else None
        fair = self._fair_device(ctx, data, sets, keys) if self._fair else None
        for block in blocks:
            first, idx_val, idx_test, pos_val, pos_test, sc_val, sc_test = _block_fields(block)
            if rnk is not None and pos_test is None:
                raise Exception(f"{self._rank} need the positions of the held-out items: blocks of (first, idx_val, idx_test, pos_val, pos_test)")
            if self.needs_scores and (sc_test is None or (sets["val"] is not None and sc_val is None)):
                raise Exception("UserMADrating / ItemMADrating need the scores of the lists: blocks of EvalBlock(first, idx_val, idx_test, "
                                "val_val=..., val_test=...)")
            for sp, c in keys:
                idx = idx_val if sp == "val" else idx_test
                if fair is not None:
                    sc = (sc_val if sp == "val" else sc_test) if self.needs_scores else None
                    if sc is not None and sc.dtype != torch.float32:
                        sc = sc.float()                       # the kernels read fp32 scores (fp64 scorers: rounded once, here)
                    for (items, users), state in zip(fair["groups"], fair["state"][(sp, c)]):
                        ops.fair_metrics(ctx, idx, sc, sets[sp], fair["train"], items, users, self._rel_threshold, c, data.num_items,
                                         state, u_start=first)
                if rnk is not None:
                    pos = pos_val if sp == "val" else pos_test
                    ops.rank_metrics(ctx, pos, sets[sp], self._rel_threshold, rank_train, data.num_items, c, u_start=first,
                                     u_stop=first + idx.shape[0], sums=rnk[(sp, c)])
                if self._accuracy:
                    ops.rec_metrics(ctx, idx, sets[sp], self._rel_threshold, c, u_start=first, sums=acc[(sp, c)])
                if bey is not None:
                    ops.beyond_metrics(ctx, idx, sets[sp], train, tables, self._rel_threshold, c, u_start=first,
                                       sums=bey[(sp, c)][0], hist=bey[(sp, c)][1])
            if kept is not None:
                for sp in kept:
                    if sets[sp] is not None:
                        kept[sp].append((first, idx_val if sp == "val" else idx_test))
        extra = {}
        if bey is not None:
            for (sp, c), (sums, hist) in bey.items():
                stats, nov = ops.beyond_hist_finish(ctx, hist)
                ent = torch.zeros(1, dtype=torch.float64, device=ctx.device)
                if kept is not None:
                    for first, idx in kept[sp]:
                        ops.beyond_entropy(ctx, idx, sets[sp], nov, c, u_start=first, total=ent)
                extra[(sp, c)] = (sums.cpu().numpy(), stats.cpu().numpy(), float(ent.cpu()[0]))
        fair_terms = {}
        if fair is not None:
            for key, states in fair["state"].items():
                for (items, _), state in zip(fair["groups"], states):
                    ops.fair_item_finish(ctx, sets[key[0]], fair["cols"][key[0]], items, self._rel_threshold, state)
                fair_terms[key] = [state.host_terms() for state in states]
        host = {key: v.cpu().numpy() for key, v in acc.items()}
        rank_host = {key: v.cpu().numpy() for key, v in rnk.items()} if rnk is not None else None

        def means(sp, c):
            out = {}
            if rank_host is not None:
                out = ranks.means(rank_host[(sp, c)])
                if not out:
                    return {}
            if self._accuracy:
                s = host[(sp, c)]
                if s[7] == 0:
                    return {}
                out.update({m: float(s[ops.METRIC_NAMES.index(m)] / s[7]) for m in self._accuracy})
            if self._beyond:
                sums, stats, ent = extra[(sp, c)]
                if sums[0] == 0:
                    return {}
                out.update(beyond.finish(self._beyond, sums, int(stats[0]), int(stats[1]), int(stats[2]), ent, data.num_items))
            out = {m: out[m] for m in self._metrics}
            if self._fair:
                out.update(fairness.finish(self._fair, fair_terms[(sp, c)], self._fair_bs))
            return out

        res = {}
        for c in self._k:
            test = means("test", c)
            val = means("val", c) if sets["val"] is not None else None
            if not val:
                val = test
            res[c] = {"val_results": val, "val_statistical_results": {}, "test_results": test, "test_statistical_results": {}}
        return res

    # ---------------------------------------------------------------------------------------------
    def _eval_split(self, recs, split, cutoff, validation=False, pos=None):
        """recs: {public_user: [(public_item, score), ...]}"""
        out = self._eval_accuracy(recs, split, cutoff) if self._accuracy else {}
        if self._accuracy and not out:
            return {}
        if self._rank:
            more = self._eval_ranks(pos, cutoff, validation)
            if not more:
                return {}
            out.update(more)
        if self._beyond:
            more = self._eval_beyond(recs, cutoff, validation)
            if not more:
                return {}
            out.update(more)
        out = {m: out[m] for m in self._metrics}
        if self._fair:
            out.update(self._eval_fair(recs, cutoff, validation))
        return out

    def _host_split_csr(self, validation):
        if validation not in self._host_csr:
            data = self._data
            if hasattr(data, "split_csr"):
                self._host_csr[validation] = data.split_csr(validation)
            else:
                self._host_csr[validation] = self._split_arrays(data, self._test_dict_raw(data, validation))
        return self._host_csr[validation]

    def _eval_ranks(self, pos, cutoff, validation):
        """AUC / GAUC / LAUC of one split from host positions: one int32 per entry of the split's CSR (_host_split_csr: rows =
        private users, ids ascending), what ranks.positions or the models' rank() give."""
        indptr, indices, ratings = self._host_split_csr(validation)
        pos = np.asarray(pos)
        if pos.shape[0] != indices.shape[0]:
            raise Exception(f"ranks: {pos.shape[0]} positions for {indices.shape[0]} held-out entries")
        train_len = np.diff(self._data.sp_i_train.tocsr().indptr)
        return ranks.finish(pos, indptr, ratings, self._rel_threshold, train_len, self._data.num_items, cutoff)[0]

    def _eval_beyond(self, recs, cutoff, validation):
        """The beyond-accuracy metrics of one split from the recommendation dicts, in NumPy (beyond.numpy_terms)."""
        data = self._data
        pu, pi = data.public_users, data.public_items
        users = [u for u in recs if u in pu]
        lists = np.full((len(users), cutoff), -1, dtype=np.int64)
        for r, u in enumerate(users):
            row = [pi.get(item, -1) for item, _ in recs[u][:cutoff]]
            lists[r, :len(row)] = row
        train = data.sp_i_train.tocsr()
        train.sort_indices()
        tables = self.item_tables(data)
        sums, hist, ent = beyond.numpy_terms(lists, np.array([pu[u] for u in users], dtype=np.int64), self._host_split_csr(validation),
                                             self._rel_threshold, (train.indptr.astype(np.int64), train.indices), tables, cutoff)
        if sums[0] == 0:
            return {}
        n, free, G = beyond.gini_numerator(hist, data.num_items)
        return beyond.finish(self._beyond, sums, n, free, G, ent, data.num_items)

    # ---- fairness metrics (evaluation.complex_metrics, fairness.py) ---------------------------------------------------------------
    def _fair_warn(self):
        """Held-out items the model has no row for (private ids >= num_items) belong to no item group on either route; the
        reference would count them in REO's denominator if the clustering file lists them.  Logged once, with their number."""
        if self._fair_warned:
            return
        self._fair_warned = True
        n = 0
        for validation in (False, True):
            split = self._host_split_csr(validation) if not validation or self._test_dict_raw(self._data, True) else None
            if split is not None:
                n += int((np.asarray(split[1]) >= self._data.num_items).sum())
        if n:
            logging.getLogger(__name__).warning(f"fairness metrics: {n} held-out entries are items without a train interaction; they "
                                                f"belong to no item group (REO's denominator leaves them out)")

    def _host_train_csr(self):
        train = self._data.sp_i_train.tocsr()
        train.sort_indices()
        return train.indptr.astype(np.int64), train.indices

    def _eval_fair(self, recs, cutoff, validation):
        """The complex metrics of one split from the recommendation dicts, in NumPy (fairness.numpy_terms)."""
        data = self._data
        self._fair_warn()
        pu, pi = data.public_users, data.public_items
        users = [u for u in recs if u in pu]
        lists = np.full((len(users), cutoff), -1, dtype=np.int64)
        scores = np.zeros((len(users), cutoff), dtype=np.float64)
        for r, u in enumerate(users):
            row = recs[u][:cutoff]
            lists[r, :len(row)] = [pi.get(item, -1) for item, _ in row]
            scores[r, :len(row)] = [score for _, score in row]
        train = self._host_train_csr()
        for n_pass in self._fair.needs_bs:
            if n_pass not in self._fair_bs:
                self._fair_bs[n_pass] = fairness.bs_counts(train, *self._fair.passes[n_pass])
        rows = np.array([pu[u] for u in users], dtype=np.int64)
        terms = [fairness.numpy_terms(lists, scores, rows, self._host_split_csr(validation), self._rel_threshold, train, ig, ug, cutoff,
                                      data.num_items) for ig, ug in self._fair.passes]
        return fairness.finish(self._fair, terms, self._fair_bs)

    def _fair_device(self, ctx, data, sets, keys):
        """Device copies of the groupings, the train CSR and the item-major held-out sets (built once), BiasDisparityBS's counts
        (once per data set) and fresh accumulators per (split, cutoff, pass)."""
        from .. import ops
        from ..recommender.masks import device_masks
        self._fair_warn()
        dev = self._fair_dev
        if dev is None or dev["device"] != ctx.device:
            dev = self._fair_dev = {
                "device": ctx.device, "train": device_masks(data, ctx).train,
                "groups": [(ops.DeviceGrouping(ig, ctx.device), ops.DeviceGrouping(ug, ctx.device)) for ig, ug in self._fair.passes],
                "cols": {sp: ops.DeviceTestColumns(*self._host_split_csr(sp == "val")[:2], data.num_items, ctx.device)
                         for sp in ("val", "test") if sets[sp] is not None}}
        for n_pass in self._fair.needs_bs:
            if n_pass not in self._fair_bs:
                self._fair_bs[n_pass] = ops.group_counts(ctx, dev["train"], data.num_items, *dev["groups"][n_pass]).cpu().numpy()
        state = {(sp, c): [ops.FairState(ctx, sets[sp], data.num_items, items, users) for items, users in dev["groups"]] for sp, c in keys}
        return {**dev, "state": state}

    def _eval_accuracy(self, recs, split, cutoff):
        users = [u for u in recs if u in split.row]
        if not users:
            return {}
        n = len(users)
        hits = np.zeros((n, cutoff), dtype=bool)
        gains = np.zeros((n, cutoff), dtype=np.float64)
        nrel = np.zeros(n, dtype=np.float64)
        idcg = np.zeros(n, dtype=np.float64)
        disc = np.array([math.log(2) / math.log(r + 2) for r in range(cutoff)])
        thr = split.threshold
        for r, u in enumerate(users):
            rel = split.rel[split.row[u]]
            nrel[r] = len(rel)
            g = sorted((2 ** (s - thr + 1) - 1 for s in rel.values()), reverse=True)[:cutoff]
            idcg[r] = float(np.dot(g, disc[:len(g)]))
            for c, (item, _) in enumerate(recs[u][:cutoff]):
                s = rel.get(item)
                if s is not None:
                    hits[r, c] = True
                    gains[r, c] = 2 ** (s - thr + 1) - 1
        nh = hits.sum(1)
        out = {}
        for m in self._accuracy:
            if m == "nDCG":
                dcg = gains @ disc
                v = np.where(dcg > 0, dcg / np.where(idcg > 0, idcg, 1.0), 0.0)
            elif m == "Precision":
                v = nh / cutoff
            elif m == "Recall":
                v = nh / nrel
            elif m == "HR":
                v = (nh > 0).astype(np.float64)
            elif m == "MAP":
                v = (np.cumsum(hits, 1) / np.arange(1, cutoff + 1)).mean(1)
            elif m == "MRR":
                first = np.argmax(hits, 1)
                v = np.where(nh > 0, 1.0 / (first + 1), 0.0)
            elif m == "F1":
                p, rc = nh / cutoff, nh / nrel
                v = np.where(p + rc > 0, 2 * p * rc / np.where(p + rc > 0, p + rc, 1.0), 0.0)
            out[m] = float(np.average(v))
        return out

    def eval(self, recommendations, ranks=None):
        """recommendations = (recs_val, recs_test); returns {cutoff: {"val_results", "test_results", ...}}
        exactly as evaluator.py:79-92 (a missing validation split mirrors the test results).
        ranks = (pos_val, pos_test): host positions of the held-out entries in the users' complete rankings, required when AUC /
        GAUC / LAUC are asked for -- they are never derived from the (truncated) recommendation lists."""
        if self._rank and ranks is None:
            raise Exception(f"{self._rank} need the positions of the held-out items in the complete rankings: eval(recs, ranks=(pos_val, "
                            f"pos_test)); lists of length top_k cannot give them")
        res = {}
        for k in self._k:
            val = self._eval_split(recommendations[0], self._val, k, validation=True, pos=ranks[0] if ranks else None) if self._val else None
            test = self._eval_split(recommendations[1], self._test, k, pos=ranks[1] if ranks else None)
            if not val:
                val = test
            res[k] = {"val_results": val, "val_statistical_results": {}, "test_results": test,
                      "test_statistical_results": {}}
        return res
