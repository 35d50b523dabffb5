"""The plugin surface against what the REAL host framework does: on a synthetic TSV, the reference's own
DataSetLoader + Splitter + DataSet and its Evaluator produced tests/golden/host_boundary_ref.npz (oracle/gen_golden_host_boundary.py,
run against the reference checkout).  Here, stand-alone: our array data plane (el_host_split_flags / el_host_pyset_order / vectorised
CSR) builds the same ids, split and matrices; our RecMixin / BaseRecommenderModel / init_charger, driven the way elliot/run.py:61-75
and hyperoptimization/model_coordinator.py:62-65 drive a model class, give the recommendation dicts the reference's
get_single_recommendation would build, and their evaluation equals the reference Evaluator's; folders and the recommendation writer
leave the reference's layout.  No GPU: the inner `_model` is a stub that ranks by a fixed score table."""
import inspect
import os
from types import SimpleNamespace

import numpy as np
import torch

from oracle.gen_golden_host_boundary import CUTOFFS, METRICS, TOP_K, expected_recs, stub_scores, write_dataset_tsv


def _dict_of(u, i, r):
    d = {}
    for a, b, c in zip(u.tolist(), i.tolist(), r.tolist()):
        d.setdefault(a, {})[b] = c
    return d


def test_plugin_surface_inside_the_reference_host(golden, tmp_path):
    ref = golden("host_boundary_ref.npz")
    tsv = str(tmp_path / "dataset.tsv")
    write_dataset_tsv(tsv)
    from elliot_amd.dataset.dataset import default_config, load_tsv_dataset
    from elliot_amd.recommender.base_recommender_model import BaseRecommenderModel, init_charger, param
    from elliot_amd.recommender.recommender_utils_mixin import RecMixin

    config = default_config(top_k=TOP_K, cutoffs=CUTOFFS, simple_metrics=METRICS, out_dir=str(tmp_path))
    config.path_log_folder = str(tmp_path / "log")
    for d in ("log", "recs", "weights"):
        os.makedirs(tmp_path / d, exist_ok=True)
    data = load_tsv_dataset(config, tsv, 0.2, 42)

    # our TSV -> split -> id maps -> CSR equals the reference's DataSetLoader / Splitter / DataSet on the same file
    assert list(data.users) == ref["users"].tolist() and list(data.items) == ref["items"].tolist()
    assert int(data.transactions) == int(ref["transactions"][0]) and data.num_users == 120 and data.num_items > 250
    assert [data.private_users[u] for u in range(data.num_users)] == ref["private_users"].tolist()
    assert [data.private_items[i] for i in range(data.num_items)] == ref["private_items"].tolist()
    sp = data.sp_i_train.tocsr()
    assert np.array_equal(sp.indptr, ref["sp_i_train_indptr"]) and np.array_equal(sp.indices, ref["sp_i_train_indices"])
    assert np.array_equal(sp.data.astype(np.float64), ref["sp_i_train_data"])
    assert {u: dict(v) for u, v in data.train_dict.items()} == _dict_of(ref["train_u"], ref["train_i"], ref["train_r"])
    ref_test = _dict_of(ref["test_u"], ref["test_i"], ref["test_r"])
    assert {u: dict(v) for u, v in data.test_dict.items() if v} == ref_test
    assert np.array_equal(np.asarray(data.allunrated_mask, dtype=bool), ref["allunrated_mask"])
    ip, cols, vals = data.split_csr(False)
    pu, pi = data.public_users, data.public_items
    for u, its in ref_test.items():
        row = {int(c): float(v) for c, v in zip(cols[ip[pu[u]]:ip[pu[u] + 1]], vals[ip[pu[u]]:ip[pu[u] + 1]]) if c < data.num_items}
        assert row == {pi[i]: float(r) for i, r in its.items() if i in pi}, u

    class StubScores:
        """Inner `_model`: a fixed [U, I] score table ranked under the tagged CSR mask get_candidate_mask() hands over
        (("excl", CSR) = every item NOT in the row, the allunrated_mask semantics of dataset.py:245)."""

        def __init__(self, U, I):
            self.ctx = SimpleNamespace(device=torch.device("cpu"))
            self.S = stub_scores(U, I)
            self.saved = None

        def recommend(self, mask, k, start, stop):
            kind, csr = mask
            S = self.S[start:stop].copy()
            ip, ix = csr.indptr.numpy(), csr.indices.numpy()
            allowed = np.zeros_like(S, dtype=bool)
            for r, u in enumerate(range(start, stop)):
                allowed[r, ix[ip[u]:ip[u + 1]]] = True
            if kind == "excl":
                allowed = ~allowed
            S[~allowed] = -np.inf
            idx = np.argsort(-S, axis=1, kind="stable")[:, :k].astype(np.int32)
            return torch.from_numpy(idx), torch.from_numpy(np.take_along_axis(S, idx, 1))

        def save_weights(self, path):
            self.saved = path

    class StubModel(RecMixin, BaseRecommenderModel):
        @init_charger
        def __init__(self, data, config, params, *args, **kwargs):
            self._params_list = [param("factors", "f", 8)]
            self.autoset_params()
            self._model = StubScores(self._num_users, self._num_items)
            self._sampler = None

        @property
        def name(self):
            return "StubModel_" + self.get_base_params_shortcut() + "_" + self.get_params_shortcut()

    params = SimpleNamespace(meta=SimpleNamespace(save_recs=True, save_weights=True, validation_metric="nDCG@10"),
                             epochs=1, batch_size=64, seed=42, factors=8)
    model = StubModel(data=data, config=config, params=params)            # model_coordinator.py:62
    model.evaluate(it=0, loss=1.5)                                       # -> get_recommendations -> Evaluator.eval -> recs TSV
    res = model.get_results()
    _, test_recs = model.get_recommendations(TOP_K)
    # the dicts are what the reference's own get_single_recommendation would have produced for the same scores
    exp = expected_recs(model._model.S, ref["allunrated_mask"], ref["private_users"].tolist(), ref["private_items"].tolist())
    assert set(test_recs) == set(exp) and all(test_recs[u] == exp[u] for u in exp)
    # ... and their evaluation is the reference Evaluator's on the same lists
    for c in CUTOFFS:
        for m in METRICS:
            assert abs(float(res[c]["test_results"][m]) - float(ref[f"ref_{m}@{c}"][0])) < 1e-15, (m, c)
    assert 0 <= res[5]["test_results"]["Precision"] <= 1
    files = sorted(os.listdir(config.path_output_rec_result))
    assert len(files) == 1 and files[0].endswith("_it=1.tsv")
    first = open(os.path.join(config.path_output_rec_result, files[0])).readline().rstrip("\n").split("\t")
    assert len(first) == 3
    assert os.path.isdir(os.path.join(config.path_output_rec_weight, model.name))
    assert os.path.basename(model._model.saved or "").startswith("best-weights-StubModel_")
    assert int(getattr(params, "best_iteration", -1)) == 1 and params.name.startswith("StubModel_seed=42_e=1_bs=64")
    assert list(inspect.signature(RecMixin.get_single_recommendation).parameters) == ["self", "mask", "k", "predictions", "offset", "offset_stop"]


def test_get_single_recommendation_has_the_reference_signature():
    from elliot_amd.recommender.recommender_utils_mixin import RecMixin
    assert list(inspect.signature(RecMixin.get_single_recommendation).parameters) == ["self", "mask", "k", "predictions", "offset", "offset_stop"]
