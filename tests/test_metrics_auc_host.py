"""AUC, GAUC and LAUC on the host (evaluation/ranks.py, Evaluator.eval(recs, ranks=...)) against the reference's own Evaluator run
on full-length lists (tests/golden/metrics_auc_ref.npz, scripts/gen_golden_metrics_auc.py)."""
import numpy as np
import pytest

from elliot_amd.evaluation import ranks
from elliot_amd.evaluation.evaluator import Evaluator
from tests.helpers import rank_ref

Z = rank_ref.load()
CASES = [str(t) for t in Z["cases"]]
SPLITS = [(tag, name) for tag in CASES for name in ("test", "val") if f"{tag}_{name}_pos" in Z.files]


def _positions(tag, name):
    tp, tc, _ = rank_ref.split_of(Z, tag, name)
    return ranks.positions(Z[f"{tag}_scores"], rank_ref.admissible(Z, tag), (tp, tc))


@pytest.mark.parametrize("tag,name", SPLITS)
def test_positions_are_the_reference_lists_positions(tag, name):
    got = _positions(tag, name)
    ref = Z[f"{tag}_{name}_pos"]
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    tc = Z[f"{tag}_{name}_indices"]
    I = int(Z[f"{tag}_shape"][1])
    assert np.array_equal(got < 0, tc >= I)             # every held-out item with a model row is admissible in these fixtures
    if name == "test":
        assert (tc >= I).any()


@pytest.mark.parametrize("tag,name", SPLITS)
def test_finish_matches_the_reference(tag, name):
    tp, tc, tr = rank_ref.split_of(Z, tag, name)
    thr = float(Z[f"{tag}_threshold"])
    U, I = (int(v) for v in Z[f"{tag}_shape"])
    train_len = np.diff(Z[f"{tag}_train_indptr"])
    ref = Z[f"{tag}_values" if name == "test" else f"{tag}_val_values"]
    pos = Z[f"{tag}_{name}_pos"]
    for r, c in enumerate(Z[f"{tag}_cutoffs"].tolist()):
        values, sums = ranks.finish(pos, tp, tr, thr, train_len, I, c)
        rank_ref.check_values(values, ref[r], f"{tag}/{name}@{c}")
        # the integer slots, counted independently
        rel = tr >= thr
        users = sum(1 for u in range(U) if rel[tp[u]:tp[u + 1]].any())
        assert sums[1] == float((rel & (pos >= 0)).sum()) and sums[4] == float(users) and sums[5] == 0.0
    if thr > 0:
        assert users < int((np.diff(tp) > 0).sum())      # some user with a held-out row has no relevant item


@pytest.mark.parametrize("tag", CASES)
def test_eval_with_ranks_matches_the_reference(tag):
    metrics = ["nDCG", "auc", "GAUC", "lauc"]
    data = rank_ref.golden_case(Z, tag, metrics)
    ev = Evaluator(data, None)
    assert ev.get_needed_recommendations() == data.config.top_k           # full-length lists are never asked for
    recs = {u: [(0, 1.0)] for u in range(data.num_users)}
    has_val = f"{tag}_val_pos" in Z.files
    res = ev.eval((recs, recs), ranks=(_positions(tag, "val") if has_val else None, _positions(tag, "test")))
    for r, c in enumerate(Z[f"{tag}_cutoffs"].tolist()):
        assert list(res[c]["test_results"]) == ["nDCG", "AUC", "GAUC", "LAUC"]
        rank_ref.check_values(res[c]["test_results"], Z[f"{tag}_values"][r], f"{tag}@{c}")
        if has_val:
            rank_ref.check_values(res[c]["val_results"], Z[f"{tag}_val_values"][r], f"{tag}/val@{c}")
        else:
            assert res[c]["val_results"] == res[c]["test_results"]
    a, b = (res[c]["test_results"] for c in Z[f"{tag}_cutoffs"].tolist())
    assert a["AUC"] == b["AUC"] and a["GAUC"] == b["GAUC"] and a["LAUC"] != b["LAUC"]


@pytest.mark.parametrize("name", ["AUC", "gauc", "LAUC"])
def test_without_the_gate_the_constructor_raises_as_before(name):
    data = rank_ref.golden_case(Z, CASES[0], ["nDCG", name], gate=False)
    with pytest.raises(Exception, match="not available in the stand-alone evaluator") as e:
        Evaluator(data, None)
    assert "rank_metrics: True" in str(e.value)


def test_eval_without_ranks_raises():
    data = rank_ref.golden_case(Z, CASES[0], ["nDCG", "AUC"])
    recs = {u: [(0, 1.0)] for u in range(data.num_users)}
    with pytest.raises(Exception, match="need the positions"):
        Evaluator(data, None).eval((recs, recs))


def test_a_user_without_negatives_raises_like_the_reference():
    # 3 items, 2 in train, 2 relevant held out (one without a model row): neg = 3 - 2 - 2 + 1 = 0
    tp, tr = np.array([0, 2]), np.array([1.0, 1.0], np.float32)
    rows = ranks.user_rows(np.array([0, -1], np.int32), tp, tr, 0.0, np.array([2]), 3, 5)
    assert rows[0].tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    with pytest.raises(ZeroDivisionError):
        ranks.finish(np.array([0, -1], np.int32), tp, tr, 0.0, np.array([2]), 3, 5)


def test_positions_edges():
    s = np.array([[0.0, -0.0, 1.0, 1.0, -1.0]], np.float32)
    tg = (np.array([0, 6]), np.array([0, 1, 2, 3, 4, 9], np.int32))
    assert ranks.positions(s, None, tg).tolist() == [2, 3, 0, 1, 4, -1]          # -0.0 ties +0.0, the index breaks ties
    adm = np.array([[True, True, False, True, True]])
    assert ranks.positions(s, adm, tg).tolist() == [1, 2, -1, 0, 3, -1]          # a masked target gets -1 and precedes nothing
