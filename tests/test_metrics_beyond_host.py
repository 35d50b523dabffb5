"""Beyond-accuracy metrics, dict route of the stand-alone Evaluator (NumPy) against the reference's own Evaluator
(tests/golden/metrics_beyond_ref.npz, scripts/gen_golden_metrics_beyond.py)."""
import numpy as np
import pytest

from elliot_amd.evaluation import beyond
from elliot_amd.evaluation.evaluator import Evaluator
from tests.helpers import beyond_ref

# non-negative fp64 sums of <= 25 000 terms in two orders differ by <= 2 n 2^-53 ~ 5.6e-12 relative
TOL = 1e-11
Z = beyond_ref.load()
CASES = [str(t) for t in Z["cases"]]
NAMES = [str(n) for n in Z["names"]]


@pytest.mark.parametrize("tag", CASES)
def test_eval_matches_the_reference(tag):
    data, lists = beyond_ref.golden_case(Z, tag, NAMES)
    ev = Evaluator(data, None)
    recs = beyond_ref.recs_of(lists)
    res = ev.eval((recs, recs))
    for r, c in enumerate(Z[f"{tag}_cutoffs"].tolist()):
        assert list(res[c]["test_results"]) == NAMES
        beyond_ref.check_against(res[c]["test_results"], NAMES, Z[f"{tag}_values"][r], TOL, f"{tag}@{c}")
        assert res[c]["val_results"] == res[c]["test_results"]
        # the Gini numerator in exact integers
        tp = Z[f"{tag}_test_indptr"]
        inA = np.diff(tp) > 0
        L = lists[inA][:, :c]
        hist = np.bincount(L[L >= 0], minlength=data.num_items)
        n, free, G = beyond.gini_numerator(hist, data.num_items)
        assert G == int(Z[f"{tag}_G"][r]) and n == int(Z[f"{tag}_values"][r][0])


@pytest.mark.parametrize("tag", CASES)
def test_short_head_is_the_reference_list(tag):
    data, _ = beyond_ref.golden_case(Z, tag, NAMES)
    tables = Evaluator(data, None).item_tables(data)
    assert tables.short_head.tolist() == Z[f"{tag}_head"].tolist()
    assert tables.n_head == len(Z[f"{tag}_head"]) and int(tables.head.sum()) == tables.n_head


def test_names_are_matched_case_insensitively_with_accuracy_metrics():
    tag = CASES[1]
    mixed = ["nDCG", "itemcoverage", "Precision", "EPC", "gini"]
    data, lists = beyond_ref.golden_case(Z, tag, mixed)
    recs = beyond_ref.recs_of(lists)
    res = Evaluator(data, None).eval((recs, recs))
    c = int(Z[f"{tag}_cutoffs"][0])
    got = res[c]["test_results"]
    assert list(got) == ["nDCG", "ItemCoverage", "Precision", "EPC", "Gini"]
    ref = dict(zip(NAMES, Z[f"{tag}_values"][0]))
    assert got["ItemCoverage"] == int(ref["ItemCoverage"])
    assert abs(got["EPC"] - ref["EPC"]) <= TOL and abs(got["Gini"] - ref["Gini"]) <= TOL
    assert 0.0 < got["nDCG"] <= 1.0


@pytest.mark.parametrize("name", ["MAR", "nDCGRendle2020", "AUC", "MAE"])
def test_unsupported_names_still_raise(name):
    data, _ = beyond_ref.golden_case(Z, CASES[0], ["nDCG", name])
    with pytest.raises(Exception, match="not available in the stand-alone evaluator"):
        Evaluator(data, None)
