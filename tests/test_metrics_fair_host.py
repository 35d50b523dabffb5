"""Fairness metrics (evaluation.complex_metrics), dict route of the stand-alone Evaluator (NumPy) against the reference's own
Evaluator (tests/golden/metrics_fair_ref.npz, scripts/gen_golden_metrics_fair.py)."""
import os

import numpy as np
import pytest

from elliot_amd import run
from elliot_amd.evaluation import fairness
from elliot_amd.evaluation.evaluator import Evaluator
from tests.helpers import fair_ref

# the bound of the beyond-accuracy goldens: fp64 sums of <= 25 000 terms in two orders differ by <= 2 n 2^-53 ~ 5.6e-12 relative
TOL = 1e-11
Z = fair_ref.load()
CASES = [str(t) for t in Z["cases"]]


def host_tables(ev, data, lists, scores, cutoff):
    """numpy_terms of the pass that serves RSP, REO and BiasDisparity for the test split, and BiasDisparityBS's counts"""
    n_pass = {s.n_pass for s in ev._fair.specs if s.metric in ("RSP", "REO") + fairness.PAIR}
    assert len(n_pass) == 1
    ig, ug = ev._fair.passes[n_pass.pop()]
    train = ev._host_train_csr()
    users = np.arange(data.num_users, dtype=np.int64)
    terms = fairness.numpy_terms(lists, scores, users, data.split_csr(False), float(data.config.evaluation.relevance_threshold), train, ig,
                                 ug, cutoff, data.num_items)
    return terms, fairness.bs_counts(train, ig, ug)


@pytest.mark.parametrize("tag", CASES)
def test_eval_matches_the_reference(tag, tmp_path):
    data, lists, scores = fair_ref.golden_case(Z, tag, tmp_path)
    ev = Evaluator(data, None)
    recs = fair_ref.recs_of(lists, scores)
    res = ev.eval((recs, recs))
    names = [str(n) for n in Z[f"{tag}_names"]]
    for r, c in enumerate(Z[f"{tag}_cutoffs"].tolist()):
        fair_ref.check_values(res[c]["test_results"], names, Z[f"{tag}_values"][r], TOL, f"{tag}@{c}")
        assert list(res[c]["val_results"]) == names
        terms, bs = host_tables(ev, data, lists, scores, c)
        assert terms["item_counts"].tolist() == Z[f"{tag}_item_counts"][r].tolist()
        assert terms["pair"].tolist() == Z[f"{tag}_br"][r].tolist()
        assert bs.tolist() == Z[f"{tag}_bs"].tolist()


def test_the_first_case_has_49_entries_per_cutoff(tmp_path):
    data, lists, scores = fair_ref.golden_case(Z, CASES[0], tmp_path)
    recs = fair_ref.recs_of(lists, scores)
    res = Evaluator(data, None).eval((recs, recs))
    for c in Z[f"{CASES[0]}_cutoffs"].tolist():
        got = res[c]["test_results"]
        assert len(got) == 49 and list(got)[0] == "nDCG"
        assert list(got)[1] == "RSP-ProbToBeRanked_items:IG-0" and list(got)[-1] == "ItemMADrating_IG"


def test_metric_names_are_matched_case_insensitively(tmp_path):
    data, lists, scores = fair_ref.golden_case(Z, CASES[1], tmp_path)
    cm = data.config.evaluation.complex_metrics
    data.config.evaluation.complex_metrics = [dict(d, metric=d["metric"].lower()) for d in cm if d["metric"] in ("RSP", "ItemMADrating")]
    recs = fair_ref.recs_of(lists, scores)
    c = int(Z[f"{CASES[1]}_cutoffs"][0])
    got = Evaluator(data, None).eval((recs, recs))[c]["test_results"]
    ref = dict(zip([str(n) for n in Z[f"{CASES[1]}_names"]], Z[f"{CASES[1]}_values"][0]))
    assert list(got) == ["nDCG", "RSP-ProbToBeRanked_items:IG-0", "RSP-ProbToBeRanked_items:IG-1", "RSP_items:IG", "ItemMADrating_IG"]
    for m, v in got.items():
        assert abs(v - ref[m]) <= TOL * max(1.0, abs(ref[m])), (m, v, ref[m])


def test_without_complex_metrics_nothing_changes(tmp_path):
    data, lists, scores = fair_ref.golden_case(Z, CASES[1], tmp_path)
    data.config.evaluation.complex_metrics = []
    ev = Evaluator(data, None)
    assert ev._fair is None and not ev.needs_scores
    recs = fair_ref.recs_of(lists, scores)
    c = int(Z[f"{CASES[1]}_cutoffs"][0])
    assert list(ev.eval((recs, recs))[c]["test_results"]) == ["nDCG"]


def test_a_label_file_with_a_gap_raises(tmp_path):
    data, _, _ = fair_ref.golden_case(Z, CASES[1], tmp_path)
    bad = fair_ref.write_tsv(tmp_path / "gap.tsv", [0, 1, 2, 3], [0, 2, 2, 0])
    data.config.evaluation.complex_metrics = [{"metric": "RSP", "clustering_name": "G", "clustering_file": bad}]
    with pytest.raises(Exception, match="gap.tsv"):
        Evaluator(data, None)


def test_more_than_64_groups_raises_and_says_so(tmp_path):
    data, _, _ = fair_ref.golden_case(Z, CASES[0], tmp_path)
    many = fair_ref.write_tsv(tmp_path / "many.tsv", list(range(65)), list(range(65)))
    data.config.evaluation.complex_metrics = [{"metric": "REO", "clustering_name": "G", "clustering_file": many}]
    with pytest.raises(Exception, match="at most 64"):
        Evaluator(data, None)


@pytest.mark.parametrize("name", ["ExtendedPopREO", "BiasDisparity", "MAD"])
def test_an_unknown_complex_metric_raises(name, tmp_path):
    data, _, _ = fair_ref.golden_case(Z, CASES[1], tmp_path)
    data.config.evaluation.complex_metrics = [{"metric": name}]
    with pytest.raises(Exception, match="not available in the stand-alone evaluator"):
        Evaluator(data, None)


def test_build_config_resolves_the_clustering_files(tmp_path):
    exp = {"dataset": "toy", "top_k": 5,
           "path_output_rec_result": str(tmp_path / "r"), "path_output_rec_weight": str(tmp_path / "w"),
           "path_output_rec_performance": str(tmp_path / "p"),
           "evaluation": {"simple_metrics": ["nDCG"], "complex_metrics": [
               {"metric": "RSP", "clustering_name": "Pop", "clustering_file": "../data/{0}/i_pop.tsv"},
               {"metric": "BiasDisparityBD", "user_clustering_name": "U", "user_clustering_file": "groups/{0}_users.tsv",
                "item_clustering_name": "Pop", "item_clustering_file": str(tmp_path / "abs" / "items.tsv")}]}}
    base = str(tmp_path / "cfg")
    cm = run.build_config(exp, base).evaluation.complex_metrics
    assert cm[0] == {"metric": "RSP", "clustering_name": "Pop", "clustering_file": os.path.abspath(os.path.join(base, "..", "data", "toy", "i_pop.tsv"))}
    assert cm[1]["user_clustering_file"] == os.path.join(base, "groups", "toy_users.tsv")
    assert cm[1]["item_clustering_file"] == str(tmp_path / "abs" / "items.tsv")
    assert cm[1]["metric"] == "BiasDisparityBD" and cm[1]["user_clustering_name"] == "U" and cm[1]["item_clustering_name"] == "Pop"
    assert exp["evaluation"]["complex_metrics"][0]["clustering_file"] == "../data/{0}/i_pop.tsv"      # the input is left alone
