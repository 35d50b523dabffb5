"""CPU: SlopeOne's host side -- the restatement the GPU tests compare with equals the reference's own arrays
(tests/golden/slopeone_ref.npz, written by scripts/gen_golden_slopeone.py from the reference's SlopeOneModel) bit for bit; the
plug-in is registered; the checkpoint has the reference's keys and types; other ratings than integers and half steps are
refused."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import slopeone_ref

CASES = ["int", "half", "cold_item", "one_rating", "split"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("tag", CASES)
def test_helper_equals_reference(golden, tag):
    g = golden("slopeone_ref.npz")
    indptr, indices, ratings, U, I = slopeone_ref.case(g, tag)
    freq, dev, mean = slopeone_ref.build(indptr, indices, ratings, U, I)
    assert np.array_equal(freq, g[f"{tag}_freq"])
    assert np.array_equal(bits(dev), bits(g[f"{tag}_dev"]))                 # the -0.0 pattern included
    assert np.array_equal(bits(mean), bits(g[f"{tag}_user_mean"]))
    pred = slopeone_ref.predictions(indptr, indices, freq, dev, mean)
    if f"{tag}_pred" in g.files:
        assert np.array_equal(bits(pred), bits(g[f"{tag}_pred"]))
    k = int(g["k"])
    allowed = np.ones((U, I), dtype=bool)
    allowed[np.repeat(np.arange(U), np.diff(indptr)), indices] = False
    for u in range(U):
        _, val = slopeone_ref.topk(pred[u], allowed[u], k)
        assert np.array_equal(bits(val), bits(g[f"{tag}_rec_val"][u])), u


def test_golden_cases_hold_what_they_are_for(golden):
    g = golden("slopeone_ref.npz")
    assert np.any(g["half_ratings"] * 2 % 2 == 1)
    assert not g["cold_item_freq"][7].any()
    assert np.diff(g["one_rating_indptr"]).min() == 1
    freq, dev = g["split_freq"], g["split_dev"]
    empty = np.tril(freq == 0, -1)
    assert empty.any() and np.signbit(dev[empty]).all() and not np.signbit(dev[empty.T]).any()
    for tag in CASES:                                                       # rows are stored in a shuffled order
        indptr, indices = g[f"{tag}_indptr"], g[f"{tag}_indices"]
        assert any(np.any(np.diff(indices[a:b]) < 0) for a, b in zip(indptr[:-1], indptr[1:]))


@pytest.mark.parametrize("tag", ["int", "half", "one_rating"])
def test_host_user_mean_equals_reference(golden, tag):
    from elliot_amd import ops
    g = golden("slopeone_ref.npz")
    mean = ops.slope_user_mean(g[f"{tag}_indptr"], g[f"{tag}_ratings"])
    assert mean.dtype == np.float64 and np.array_equal(bits(mean), bits(g[f"{tag}_user_mean"]))


def test_user_mean_of_an_empty_row_is_nan():
    from elliot_amd import ops
    mean = ops.slope_user_mean(np.array([0, 2, 2, 3]), np.array([1.0, 4.0, 2.5]))
    assert mean[0] == 2.5 and np.isnan(mean[1]) and mean[2] == 2.5


def test_plugin_is_registered():
    import elliot_amd.external as external
    import elliot_amd.recommender as rec
    from elliot_amd.recommender.algebric.slope_one import SlopeOne
    assert rec.SlopeOne is SlopeOne and "SlopeOne" in rec.__all__
    assert external.SlopeOne is SlopeOne
    assert SlopeOne.name.fget(None) == "SlopeOne"


def test_checkpoint_keys_and_types_are_the_reference_s(golden):
    from elliot_amd.recommender.algebric.slope_one.slope_one_model import SlopeOneModel
    g = golden("slopeone_ref.npz")
    m = object.__new__(SlopeOneModel)
    m.state = SimpleNamespace(freq=torch.from_numpy(g["split_freq"].astype(np.int32)), dev=torch.from_numpy(g["split_dev"]),
                              user_mean_host=g["split_user_mean"])
    state = m.get_model_state()
    assert list(state) == ["freq", "dev", "user_mean"]
    assert isinstance(state["freq"], np.ndarray) and state["freq"].dtype == np.float64
    assert isinstance(state["dev"], np.ndarray) and state["dev"].dtype == np.float64
    assert isinstance(state["user_mean"], list) and all(type(x) is np.float64 for x in state["user_mean"])
    assert np.array_equal(state["freq"], g["split_freq"])
    assert np.array_equal(bits(state["dev"]), bits(g["split_dev"]))
    assert np.array_equal(bits(state["user_mean"]), bits(g["split_user_mean"]))


def test_non_half_step_ratings_refused():
    from elliot_amd import ops
    assert ops.slope_integer_ratings(np.array([1.0, 5.0]))[0] == 1
    assert ops.slope_integer_ratings(np.array([1.5, 5.0]))[0] == 2
    with pytest.raises(ValueError, match="SlopeOne needs integer or half-step"):
        ops.slope_integer_ratings(np.array([1.0, 2.3]))
    with pytest.raises(ValueError, match="SlopeOne"):
        ops.slope_integer_ratings(np.array([1.25]))
