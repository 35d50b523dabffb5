"""CPU: BPRSlim's host side -- el_bprslim_levels_host against the restatement, the restatement against the reference's own
arrays (tests/golden/bprslim_ref.npz, written by scripts/gen_golden_bprslim.py from the reference's BPRSlimModel and sampler) bit
for bit, the memory guard's arithmetic, the registration and the checkpoint's key."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import bprslim_ref as br


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def random_triplets(n=2000, U=20, I=30, seed=5):
    rs = np.random.RandomState(seed)
    u = rs.randint(0, U, n).astype(np.int32)
    i = rs.randint(0, I, n).astype(np.int32)
    j = ((i + 1 + rs.randint(0, I - 1, n)) % I).astype(np.int32)              # never i itself
    return u, i, j, U, I


def test_levels_equal_the_restatement_and_ignore_the_user():
    from elliot_amd import ops
    u, i, j, U, I = random_triplets()
    order, start = ops.bprslim_levels(i, j, I)
    lev, ref_order, ref_start = br.levels(i, j, I)
    assert order.dtype == np.int32 and start.dtype == np.int64
    assert len(start) - 1 == len(ref_start) - 1 == lev.max()                 # the level count
    assert np.array_equal(start, ref_start) and np.array_equal(order, ref_order)        # stable: sequence order within a level
    assert np.array_equal(np.sort(order), np.arange(len(i)))
    for a, b in zip(start[:-1], start[1:]):                                  # every level is free of shared rows
        rows = np.concatenate([i[order[a:b]], j[order[a:b]]])
        assert b > a and len(np.unique(rows)) == 2 * (b - a)
    # a triplet stands one level above the last earlier one that shares a row with it
    pos = np.empty(len(i), dtype=np.int64)
    pos[order] = np.searchsorted(start, np.arange(len(i)), side="right")
    assert np.array_equal(pos, lev)
    _, sgd_start = ops.sgd_levels(u, i, j, U, I)
    assert len(start) - 1 < len(sgd_start) - 1                               # the user is no dependency here


def test_levels_edges():
    from elliot_amd import _lib, ops
    order, start = ops.bprslim_levels(np.zeros(0, np.int32), np.zeros(0, np.int32), 4)
    assert len(order) == 0 and start.tolist() == [0]
    order, start = ops.bprslim_levels([0, 2, 0, 1], [1, 3, 2, 3], 4)        # 0|1, 2|3 -> level 1; 0|2 -> 2; 1|3 -> 2
    assert order.tolist() == [0, 1, 2, 3] and start.tolist() == [0, 2, 4]
    with pytest.raises(_lib.ElliotHipError, match="out of range"):
        ops.bprslim_levels([0, 4], [1, 2], 4)
    with pytest.raises(_lib.ElliotHipError, match="out of range"):
        ops.bprslim_levels([0, 1], [1, -1], 4)


@pytest.mark.parametrize("tag", br.CASES)
def test_helper_equals_reference(golden, tag):
    g = golden("bprslim_ref.npz")
    indptr, indices, U, I = br.case(g, tag)
    sp_indptr, sp_indices = br.sorted_rows(indptr, indices)
    h = br.hyper(g, tag)
    S = np.zeros((I, I))
    for e in range(g[f"{tag}_trip"].shape[0]):
        x = br.train(S, sp_indptr, sp_indices, g[f"{tag}_trip"][e], h["lr"], h["li_reg"], h["lj_reg"])
        assert np.array_equal(bits(S), bits(g[f"{tag}_S"][e])), e
        assert np.array_equal(bits(x), bits(g[f"{tag}_x"][e])), e
        assert float(np.cumsum(x * x)[-1]) == float(g[f"{tag}_loss"][e])
    pred = br.predictions(sp_indptr, sp_indices, S)
    if f"{tag}_pred" in g.files:
        assert np.array_equal(bits(pred), bits(g[f"{tag}_pred"]))
    allowed = np.ones((U, I), dtype=bool)
    allowed[np.repeat(np.arange(U), np.diff(indptr)), indices] = False
    for u in range(U):
        _, val = br.topk(pred[u], allowed[u], int(g["k"]))
        assert np.array_equal(bits(val), bits(g[f"{tag}_rec_val"][u])), u
        assert bool(g[f"{tag}_fragile"][u]) == (br.min_gap(pred[u], allowed[u], int(g["k"])) < 1e-9)


def test_golden_cases_hold_what_they_are_for(golden):
    g = golden("bprslim_ref.npz")
    for tag in br.CASES:
        indptr, indices, U, I = br.case(g, tag)
        assert (U, I) == (60, 40) and np.diff(indptr).min() >= 1 and np.diff(indptr).max() < I
        assert any(np.any(np.diff(indices[a:b]) < 0) for a, b in zip(indptr[:-1], indptr[1:]))     # a shuffled dict order
        assert g[f"{tag}_trip"].shape == (2, 3, len(indices)) and g[f"{tag}_fragile"].mean() <= 0.05
        assert not np.diagonal(g[f"{tag}_S"], axis1=1, axis2=2).any()                             # S[i, i] never moves
        assert float(g[f"{tag}_d_reorder"]) < 1e-15
    indptr, indices, U, I = br.case(g, "short_rows")
    single = np.flatnonzero(np.diff(indptr) == 1)
    assert len(single) >= 5 and np.isin(g["short_rows_trip"][0, 0], single).any()
    assert len(np.setdiff1d(np.arange(I), indices)) == 1
    assert g["defaults_hyper"].tolist() == [0.001, 0.001, 0.1] and np.abs(g["defaults_S"]).max() < 0.05


def test_memory_guard_arithmetic():
    from elliot_amd import ops
    assert ops.BPRSLIM_SCORE_BLOCK_BYTES == 1 << 28
    assert ops.bprslim_block_rows(3706, 6040) == 6040 and ops.bprslim_block_rows(200_000, 6040) == 167
    assert ops.bprslim_block_rows(10, 0) == 1 and ops.bprslim_block_rows(1 << 26, 5) == 1
    assert ops.bprslim_memory_need(3706, 6040) == 2 * 8 * 3706 * 3706 + 6040 * 8 * 3706
    assert ops.bprslim_memory_need(200_000, 6040) == 2 * 8 * 200_000 ** 2 + 167 * 8 * 200_000
    for I, U in ((40, 60), (3706, 6040), (200_000, 1_000_000)):
        assert ops.bprslim_block_rows(I, U) * 8 * I <= max(ops.BPRSLIM_SCORE_BLOCK_BYTES, 8 * I)


def test_plugin_is_registered():
    import elliot_amd.external as external
    import elliot_amd.recommender as rec
    from elliot_amd.recommender.latent_factor_models.BPRSlim import BPRSlim
    assert rec.BPRSlim is BPRSlim and "BPRSlim" in rec.__all__
    assert external.BPRSlim is BPRSlim
    assert "external.BPRSlim" in external.__doc__


def test_name_and_shortcuts_are_the_reference_s():
    from elliot_amd.recommender import BPRSlim
    m = object.__new__(BPRSlim)
    m._params_list = [("_lr", "lr", "lr", 0.001, None, None), ("_lj_reg", "lj_reg", "ljreg", 0.001, None, None),
                      ("_li_reg", "li_reg", "lireg", 0.1, None, None)]
    m._seed, m._epochs, m._batch_size, m._lr, m._lj_reg, m._li_reg = 42, 2, 1, 0.001, 0.001, 0.1
    assert m.name == "BPRSlim_seed=42_e=2_bs=1_lr=0$001_ljreg=0$001_lireg=0$1"


def test_checkpoint_key_and_type_are_the_reference_s(golden):
    from elliot_amd.recommender.latent_factor_models.BPRSlim.bprslim_model import BPRSlimModel
    S = golden("bprslim_ref.npz")["plain_S"][-1]
    m = object.__new__(BPRSlimModel)
    m.state = SimpleNamespace(S=torch.from_numpy(S.copy()))
    state = m.get_model_state()
    assert list(state) == ["_s_dense"]
    assert isinstance(state["_s_dense"], np.ndarray) and state["_s_dense"].dtype == np.float64
    assert np.array_equal(bits(state["_s_dense"]), bits(S))
