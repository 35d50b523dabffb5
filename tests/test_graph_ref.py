"""CPU: the restatements of tests/helpers/graph_ref.py (what tests/test_gpu_graph_edges.py holds the graph kernels to) against SciPy and
against the oracles of the graph models, and the one bound those tests take over from the existing random SpMM test."""
import numpy as np
import scipy.sparse as sp

from oracle import lightgcn as ol
from oracle import ngcf as on
from tests.helpers import graph_ref as gr

f32 = np.float32


def test_edge_csr_has_every_length_on_both_sides_and_sorted_distinct_columns():
    N = 9000
    indptr, indices, where = gr.edge_csr(N, seed=0)
    lens = np.diff(indptr)
    for n in gr.ROW_LENGTHS:
        rows = np.asarray(where[n])
        assert (rows < N // 2).any() and (rows >= N // 2).any(), n
    assert lens[0] > 512 and lens[N - 1] > 512 and lens[1] == 0 and lens[N - 2] == 0
    assert lens[N // 2 - 1] > 512 and lens[N // 2] > 512
    inside = np.ones(len(indices), bool)
    inside[indptr[1:-1][lens[1:] > 0]] = False                     # (the first entry of a row has no predecessor in it)
    inside[0] = False
    assert (np.diff(indices.astype(np.int64))[inside[1:]] > 0).all() and indices.min() >= 0 and indices.max() < N
    partials = set(((lens + 511) // 512)[lens > 512].tolist())
    assert {2, 3, 8, 9, 10, 16, 17} <= partials


def test_exact_values_make_the_fp32_product_exact_in_any_order():
    indptr, indices, _ = gr.edge_csr(9000, seed=0)
    rs = np.random.RandomState(1)
    vals, X = gr.exact_vals(len(indices), rs), gr.exact_table(9000, 12, rs)
    ref = gr.spmm_f64(indptr, indices, vals, X)
    L = sp.csr_matrix((vals.astype(np.float64), indices, indptr), shape=(9000, 9000))
    assert np.array_equal(ref, L.toarray() @ X.astype(np.float64))                                # the helper against a dense product
    assert np.abs(gr.spmm_magnitude(indptr, indices, vals, X)).max() < 2 ** 18                    # every partial sum, in any order
    assert np.array_equal(gr.spmm_chunk_order_f32(indptr, indices, vals, X).astype(np.float64), ref)


def test_fp32_sum_in_chunk_order_keeps_the_random_tests_bound():
    """4e-7 * mag + 1e-12 (tests/test_gpu_graph.py) holds for a fp32 sum taken term by term inside each 512-chunk and chunk by chunk
    after it, on the edge structure with normal values at F = 100 -- what the GPU test relies on before it applies the bound."""
    indptr, indices, _ = gr.edge_csr(9000, seed=0)
    rs = np.random.RandomState(11)
    vals = rs.normal(size=len(indices)).astype(f32)
    X = rs.normal(size=(9000, 100)).astype(f32)
    got = gr.spmm_chunk_order_f32(indptr, indices, vals, X)
    ref, mag = gr.spmm_f64(indptr, indices, vals, X), gr.spmm_magnitude(indptr, indices, vals, X)
    ratio = (np.abs(got - ref) / (4e-7 * mag + 1e-12)).max()
    assert ratio <= 1.0, ratio


def _small():
    rs = np.random.RandomState(0)
    U, I, k = 30, 20, 8
    R = sp.random(U, I, density=0.2, format="csr", random_state=rs, dtype=f32)
    R.data[:] = 1.0
    _, lap = ol.create_adj_mat(R, U, I)
    return rs, U, I, k, lap


def test_lightgcn_restatement_equals_the_oracle():
    rs, U, I, k, lap = _small()
    Gu, Gi = rs.normal(size=(U, k)).astype(f32), rs.normal(size=(I, k)).astype(f32)
    for n_layers in (0, 1, 3, 16):
        ref = gr.lightgcn_propagate_f64(Gu, Gi, lap, n_layers)
        orc = ol.propagate(Gu, Gi, lap, n_layers)
        assert np.abs(ref[0] - orc[0]).max() < 1e-6 and np.abs(ref[1] - orc[1]).max() < 1e-6, n_layers


def test_ngcf_restatement_equals_the_oracle():
    rs, U, I, k, lap = _small()
    sizes = (k, 12, 8)
    Gu, Gi = rs.normal(size=(U, sum(sizes))).astype(f32), rs.normal(size=(I, sum(sizes))).astype(f32)
    layers = [{"W1": rs.normal(scale=0.3, size=(a, b)).astype(f32), "b1": rs.normal(scale=0.1, size=(1, b)).astype(f32),
               "W2": rs.normal(scale=0.3, size=(a, b)).astype(f32), "b2": rs.normal(scale=0.1, size=(1, b)).astype(f32)}
              for a, b in zip(sizes[:-1], sizes[1:])]
    ref = gr.ngcf_propagate_f64(Gu, Gi, lap, layers, k)
    orc = on.propagate(Gu, Gi, lap, layers, k)
    assert np.abs(ref[0] - orc[0]).max() < 1e-5 and np.abs(ref[1] - orc[1]).max() < 1e-5
    # the pieces: one rounding each in fp32, the normalisation's two branches
    e, l = Gu[:, :k], Gu[:, k:2 * k]
    assert np.array_equal(gr.ngcf_pre(e, l), np.concatenate([l + e, e * l], 1))
    x = np.asarray([[3.0, -4.0], [0.0, 0.0], [3e-8, 4e-8]])
    assert np.allclose(gr.l2_normalize_f64(x), [[0.6, -0.8], [0.0, 0.0], [3e-2, 4e-2]], rtol=1e-15, atol=0)
    assert np.array_equal(gr.leaky_relu(np.asarray([-1.0, 0.0, 2.0], f32)), np.asarray([f32(-1.0) * f32(0.2), 0.0, 2.0], f32))


def test_adam_restatement_equals_the_oracles_layer_update_bit_for_bit():
    """graph_ref.adam_l2_dense (fp32) is NGCFOracle.train_step's GraphLayers update: three steps, every parameter, the same bits."""
    rs, U, I, k, lap = _small()
    Gu, Gi = rs.normal(scale=0.2, size=(U, k + 4)).astype(f32), rs.normal(scale=0.2, size=(I, k + 4)).astype(f32)
    layers = [{"W1": rs.normal(scale=0.3, size=(k, 4)).astype(f32), "b1": rs.normal(scale=0.1, size=(1, 4)).astype(f32),
               "W2": rs.normal(scale=0.3, size=(k, 4)).astype(f32), "b2": np.zeros((1, 4), f32)}]
    lr, l_w = 0.005, 0.02
    o = on.NGCFOracle(Gu, Gi, lap, layers, k, lr, l_w)
    mine = {name: (p.copy(), np.zeros_like(p), np.zeros_like(p)) for name, p in layers[0].items()}
    for t in range(1, 4):
        o.train_step((rs.randint(0, U, 64), rs.randint(0, I, 64), rs.randint(0, I, 64)))
        for name, (th, m, v) in mine.items():
            mine[name] = gr.adam_l2_dense(th, m, v, float(on.ob.adam_lr_t(lr, t)), 2.0 * l_w)[:3]
            assert mine[name][0].dtype == f32
            assert np.array_equal(mine[name][0].view(np.uint32), o.layers[0][name].view(np.uint32)), (t, name)
    assert not mine["b2"][0].any()                                 # theta = 0 stays 0: 0 / (0 + epsilon)


def test_dropout_mask_restatement_is_a_fair_counter_based_draw():
    keep = gr.dropout_keep(64, 64, 0.3, 42, 3)
    assert abs((~keep).mean() - 0.3) < 6 * np.sqrt(0.21 / 4096)
    assert np.array_equal(keep, gr.dropout_keep(64, 64, 0.3, 42, 3))
    assert not np.array_equal(keep, gr.dropout_keep(64, 64, 0.3, 42, 4)) and not np.array_equal(keep, gr.dropout_keep(64, 64, 0.3, 43, 3))
