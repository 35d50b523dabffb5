"""The protocol the device model classes share (recommender/device_model.py), the host draws of the initial weights and
ops._own -- all on the CPU: no library call, no GPU."""
import types

import numpy as np
import torch

from elliot_amd import ops
from elliot_amd.recommender.device_model import DeviceModel, glorot_uniform
from elliot_amd.recommender.latent_factor_models import pointwise_model
from elliot_amd.recommender.latent_factor_models.BPRMF_batch import BPRMF_batch_model
from elliot_amd.recommender.visual_recommenders.VBPR import VBPR_model

U, I, F, FD, D, SEED = 7, 5, 4, 3, 6, 42


class ToyModel(DeviceModel):
    def __init__(self):
        self.ctx = types.SimpleNamespace(device=torch.device("cpu"))
        self.state = {"w": np.arange(6, dtype=np.float32).reshape(2, 3), "step": 3}
        self.set_calls = 0

    def get_model_state(self):
        return dict(self.state)

    def set_model_state(self, d):
        self.set_calls += 1
        self.state = dict(d)


def test_checkpoint_round_trip(tmp_path):
    a, b = ToyModel(), ToyModel()
    b.state = {"w": np.zeros((2, 3), np.float32), "step": 0}
    path = str(tmp_path / "weights.pkl")
    a.save_weights(path)
    b.load_weights(path)
    assert b.set_calls == 1 and a.set_calls == 0
    assert sorted(b.state) == ["step", "w"] and b.state["step"] == 3
    assert np.array_equal(b.state["w"], a.state["w"]) and b.state["w"].dtype == np.float32


def test_as_index():
    m = ToyModel()
    want = torch.tensor([3, 0, 6, 2], dtype=torch.int32)
    for x in (np.array([[3], [0], [6], [2]], dtype=np.int64), [3, 0, 6, 2], torch.tensor([[3, 0], [6, 2]], dtype=torch.int32),
              torch.tensor([3, 9, 0, 9, 6, 9, 2, 9], dtype=torch.int64)[::2]):
        t = m._as_index(x)
        assert t.dtype == torch.int32 and tuple(t.shape) == (4,) and t.is_contiguous() and t.device == m.ctx.device
        assert torch.equal(t, want)


def test_version_protocol():
    m = ToyModel()
    assert m._items_unchanged() is False          # a fresh model: nothing was scored yet
    assert m._items_unchanged() is True
    assert m._items_unchanged() is True
    m._touch()
    assert m._items_unchanged() is False          # changed, once
    assert m._items_unchanged() is True
    m._touch()
    m._touch()
    assert m._items_unchanged() is False
    assert m._items_unchanged() is True
    other = ToyModel()                            # the counters are per instance
    assert other._items_unchanged() is False


def _draw(rs, rows, cols):
    lim = np.sqrt(6.0 / (rows + cols))
    return rs.uniform(-lim, lim, size=(rows, cols)).astype(np.float32)


def test_glorot_uniform():
    got = glorot_uniform(np.random.RandomState(SEED), U, F)
    assert got.dtype == np.float32 and got.shape == (U, F)
    assert np.array_equal(got, _draw(np.random.RandomState(SEED), U, F))
    assert np.abs(got).max() <= np.float32(np.sqrt(6.0 / (U + F)))


def test_bprmf_batch_initial_weights():
    """BPRMF_batch and AMF: Gu, then Gi; Bi = 0."""
    Gu, Gi, Bi = BPRMF_batch_model.initial_weights(SEED, U, I, F)
    rs = np.random.RandomState(SEED)
    assert np.array_equal(Gu, _draw(rs, U, F)) and np.array_equal(Gi, _draw(rs, I, F))
    assert np.array_equal(Bi, np.zeros(I, np.float32)) and Bi.dtype == np.float32 and Bi.shape == (I,)
    assert Gu.dtype == Gi.dtype == np.float32


def test_vbpr_initial_weights():
    """Bi = 0, then Gu, Gi, Bp ([D, 1]), Tu, E."""
    w = VBPR_model.initial_weights(SEED, U, I, F, FD, D)
    rs = np.random.RandomState(SEED)
    want = {"Bi": np.zeros(I, np.float32)}
    want["Gu"], want["Gi"] = _draw(rs, U, F), _draw(rs, I, F)
    want["Bp"] = _draw(rs, D, 1)
    want["Tu"], want["E"] = _draw(rs, U, FD), _draw(rs, D, FD)
    assert sorted(w) == sorted(VBPR_model.NAMES) == sorted(want)
    for n in want:
        assert w[n].dtype == np.float32 and w[n].shape == want[n].shape and np.array_equal(w[n], want[n]), n


def test_pointwise_initial_weights():
    """Gu, Gi; with biases Bu and Bi follow, each drawn as a [rows, 1] kernel (its limit is sqrt(6 / (rows + 1)))."""
    w = pointwise_model.initial_weights(np.random.RandomState(SEED), U, I, F, with_biases=False)
    rs = np.random.RandomState(SEED)
    assert sorted(w) == ["Gi", "Gu"]
    assert np.array_equal(w["Gu"], _draw(rs, U, F)) and np.array_equal(w["Gi"], _draw(rs, I, F))

    w = pointwise_model.initial_weights(np.random.RandomState(SEED), U, I, F, with_biases=True)
    rs = np.random.RandomState(SEED)
    want = {"Gu": _draw(rs, U, F), "Gi": _draw(rs, I, F), "Bu": _draw(rs, U, 1)[:, 0], "Bi": _draw(rs, I, 1)[:, 0]}
    assert sorted(w) == sorted(want)
    for n in want:
        assert w[n].dtype == np.float32 and w[n].shape == want[n].shape and np.array_equal(w[n], want[n]), n
    assert w["Bu"].flags.c_contiguous and w["Bi"].flags.c_contiguous


def test_own():
    cpu = torch.device("cpu")
    a = np.arange(12, dtype=np.float64).reshape(3, 4) / 3
    strided = torch.arange(24, dtype=torch.float32).reshape(4, 6)[:, ::2]
    plain = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    assert not strided.is_contiguous() and plain.is_contiguous()
    for x, dt in ((a, torch.float32), (a, torch.float64), (strided, torch.float32), (plain, torch.float32), (plain, torch.float64)):
        src = torch.from_numpy(x) if isinstance(x, np.ndarray) else x
        before = src.clone()
        t = ops._own(x, cpu, dt)
        assert t.dtype == dt and t.is_contiguous() and t.device == cpu and tuple(t.shape) == tuple(src.shape)
        assert torch.equal(t, before.to(dt))
        assert t.untyped_storage().data_ptr() != src.untyped_storage().data_ptr()
        t.add_(1)                                 # the state's copy moves, the caller's does not
        assert torch.equal(src, before)
    assert ops._own(a, cpu).dtype == torch.float32
    assert ops._own(None, cpu) is None
