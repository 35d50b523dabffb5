"""UserAutoRecModel on the MI355X -- counterpart of elliot/recommender/neural/UserAutoRec/userautorec_model.py:54-123:
rows are users, the layer width is the number of items, the decoder is linear (:43)."""
import torch

from ..autorec_model import AutoRecModel


class UserAutoRecModel(AutoRecModel):
    out_act = None

    def __init__(self, data, num_users, num_items, lr, hidden_neuron, l_w, random_seed=42, name="UserAutoRec", **kwargs):
        super().__init__(data, num_users, num_items, lr, hidden_neuron, l_w, random_seed, name, **kwargs)

    def predict(self, start, stop, **kwargs):
        """:109-119 for users [start, stop): the reconstruction [n, I] on the device."""
        return self.predict_rows(torch.arange(start, stop, dtype=torch.int32, device=self.ctx.device))

    def recommend(self, mask, k, start, stop, item_offset=0):
        return self._topk(self.predict(start, stop), mask, k, start, stop)
