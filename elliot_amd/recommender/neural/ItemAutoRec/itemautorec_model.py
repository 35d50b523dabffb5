"""ItemAutoRecModel on the MI355X -- counterpart of elliot/recommender/neural/ItemAutoRec/itemautorec_model.py:51-131:
rows are items, the layer width is the number of users, the decoder ends in a sigmoid (:40).

The reference predicts every item row, [I, U], and transposes on the host (itemautorec.py:102-104).  Here the items are encoded
once per evaluation and a block of users is scored as sigmoid(W2T[u] . h[i] + b2[u]): that block IS the transpose."""
import torch

from ..autorec_model import AutoRecModel


class ItemAutoRecModel(AutoRecModel):
    out_act = "sigmoid"

    def __init__(self, data, num_users, num_items, lr, hidden_neuron, l_w, random_seed=42, name="ItemAutoRec", **kwargs):
        super().__init__(data, num_users, num_items, lr, hidden_neuron, l_w, random_seed, name, **kwargs)
        self._order, self._h_all = None, None

    def set_eval_order(self, order=None):
        """The item whose prediction fills column c of the next blocks: None = item c, else order[c] (the reference's get_recs on a
        freshly shuffled batch).  Starts a new evaluation: the items are encoded again."""
        self._order = None if order is None else torch.as_tensor(order, dtype=torch.int32).to(self.ctx.device).contiguous()
        self._h_all = None

    def get_recs_block(self, start, stop):
        """Rows [start, stop) of transpose(get_recs(all items)) (:123-131, itemautorec.py:104): [n users, I] on the device."""
        key = self.state.step
        if self._h_all is None or self._h_all[0] != key:
            rows = self._order if self._order is not None else torch.arange(self.num_items, dtype=torch.int32, device=self.ctx.device)
            self._h_all = (key, self.state.encode(self.train_csr, rows))
        return self.state.predict_columns(self._h_all[1], start, stop)

    def recommend(self, mask, k, start, stop, item_offset=0):
        return self._topk(self.get_recs_block(start, stop), mask, k, start, stop)
