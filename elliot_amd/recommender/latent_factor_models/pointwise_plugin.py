"""What the four point-wise plugins share beyond RecMixin: context, the device sampler, the default batch size."""
from ... import ops
from ...dataset.samplers import pointwise_pos_neg_sampler


class RatingLabels:
    """A point-wise sampler with the ratings samplers' labels: (u, i, coin) -> (u, i, rating of a positive | 0)  (FM, FISM)."""

    def __init__(self, sampler, ctx, ratings):
        self._sampler, self._ctx = sampler, ctx
        self._ratings = ops.fm_ratings_csr(ctx, ratings)

    def step(self, events, batch_size):
        for u, i, coin in self._sampler.step(events, batch_size):
            yield u, i, ops.fm_labels(self._ctx, self._ratings, u, i, coin)


class PointwisePluginMixin:
    def _pointwise_setup(self, neg_ratio=None):
        """matrix_factorization.py:60-67 (identical in PMF / FunkSVD / LogisticMF): batch_size < 1 = one batch per epoch;
        pointwise_pos_neg_sampler over the training interactions."""
        if self._batch_size < 1:
            self._batch_size = self._data.transactions
        self._ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        # `sampler: replay` = the reference's exact (u, i, label) stream (pointwise_pos_neg_sampler.py:33-46), host-replayed
        replay = getattr(self._params, "sampler", "philox") == "replay"
        self._sampler = pointwise_pos_neg_sampler.Sampler(self._data.i_train_dict if replay else self._data.sp_i_train,
                                                          ctx=self._ctx, replay=replay, neg_ratio=neg_ratio)
