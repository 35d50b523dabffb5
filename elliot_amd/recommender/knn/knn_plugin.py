"""Plugin half shared by ItemKNN and UserKNN (item_knn.py / user_knn.py: __init__, name, train)."""
from ... import ops

# the reference's _params_list, verbatim (item_knn.py:48-59): `name` and every output file name depend on it
KNN_PARAMS = [
    ("_num_neighbors", "neighbors", "nn", 40, int, None),
    ("_similarity", "similarity", "sim", "cosine", None, None),
    ("_implementation", "implementation", "imp", "standard", None, None),
    ("_implicit", "implicit", "bin", False, None, None),
    ("_shrink", "shrink", "shrink", 0, None, None),
    ("_normalize", "normalize", "norm", True, None, None),
    ("_asymmetric_alpha", "asymmetric_alpha", "asymalpha", False, None, lambda x: x if x else ""),
    ("_tversky_alpha", "tversky_alpha", "tvalpha", False, None, lambda x: x if x else ""),
    ("_tversky_beta", "tversky_beta", "tvbeta", False, None, lambda x: x if x else ""),
    ("_row_weights", "row_weights", "rweights", None, None, lambda x: x if x else ""),
]


class KnnPluginMixin(object):
    """__init__ body and train() of both plugins; the subclass names its Similarity class."""
    _similarity_class = None

    def _init_knn(self):
        self._params_list = list(KNN_PARAMS)
        self.autoset_params()
        self._ratings = self._data.train_dict
        if self._implementation == "aiolli":
            raise NotImplementedError(f"{type(self).__name__}: implementation 'aiolli' (shrink, asymmetric / Tversky "
                                      "similarities, row weights) is not implemented by elliot_amd; use implementation: standard")
        if (not self._normalize) or self._asymmetric_alpha or self._tversky_alpha or self._tversky_beta or self._row_weights \
                or self._shrink:
            self.logger.info("Options normalize, asymmetric_alpha, tversky_alpha, tversky_beta, row_weights are ignored with "
                             "standard implementation. Try with implementation: aiolli")
        self._ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        self._model = self._similarity_class(data=self._data, num_neighbors=self._num_neighbors,
                                             similarity=self._similarity, implicit=self._implicit, ctx=self._ctx)

    def train(self):
        if self._restore:
            return self.restore_weights()
        self._model.initialize()                      # no epochs: one evaluation of the built model
        self.evaluate()
