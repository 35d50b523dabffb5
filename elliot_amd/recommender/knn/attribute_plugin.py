"""Plugin half shared by AttributeItemKNN and AttributeUserKNN (attribute_item_knn.py / attribute_user_knn.py: __init__, train)."""
from .. import attribute_profiles as ap
from ... import ops


class AttributeKnnPluginMixin(object):
    """The subclass sets `_params_list`, names its Similarity class and gives attribute_matrix()."""
    _similarity_class = None

    def _init_attribute_knn(self):
        self.autoset_params()
        self._side = ap.side_of(self._data, self._loader, type(self).__name__)
        self._ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        self._model = self._similarity_class(data=self._data, attribute_matrix=self.attribute_matrix,
                                             num_neighbors=self._num_neighbors, similarity=self._similarity,
                                             implicit=self._implicit, ctx=self._ctx)

    def train(self):
        if self._restore:
            return self.restore_weights()
        self._model.initialize()                      # no epochs: one evaluation of the built model
        self.evaluate()
