"""train() shared by the iALS and WRMF plugins (iALS.py:91-100, wrmf.py:81-90): one ALS step, then evaluate(it), per iteration."""
from ... import ops


class AlsPluginMixin(object):

    def _als_context(self):
        return ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))

    def train(self):
        if self._restore:
            return self.restore_weights()
        for it in self.iterate(self._epochs):
            self._model.train_step()
            print("Iteration Finished")
            self.evaluate(it)
