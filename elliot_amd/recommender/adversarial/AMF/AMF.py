"""AMF plugin (YAML key `external.AMF`): Adversarial Matrix Factorization / APR (He et al., https://arxiv.org/abs/1808.03908).

Contract of elliot/recommender/adversarial/AMF/AMF.py:21-198: hyper-parameters `factors`, `lr`, `l_w`, `l_b`, `eps`, `l_adv`,
`eps_iter` (default 2.5 * eps / nb_iter), `nb_iter`, `adversarial_epochs` (default epochs // 2), result-file name "AMF_...".  The
last `adversarial_epochs` epochs run adversarial steps; with `meta.eval_perturbations` every evaluated epoch also builds an MSAP
and then an FGSM perturbation on ONE batch of `transactions` samples, evaluates both, and leaves the FGSM one set for the next
epoch's steps; get_results() then writes `adversarial-{name}.tsv`.  The sampler is BPRMF_batch's.
"""
import os

import pandas as pd
from tqdm import tqdm

from .... import ops
from ....dataset.samplers import custom_sampler
from ...base_recommender_model import BaseRecommenderModel, init_charger, param
from ...recommender_utils_mixin import RecMixin
from .AMF_model import AMF_model


class AMF(RecMixin, BaseRecommenderModel):

    @init_charger
    def __init__(self, data, config, params, *args, **kwargs):
        self._params_list = [
            param("factors", "factors", 200, int),
            param("lr", "lr", 0.001, attr="_learning_rate"),
            param("l_w", "l_w", 0.1),
            param("l_b", "l_b", 0.001),
            param("eps", "eps", 0.1),
            param("l_adv", "l_adv", 0.001),
            param("eps_iter", "eps_iter", None),
            param("nb_iter", "nb_iter", 1),
            param("adversarial_epochs", "adv_epochs", self._epochs // 2, int),
        ]
        self.autoset_params()
        if self._adversarial_epochs > self._epochs:
            raise Exception(f"The total epoch ({self._epochs}) "
                            f"is smaller than the adversarial epochs ({self._adversarial_epochs}).")
        if self._eps_iter is None:
            self._eps_iter = 2.5 * self._eps / self._nb_iter
        if self._batch_size < 1:
            self._batch_size = self._data.transactions
        self._ctx = ops.get_context(max(int(getattr(self._config, "gpu", 0) or 0), 0))
        replay = getattr(self._params, "sampler", "philox") == "replay"
        positives = self._data.i_train_dict if replay else self._data.sp_i_train
        self._sampler = custom_sampler.Sampler(positives, ctx=self._ctx, replay=replay)
        self._results_perturbation = {}
        self._model = AMF_model(self._factors, self._learning_rate, self._l_w, self._l_b, self._eps, self._l_adv, self._num_users,
                                self._num_items, self._seed, ctx=self._ctx, init_weights=kwargs.get("init_weights"))

    @property
    def name(self):
        return "AMF" + f"_{self.get_base_params_shortcut()}" + f"_{self.get_params_shortcut()}"

    def train(self):
        if self._restore:
            return self.restore_weights()
        events = self._data.transactions
        for it in self.iterate(self._epochs):
            user_adv_train = (self._epochs - it) <= self._adversarial_epochs
            fused = (not user_adv_train and self._model.amf.delta_is_zero and getattr(self._sampler, "philox", False)
                     and getattr(self._config, "fused_epoch", True) and not self._verbose)
            loss = 0
            if fused:                                               # plain epochs without a perturbation: BPRMF_batch's loop
                loss = self._model.train_epoch(self._sampler, events, self._batch_size)
            else:
                with tqdm(total=int(events // self._batch_size), disable=not self._verbose) as bar:
                    for batch in self._sampler.step(events, self._batch_size):
                        loss += self._model.train_step(batch, user_adv_train)
                        bar.update()
            self.evaluate(it, float(loss) / (it + 1))
            if getattr(self._params.meta, "eval_perturbations", False):
                self.evaluate_perturbations(it)

    def evaluate_perturbations(self, it=None):
        if (it is None) or (not (it + 1) % self._validation_rate):
            needed = self.evaluator.get_needed_recommendations()
            for full_batch in self._sampler.step(self._data.transactions, self._data.transactions):
                self._model.build_msap_perturbation(full_batch, self._eps_iter, self._nb_iter)
                adversarial_iterative = self._evaluate_lists(needed, adversarial=True)
                self._model.build_perturbation(full_batch)
                adversarial_single = self._evaluate_lists(needed, adversarial=True)
            self._results_perturbation[it] = {"clean": self._results[-1],
                                              "adversarial_single": adversarial_single,
                                              "adversarial_msap": adversarial_iterative}

    def _evaluate_lists(self, k, adversarial):
        return self.evaluator.eval(self.get_recommendations(k, adversarial=adversarial))

    def get_recommendations(self, k: int = 100, adversarial: bool = False):
        self._adversarial_lists = bool(adversarial)
        try:
            return super().get_recommendations(k)
        finally:
            self._adversarial_lists = False

    def get_single_recommendation(self, mask, k, predictions, offset, offset_stop):
        """predict(offset, offset_stop, adversarial) + get_top_k (AMF.py:171-172) in one fused pass."""
        idx, val = self._model.recommend(mask, k, offset, offset_stop, adversarial=getattr(self, "_adversarial_lists", False))
        return self._arrays_to_recs(idx.cpu().numpy(), val.cpu().numpy(), offset, offset_stop)

    def get_results(self):
        if getattr(self._params.meta, "eval_perturbations", False):
            self.store_perturbation_results()
        return self._results[self.get_best_arg()]

    def store_perturbation_results(self):
        metrics = list(getattr(self._data.config.evaluation, "simple_metrics", []))
        first = next(iter(self._results_perturbation.values()), None)
        if first is not None:
            metrics = list(next(iter(first["clean"].values()))["test_results"].keys())
        columns = ["Epoch", "AdvEpoch", "K"] + metrics + ["SSAP-" + m for m in metrics] + ["MSAP-" + m for m in metrics]
        rows = []
        for it, res in self._results_perturbation.items():
            for k in res["clean"].keys():
                rows.append([it, self._adversarial_epochs, k]
                            + list(res["clean"][k]["test_results"].values())
                            + list(res["adversarial_single"][k]["test_results"].values())
                            + list(res["adversarial_msap"][k]["test_results"].values()))
        os.makedirs(self._config.path_output_rec_performance, exist_ok=True)
        pd.DataFrame(rows, columns=columns).to_csv(
            os.path.join(self._config.path_output_rec_performance, f"adversarial-{self.name}.tsv"), index=False, sep="\t")
