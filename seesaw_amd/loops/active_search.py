"""ActiveSearch / LKNNSearch loops (seesaw/loops/active_search.py:32-223): the next image is chosen by planning over
the L-KNN model instead of by the current query vector.  ActiveSearch plans with efficient non-myopic search (the
vectorised two-step look-ahead runs on the GPU); LKNNSearch greedily takes the most probable remaining node.
interactive_options["model_on_device"] = True keeps the model's state on the device (DeviceLKNNModel): set_text_vec
uploads gamma once, next_batch is one step call, refine one condition call; absent or false, the host LKNNModel runs."""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

from ..calibration import FixedCalibrator
from ..research.active_search.common import Dataset
from ..research.active_search.efficient_nonmyopic_search import efficient_nonmyopic_search, efficient_nonmyopic_search_batch
from .graph_based import get_label_prop
from .LKNN_model import DeviceLKNNModel, LKNNModel, initial_gamma_array
from .loop_base import LoopBase


def _model_class(opts, planner: bool):
    """interactive_options["model_on_device"]: the model whose state stays on the device (DeviceLKNNModel).  What it
    cannot serve is refused here, at construction, not met half way through a session."""
    if not opts.get("model_on_device", False):
        return LKNNModel
    if planner:
        if opts["implementation"] != "vectorized":
            raise ValueError(f"model_on_device serves implementation='vectorized' only, not {opts['implementation']!r}")
        if opts["pruning_on"]:
            raise ValueError("model_on_device does not serve pruning_on=True")
        if opts["reward_horizon"] > DeviceLKNNModel.KERNEL_MAX_K + 1:
            raise ValueError(f"model_on_device serves a reward_horizon of at most {DeviceLKNNModel.KERNEL_MAX_K + 1}, "
                             f"not {opts['reward_horizon']}")
    return DeviceLKNNModel


def _condition_all(model, answers):
    """the answers [(node, y), ...] in order: one enqueued call on the device model, one condition_ each on the host model"""
    if isinstance(model, DeviceLKNNModel):
        model.condition_many_(answers)
    else:
        for idx, y in answers:
            model.condition_(idx, y)


def _vector_position(index, dbidx) -> int:
    """first vector of image `dbidx` (`vector_meta.query(f'dbidx == {idx}').index[0]`)"""
    return int(np.searchsorted(index.vector_meta.dbidx.values, dbidx, side="left"))


class ActiveSearch(LoopBase):
    def __init__(self, gdm, q, params, weight_matrix: sp.csr_array):
        super().__init__(gdm, q, params)
        self.scores = None
        opts = params.interactive_options
        n = q.index.vectors.shape[0]
        self.gamma = opts["gamma"]
        if self.gamma["mode"] == "clip":
            calibration = self.gamma["calibration"]
            if calibration == "ground_truth":
                self._calibrator = q.get_calibrator()
                assert self._calibrator is not None
            elif calibration == "sigmoid":
                self._calibrator = FixedCalibrator(a=self.gamma["a"], b=self.gamma["b"], sigmoid=True)
            else:
                assert calibration == "raw", f"unknown {calibration=}"
                self._calibrator = FixedCalibrator(a=1.0, b=0.0, sigmoid=False)
            initial_gamma = initial_gamma_array(0.1, n)  # over-written by set_text_vec
        else:
            assert self.gamma["mode"] == "fixed"
            initial_gamma = initial_gamma_array(self.gamma["value"], n)
        self.prob_model = _model_class(opts, planner=True).from_dataset(
            Dataset.from_vectors(q.index.vectors), gamma=initial_gamma, weight_matrix=weight_matrix,
            device=getattr(q.index, "device", 0) or 0)
        self.dataset = self.prob_model.dataset
        self.pruned_fractions = []
        self.refine_not_called_before = True

    @staticmethod
    def from_params(gdm, q, p):
        return ActiveSearch(gdm, q, p, weight_matrix=get_label_prop(q, p.interactive_options).lp.weight_matrix)

    def set_text_vec(self, tvec):
        super().set_text_vec(tvec)
        self.scores = self.q.index.score(tvec)
        if self.gamma["mode"] == "clip":
            probs = self._calibrator.get_probabilities(tvec, self.q.index.vectors, scores=self.scores)
            self.prob_model = self.prob_model.with_gamma(np.asarray(probs, dtype=np.float64))

    def get_stats(self):
        return {"pruned_fractions": self.pruned_fractions}

    def next_batch(self):
        opts = self.params.interactive_options
        horizon = self._horizon()
        res = efficient_nonmyopic_search(self.prob_model, reward_horizon=horizon, lookahead_limit=min(2, horizon),
                                         pruning_on=opts["pruning_on"], implementation=opts["implementation"])
        print(f"{res.index=}, {res.value=}")
        self.pruned_fractions.append(res.pruned_fraction)
        abs_idx = self.q.index.vector_meta["dbidx"].iloc[np.array([int(res.index)])].values
        ans = {"dbidxs": abs_idx, "activations": None}
        self.q.returned.update(ans["dbidxs"])
        return ans

    def _horizon(self):
        opts = self.params.interactive_options
        remaining = opts["max_steps"] - len(self.q.returned) if opts["adjust_horizon"] else math.inf
        horizon = int(min(opts["reward_horizon"], remaining))
        assert horizon > 0, "need a non-negative horizon for reward to be defined"
        return horizon

    @classmethod
    def next_batch_group(cls, loops):
        """`[l.next_batch() for l in loops]` with ONE planning call (ssw_lknn_step_batch) for loops whose models are
        DeviceLKNNModels of one device, node count and degree: every loop's horizon is worked out (and asserted) on the
        host first, then one call plans for all, then every loop prints, records and returns as its own `next_batch`.
        A loop whose slot the library refused surfaces its error after the other loops have been served."""
        loops = list(loops)
        if not loops:
            return []
        horizons = [l._horizon() for l in loops]
        results = efficient_nonmyopic_search_batch([l.prob_model for l in loops], horizons, [min(2, t) for t in horizons],
                                                   return_errors=True)
        out, failed = [], None
        for l, res in zip(loops, results):
            if isinstance(res, Exception):
                failed = failed or res
                out.append(None)
                continue
            print(f"{res.index=}, {res.value=}")
            l.pruned_fractions.append(res.pruned_fraction)
            abs_idx = l.q.index.vector_meta["dbidx"].iloc[np.array([int(res.index)])].values
            ans = {"dbidxs": abs_idx, "activations": None}
            l.q.returned.update(ans["dbidxs"])
            out.append(ans)
        if failed is not None:
            raise failed
        return out

    def refine(self, change=None):
        assert change is not None
        print(f"updating model with {change=}")
        if self.refine_not_called_before:  # getXy already includes this latest update
            pos, neg = self.q.getXy(get_positions=True)
            translated = [(int(i), 1) for i in pos] + [(int(i), 0) for i in neg]
        else:
            translated = [(_vector_position(self.q.index, idx), y) for idx, y in change]
        _condition_all(self.prob_model, translated)
        self.refine_not_called_before = False


class LKNNSearch(LoopBase):
    def __init__(self, gdm, q, params, weight_matrix: sp.csr_array):
        super().__init__(gdm, q, params)
        opts = params.interactive_options
        self._calibrator = q.get_calibrator()  # debug / experiments only
        if opts["gamma"] == "calibrate":
            assert self._calibrator is not None
            gamma_mean = self._calibrator.get_mean()
        else:
            gamma_mean = opts["gamma"]
        n = q.index.vectors.shape[0]
        self.use_clip_as_gamma = opts["use_clip_as_gamma"]
        self.prob_model = _model_class(opts, planner=False).from_dataset(
            Dataset.from_vectors(q.index.vectors), gamma=initial_gamma_array(gamma_mean, n), weight_matrix=weight_matrix,
            device=getattr(q.index, "device", 0) or 0)
        self.dataset = self.prob_model.dataset

    @staticmethod
    def from_params(gdm, q, p):
        return LKNNSearch(gdm, q, p, weight_matrix=get_label_prop(q, p.interactive_options).lp.weight_matrix)

    def set_text_vec(self, tvec):
        super().set_text_vec(tvec)
        self.scores = self.q.index.score(tvec)
        if self.use_clip_as_gamma:
            probs = self.scores if self._calibrator is None else self._calibrator.get_probabilities(tvec, self.q.index.vectors, scores=self.scores)
            self.prob_model = self.prob_model.with_gamma(np.asarray(probs, dtype=np.float64))

    def next_batch(self):
        vec_idx, _ = self.prob_model.top_k_remaining(top_k=1)
        print(f"{vec_idx=}")
        abs_idx = self.q.index.vector_meta["dbidx"].iloc[vec_idx].values
        ans = {"dbidxs": abs_idx, "activations": None}
        self.q.returned.update(ans["dbidxs"])
        return ans

    @classmethod
    def next_batch_group(cls, loops):
        """`[l.next_batch() for l in loops]` with ONE ssw_lknn_top_remaining_batch call for loops whose models are
        DeviceLKNNModels of one device, node count and degree.  A loop whose slot failed surfaces its error after the
        other loops have been served."""
        loops = list(loops)
        if not loops:
            return []
        entries = DeviceLKNNModel.top_k_remaining_batch([l.prob_model for l in loops], [1] * len(loops))
        out, failed = [], None
        for l, entry in zip(loops, entries):
            if isinstance(entry, Exception):
                failed = failed or entry
                out.append(None)
                continue
            vec_idx, _ = entry
            print(f"{vec_idx=}")
            abs_idx = l.q.index.vector_meta["dbidx"].iloc[vec_idx].values
            ans = {"dbidxs": abs_idx, "activations": None}
            l.q.returned.update(ans["dbidxs"])
            out.append(ans)
        if failed is not None:
            raise failed
        return out

    def refine(self, change=None):
        assert change is not None
        print(f"updating model with {change=}")
        translated = [(_vector_position(self.q.index, idx), y) for idx, y in change]
        _condition_all(self.prob_model, translated)
