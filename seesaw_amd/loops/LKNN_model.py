"""LKNNModel: the L-KNN probability model of the active-search loops (seesaw/loops/LKNN_model.py:76-281).

p_i = (gamma_i + sum of the labels of i's labelled neighbours) / (1 + number of labelled neighbours).  The state is
three host arrays (numerators, denominators, gamma) over the nodes and the CSR neighbour lists; conditioning on a
label touches one row of neighbours.  What is expensive in the reference -- the look-ahead value of every node,
an N x (K + 2D) argsort per planning step -- runs on the GPU (`top_sum`, ssw_lknn_top_sum).  The descending order of the
scores is sorted in full only where the scores are new as a whole (from_dataset, with_gamma: once per text query);
after an answer (condition_) the handful of changed nodes is merged back into it.

DeviceLKNNModel (below) is the same model with its state resident on the device and no order kept at all."""
from __future__ import annotations

import ctypes
import math
from typing import Tuple

import numpy as np
import scipy.sparse as sp

from .. import _lib
from ..bitmap import FrozenBitMap
from ..research.active_search.common import Dataset, ProbabilityModel


def initial_gamma_array(gamma, shape):
    """the prior, jittered by 1e-6 so that no two nodes tie (LKNN_model.py:70-73)"""
    return np.random.default_rng(seed=0).normal(loc=gamma, scale=1e-6, size=shape)


def _reinsert_sorted(desc_idx, desc_score, changed, score):
    """the descending order after the scores of a handful of nodes changed: those nodes are taken out of the order and
    merged back at their new places -- O(N) copies instead of the reference's full `np.argsort(-score)` per answer
    (seesaw/loops/LKNN_model.py:185: ~0.1 s at 1.56 M nodes).  Equal to that argsort whenever the scores are distinct (the
    prior is jittered so that they are, LKNN_model.py:70-73); among exactly equal scores a node that moved goes before
    the ones that stayed, where introsort's order is unspecified."""
    changed = np.unique(np.asarray(changed, dtype=np.int64))
    if changed.shape[0] == 0:
        return desc_idx, desc_score
    stay = np.ones(score.shape[0], dtype=bool)
    stay[changed] = False
    keep = stay[desc_idx]
    old_idx, old_score = desc_idx[keep], desc_score[keep]
    new_score = score[changed]
    order = np.argsort(-new_score, kind="stable")
    changed, new_score = changed[order], new_score[order]
    at = np.searchsorted(-old_score, -new_score, side="left")  # before the stayers of equal score
    return np.insert(old_idx, at, changed), np.insert(old_score, at, new_score)


class LKNNModel(ProbabilityModel):
    def __init__(self, dataset: Dataset, gamma, matrix: sp.csr_array, numerators, denominators, score, desc_idx, desc_score,
                 desc_changed_idx, desc_changed_score, device: int = 0, _gpu=None):
        super().__init__(dataset)
        self.matrix, self.numerators, self.denominators, self.score, self.gamma = matrix, numerators, denominators, score, gamma
        assert gamma.shape == self.numerators.shape
        assert ((0 < gamma) & (gamma < 1)).all(), "this could fail by chance, decrase var. or fix properly by applying sigmoid"
        self.desc_idx, self.desc_score = desc_idx, desc_score
        self.desc_changed_idx, self.desc_changed_score = desc_changed_idx, desc_changed_score  # filled by condition()
        self.device = device
        self._gpu = _gpu if _gpu is not None else {}  # shared by the models derived from one another: one device handle
        self._init_sets()

    def _init_sets(self):
        self.changed_idx_set = FrozenBitMap(self.desc_changed_idx) if self.desc_changed_idx is not None else FrozenBitMap()
        self.ignore_set = self.dataset.seen_indices.union(self.changed_idx_set)

    @staticmethod
    def from_dataset(dataset: Dataset, weight_matrix: sp.csr_array, gamma: np.ndarray, device: int = 0):
        assert weight_matrix.format == "csr"
        assert len(dataset.idx2label) == 0, "not implemented other case"
        sz = weight_matrix.shape[0]
        assert gamma.shape == (sz,)
        init_scores = (np.zeros(sz) + gamma) / (np.zeros(sz) + 1)
        order = np.argsort(-init_scores)
        return LKNNModel(dataset, gamma=gamma, matrix=weight_matrix, numerators=np.zeros(sz), denominators=np.zeros(sz),
                         score=init_scores, desc_idx=order, desc_score=init_scores[order], desc_changed_idx=None,
                         desc_changed_score=None, device=device)

    def _derive(self, **kw):
        base = dict(dataset=self.dataset, gamma=self.gamma, matrix=self.matrix, numerators=self.numerators,
                    denominators=self.denominators, score=self.score, desc_idx=self.desc_idx, desc_score=self.desc_score,
                    desc_changed_idx=self.desc_changed_idx, desc_changed_score=self.desc_changed_score, device=self.device,
                    _gpu=self._gpu)
        base.update(kw)
        return LKNNModel(**base)

    # ---- conditioning -------------------------------------------------------------------------
    def _condition_shared(self, idx, y, ret_num_denom=False):
        start, end = self.matrix.indptr[idx:idx + 2]
        neighbors = self.matrix.indices[start:end]
        assert self.dataset.idx2label.get(idx, None) is None, "no benchmark scenario should reach this"
        num, den, gam = self.numerators[neighbors], self.denominators[neighbors], self.gamma[neighbors]
        change = (num + y + gam) / (den + 1 + 1)
        order = np.argsort(-change)
        nd = (num + y, den + 1) if ret_num_denom else (None, None)
        return self.dataset.with_label(idx, y), neighbors, neighbors[order], change[order], change, nd[0], nd[1]

    def condition(self, idx, y) -> "LKNNModel":
        """a NEW model with idx labelled y: the base arrays are shared, the changed neighbours ride along sorted"""
        assert self.desc_changed_idx is None
        ds, _, chg_idx, chg_score, _, _, _ = self._condition_shared(idx, y)
        return self._derive(dataset=ds, desc_changed_idx=chg_idx, desc_changed_score=chg_score)

    def with_gamma(self, new_gamma: np.ndarray) -> "LKNNModel":
        assert self.desc_changed_idx is None, "check this is correct"
        scores = (self.numerators + new_gamma) / (self.denominators + 1)
        order = np.argsort(-scores)
        return self._derive(gamma=new_gamma, score=scores, desc_idx=order, desc_score=scores[order])

    def condition_(self, idx, y):
        """in place (after the user's answer): neighbours' counts and scores, then the descending order"""
        assert self.desc_changed_idx is None
        ds, neighbors, _, _, change, num, den = self._condition_shared(idx, y, ret_num_denom=True)
        self.dataset = ds
        self.numerators[neighbors], self.denominators[neighbors], self.score[neighbors] = num, den, change
        self.desc_idx, self.desc_score = _reinsert_sorted(self.desc_idx, self.desc_score, neighbors, self.score)
        self._init_sets()

    # ---- queries ------------------------------------------------------------------------------
    def predict_proba(self, idxs) -> np.ndarray:
        assert self.desc_changed_idx is None, "is this ever called after first round"
        return self.score[np.asarray(idxs, dtype=np.int64)]

    def _iter_desc_scores(self):
        for idx, score in zip(self.desc_idx, self.desc_score):
            if idx not in self.ignore_set:
                yield idx, score

    def _iter_changed_scores(self):
        for idx, score in zip(self.desc_changed_idx, self.desc_changed_score):
            if idx not in self.dataset.seen_indices:
                yield idx, score

    def iter_desc(self):
        """both streams merged in descending order, without the nodes already seen"""
        if self.desc_changed_idx is None:
            yield from self._iter_desc_scores()
            return
        it1, it2 = self._iter_desc_scores(), self._iter_changed_scores()
        end = (-1, -math.inf)
        (i1, s1), (i2, s2) = next(it1, end), next(it2, end)
        while i1 > -1 or i2 > -1:
            if s1 >= s2:
                yield i1, s1
                i1, s1 = next(it1, end)
            else:
                yield i2, s2
                i2, s2 = next(it2, end)

    def top_k_remaining(self, top_k: int) -> Tuple[np.ndarray, np.ndarray]:
        idxs, vals = [], []
        for i, (idx, val) in enumerate(self.iter_desc()):
            if i >= top_k:
                break
            idxs.append(idx)
            vals.append(val)
        return np.array(idxs), np.array(vals)

    def probability_bound(self, n):
        idxs = np.asarray(self.dataset.remaining_indices(), dtype=np.int64)
        return np.max((self.gamma[idxs] + n + self.numerators[idxs]) / (1 + n + self.denominators[idxs]))

    # ---- the look-ahead on the GPU --------------------------------------------------------------
    def regular_degree(self) -> int:
        deltas = np.diff(self.matrix.indptr)
        assert (deltas == deltas[0]).all(), "the vectorised look-ahead needs the same number of neighbours for every node"
        return int(deltas[0])

    # what ssw_lknn_top_sum keeps per thread (csrc/lknn.hip): K picks, D neighbours, a K + D list with a 192-bit mask
    KERNEL_MAX_K, KERNEL_MAX_D, KERNEL_MAX_LIST = 128, 32, 192

    @staticmethod
    def _top_sum_host(numer, denom, scores, nbr_sorted, K, top, block=4096):
        """the look-ahead values on the host, for horizons / degrees beyond the kernel's registers (reward_horizon > 129,
        more than 32 neighbours): same quantities, rows in blocks.  For node i the pool is the global list `top` without i
        and without i's neighbours, plus the neighbours at their conditioned scores; value = sum of its K best."""
        N, D = nbr_sorted.shape
        t_sorted_pos = np.argsort(top, kind="stable")
        t_ids = top[t_sorted_pos].astype(np.int64)
        t_scores = scores[t_ids]
        given0 = numer / (denom + 1)
        given1 = (numer + 1) / (denom + 1)
        out = np.empty(N, dtype=np.float64)
        for a in range(0, N, block):
            b = min(N, a + block)
            rows = np.arange(a, b, dtype=np.int64)[:, None]
            nb = nbr_sorted[a:b].astype(np.int64)
            base = np.broadcast_to(t_scores, (b - a, t_ids.shape[0])).copy()
            base[t_ids[None, :] == rows] = -np.inf                      # the node itself leaves the list
            pos = np.searchsorted(t_ids, nb)                            # neighbours that sit in the list are replaced
            hit = np.take(np.append(t_ids, N), pos) == nb
            rr, cc = np.nonzero(hit)
            base[rr, pos[rr, cc]] = -np.inf
            vals = []
            for cond in (given1, given0):
                ns = np.take(cond, nb)
                ns[nb == rows] = -np.inf
                pool = np.concatenate([base, ns], axis=1)
                best = -np.sort(-pool, axis=1)[:, :K]                   # descending: the order the reference adds them in
                assert (best > -np.inf).all(), "fewer than K candidates left for some node"
                vals.append(best.sum(axis=1))
            s = scores[a:b]
            out[a:b] = s * (1 + vals[0]) + (1 - s) * vals[1]
        return out

    def top_sum(self, K: int, return_values: bool = False):
        """_top_sum (efficient_nonmyopic_search.py:94-169) for the current state: value of labelling every node next,
        K further picks into the future.  -> (best index, best value[, all values])"""
        D = self.regular_degree()
        N = self.matrix.shape[0]
        h = self._gpu.get("handle")
        if h is None:
            nbr = np.ascontiguousarray(np.sort(self.matrix.indices.reshape(-1, D)), dtype=np.int32)
            h = ctypes.c_void_p()
            _lib.call("ssw_lknn_create", int(self.device), N, D, ctypes.c_void_p(nbr.ctypes.data), ctypes.byref(h))
            self._gpu["handle"] = h
            self._gpu["owner"] = _Handle(h)
        numer = self.numerators + self.gamma
        denom = self.denominators + 1
        seen = np.asarray(self.dataset.seen_indices, dtype=np.int64)
        numer[seen] = -math.inf  # will rank lowest
        assert (numer <= denom).all()
        scores = numer / denom
        L = K + D
        assert N - seen.shape[0] >= L, f"{N - seen.shape[0]} unseen nodes cannot fill a look-ahead list of K + D = {L}"
        part = np.argpartition(-scores, L - 1)[:L]          # the K + D best, then ordered: O(N) instead of a full sort
        top = part[np.argsort(-scores[part], kind="stable")].astype(np.int32)
        assert np.isfinite(scores[top]).all()               # (the reference's `top_k_scores > -inf`)
        if K > self.KERNEL_MAX_K or D > self.KERNEL_MAX_D or L > self.KERNEL_MAX_LIST:
            with np.errstate(invalid="ignore"):
                values = self._top_sum_host(numer, denom, scores, np.sort(self.matrix.indices.reshape(-1, D)), K, top)
            best = int(np.nanargmax(values))
            return (best, float(values[best]), values) if return_values else (best, float(values[best]))
        numer, denom = np.ascontiguousarray(numer), np.ascontiguousarray(denom)
        values = np.empty(N, dtype=np.float64) if return_values else None
        best_i, best_v = ctypes.c_int64(-1), ctypes.c_double(0.0)
        _lib.call("ssw_lknn_top_sum", h, ctypes.c_void_p(numer.ctypes.data), ctypes.c_void_p(denom.ctypes.data),
                  ctypes.c_void_p(top.ctypes.data), int(K), None if values is None else ctypes.c_void_p(values.ctypes.data),
                  ctypes.byref(best_i), ctypes.byref(best_v))
        return (int(best_i.value), float(best_v.value), values) if return_values else (int(best_i.value), float(best_v.value))


class DeviceLKNNModel(ProbabilityModel):
    """LKNNModel with its state on the device (interactive_options["model_on_device"]): numerators, denominators, gamma
    and the seen marks live on an ssw_lknn handle; an answer is one enqueued kernel (ssw_lknn_condition), a planning
    step one call with one host wait (ssw_lknn_step).  The host keeps the dataset (seen bitmap, idx2label) and nothing of
    size N: no sorted order, no score array.  The object is mutable: with_gamma and condition_ change it in place, so the
    recursive planner's condition() is not offered -- implementation='vectorized' only.

    Nodes are ranked by (score descending, node id ascending).  Whenever the K + D + 1 highest unseen scores are pairwise
    distinct -- the jittered prior sees to that -- picks, values and value vectors equal LKNNModel's bit for bit."""
    device_resident = True
    KERNEL_MAX_K, KERNEL_MAX_D, KERNEL_MAX_LIST = LKNNModel.KERNEL_MAX_K, LKNNModel.KERNEL_MAX_D, LKNNModel.KERNEL_MAX_LIST
    MAX_CALL = 4096  # answers of one ssw_lknn_condition, nodes of one ssw_lknn_predict

    def __init__(self, dataset: Dataset, owner: "_Handle", n: int, degree: int, device: int):
        super().__init__(dataset)
        self._owner, self.n, self.degree, self.device = owner, n, degree, device

    @staticmethod
    def from_dataset(dataset: Dataset, weight_matrix: sp.csr_array, gamma: np.ndarray, device: int = 0):
        if getattr(weight_matrix, "format", None) != "csr":
            raise ValueError("the device-resident L-KNN model needs a CSR weight matrix")
        if len(dataset.idx2label) != 0:
            raise ValueError("the device-resident L-KNN model starts from a dataset without labels")
        n = weight_matrix.shape[0]
        deltas = np.diff(weight_matrix.indptr)
        if n == 0 or not (deltas == deltas[0]).all() or not 1 <= int(deltas[0]) <= DeviceLKNNModel.KERNEL_MAX_D:
            raise ValueError("the device-resident L-KNN model needs a regular graph (the same number of neighbours for every "
                             f"node) of degree 1..{DeviceLKNNModel.KERNEL_MAX_D}; this one has {int(deltas.min()) if n else 0}.."
                             f"{int(deltas.max()) if n else 0} neighbours a node; there is no host fallback")
        degree = int(deltas[0])
        gamma = DeviceLKNNModel._checked_gamma(gamma, n)
        nbr = np.ascontiguousarray(np.sort(weight_matrix.indices.reshape(-1, degree)), dtype=np.int32)
        h = ctypes.c_void_p()
        _lib.call("ssw_lknn_create", int(device), n, degree, ctypes.c_void_p(nbr.ctypes.data), ctypes.byref(h))
        owner = _Handle(h)
        _lib.call("ssw_lknn_state_init", h, ctypes.c_void_p(gamma.ctypes.data))
        return DeviceLKNNModel(dataset, owner, n, degree, int(device))

    @staticmethod
    def _checked_gamma(gamma, n):
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        assert gamma.shape == (n,)
        assert ((0 < gamma) & (gamma < 1)).all(), "this could fail by chance, decrase var. or fix properly by applying sigmoid"
        return gamma

    @property
    def _h(self):
        if self._owner is None:
            raise RuntimeError("this DeviceLKNNModel is closed")
        return self._owner.h

    def close(self):
        if self._owner is not None:
            self._owner.close()
            self._owner = None

    # ---- conditioning -------------------------------------------------------------------------
    def condition(self, idx, y):
        raise NotImplementedError("the device-resident model is conditioned in place (condition_); the recursive planner "
                                  "(implementation='loop') needs the host LKNNModel")

    def probability_bound(self, n):
        raise NotImplementedError("pruning is not served by the device-resident model")

    def with_gamma(self, new_gamma: np.ndarray) -> "DeviceLKNNModel":
        """replaces gamma IN PLACE (one upload), keeps counts and seen marks; returns self"""
        gamma = self._checked_gamma(new_gamma, self.n)
        _lib.call("ssw_lknn_set_gamma", self._h, ctypes.c_void_p(gamma.ctypes.data))
        return self

    def condition_(self, idx, y):
        self.condition_many_([(idx, y)])

    def condition_many_(self, pairs):
        """the answers [(idx, y), ...] in order, one enqueued call per 4096 of them (a refused call changes nothing)"""
        pairs = [(int(i), int(y)) for i, y in pairs]
        for a in range(0, len(pairs), self.MAX_CALL):
            part = pairs[a:a + self.MAX_CALL]
            ids = np.array([i for i, _ in part], dtype=np.int64)
            ys = np.array([y for _, y in part], dtype=np.int32)
            _lib.call("ssw_lknn_condition", self._h, ctypes.c_void_p(ids.ctypes.data), ctypes.c_void_p(ys.ctypes.data), len(part))
            for i, y in part:
                self.dataset = self.dataset.with_label(i, y)

    # ---- queries ------------------------------------------------------------------------------
    def step(self, K: int, lookahead: int, return_values: bool = False, return_list: bool = False):
        """one planning step (ssw_lknn_step).  lookahead 2: LKNNModel.top_sum(K); lookahead 1: the most probable unseen
        node and its score.  -> (best index, best value[, all values][, the K + D selected nodes])"""
        values = np.empty(self.n, dtype=np.float64) if return_values else None
        chosen = np.empty(K + self.degree, dtype=np.int32) if return_list and lookahead == 2 else None
        best_i, best_v = ctypes.c_int64(-1), ctypes.c_double(0.0)
        _lib.call("ssw_lknn_step", self._h, int(K), int(lookahead), ctypes.byref(best_i), ctypes.byref(best_v),
                  None if values is None else ctypes.c_void_p(values.ctypes.data),
                  None if chosen is None else ctypes.c_void_p(chosen.ctypes.data))
        out = (int(best_i.value), float(best_v.value))
        if return_values:
            out += (values,)
        if return_list:
            out += (chosen,)
        return out

    def top_sum(self, K: int, return_values: bool = False):
        return self.step(K, 2, return_values=return_values)

    def top_k_remaining(self, top_k: int) -> Tuple[np.ndarray, np.ndarray]:
        if not 1 <= top_k <= self.KERNEL_MAX_LIST:
            raise ValueError(f"top_k={top_k}: the device-resident model lists 1..{self.KERNEL_MAX_LIST} nodes")
        ids, scores = np.empty(top_k, dtype=np.int32), np.empty(top_k, dtype=np.float64)
        count = ctypes.c_int32(0)
        _lib.call("ssw_lknn_top_remaining", self._h, int(top_k), ctypes.c_void_p(ids.ctypes.data),
                  ctypes.c_void_p(scores.ctypes.data), ctypes.byref(count))
        return ids[:count.value].astype(np.int64), scores[:count.value]

    # ---- several models in one call ------------------------------------------------------------
    MAX_BATCH = 256  # SSW_LKNN_MAX_BATCH
    last_batch_stats = None  # of the last step_batch: launches, host_waits, bytes_to_device, bytes_to_host

    @staticmethod
    def _handles(models):
        hs = (ctypes.c_void_p * len(models))(*[m._h for m in models])
        return hs

    @staticmethod
    def _slot_error(model, status):
        msg = _lib.load().ssw_lknn_batch_error(model._h)
        return _lib.SeesawHipError(int(status), msg.decode("utf-8", "replace") if msg else "")

    @staticmethod
    def step_batch(models, Ks, lookaheads, return_values: bool = False, return_list: bool = False):
        """`[m.step(K, lookahead, ...) for m, K, lookahead in zip(models, Ks, lookaheads)]` in one call with one host wait
        (ssw_lknn_step_batch): one entry per model, what `step` returns or the SeesawHipError it would have raised.  The
        models are distinct and share device, node count and degree (otherwise the call raises and nothing ran)."""
        models = list(models)
        S = len(models)
        Ks = np.ascontiguousarray([int(k) for k in Ks], dtype=np.int32)
        lookaheads = np.ascontiguousarray([int(a) for a in lookaheads], dtype=np.int32)
        assert Ks.shape == (S,) and lookaheads.shape == (S,)
        hs = DeviceLKNNModel._handles(models)
        values = [np.empty(m.n, dtype=np.float64) for m in models] if return_values else None
        value_ptrs = (ctypes.c_void_p * S)(*[v.ctypes.data for v in values]) if return_values else None
        lists = np.full((S, DeviceLKNNModel.KERNEL_MAX_LIST), -1, dtype=np.int32) if return_list else None
        best_i, best_v = np.full(S, -1, dtype=np.int64), np.zeros(S, dtype=np.float64)
        status, stats = np.zeros(S, dtype=np.int32), np.zeros(4, dtype=np.int64)
        _lib.call("ssw_lknn_step_batch", hs, S, ctypes.c_void_p(Ks.ctypes.data), ctypes.c_void_p(lookaheads.ctypes.data),
                  ctypes.c_void_p(best_i.ctypes.data), ctypes.c_void_p(best_v.ctypes.data), value_ptrs,
                  None if lists is None else ctypes.c_void_p(lists.ctypes.data), ctypes.c_void_p(status.ctypes.data),
                  ctypes.c_void_p(stats.ctypes.data))
        DeviceLKNNModel.last_batch_stats = dict(launches=int(stats[0]), host_waits=int(stats[1]), bytes_to_device=int(stats[2]),
                                                bytes_to_host=int(stats[3]))
        out = []
        for j, m in enumerate(models):
            if status[j] != _lib.SSW_OK:
                out.append(DeviceLKNNModel._slot_error(m, status[j]))
                continue
            entry = (int(best_i[j]), float(best_v[j]))
            if return_values:
                entry += (values[j],)
            if return_list:
                entry += (lists[j, :int(Ks[j]) + m.degree].copy() if lookaheads[j] == 2 else None,)
            out.append(entry)
        return out

    @staticmethod
    def top_k_remaining_batch(models, top_ks):
        """`[m.top_k_remaining(k) for m, k in zip(models, top_ks)]` in one call with one host wait
        (ssw_lknn_top_remaining_batch): one entry per model, (ids, scores) or the error that call would have raised"""
        models = list(models)
        S = len(models)
        ks = np.ascontiguousarray([int(k) for k in top_ks], dtype=np.int32)
        assert ks.shape == (S,)
        hs = DeviceLKNNModel._handles(models)
        ids = np.empty((S, DeviceLKNNModel.KERNEL_MAX_LIST), dtype=np.int32)
        scores = np.empty((S, DeviceLKNNModel.KERNEL_MAX_LIST), dtype=np.float64)
        counts, status = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
        _lib.call("ssw_lknn_top_remaining_batch", hs, S, ctypes.c_void_p(ks.ctypes.data), ctypes.c_void_p(ids.ctypes.data),
                  ctypes.c_void_p(scores.ctypes.data), ctypes.c_void_p(counts.ctypes.data), ctypes.c_void_p(status.ctypes.data))
        out = []
        for j, m in enumerate(models):
            if status[j] != _lib.SSW_OK:
                if not 1 <= ks[j] <= DeviceLKNNModel.KERNEL_MAX_LIST:  # what top_k_remaining raises before the library is asked
                    out.append(ValueError(f"top_k={int(ks[j])}: the device-resident model lists 1..{DeviceLKNNModel.KERNEL_MAX_LIST} nodes"))
                else:
                    out.append(DeviceLKNNModel._slot_error(m, status[j]))
                continue
            out.append((ids[j, :counts[j]].astype(np.int64), scores[j, :counts[j]].copy()))
        return out

    def predict_proba(self, idxs) -> np.ndarray:
        idxs = np.ascontiguousarray(np.asarray(idxs, dtype=np.int64).reshape(-1))
        out = np.empty(idxs.shape[0], dtype=np.float64)
        for a in range(0, idxs.shape[0], self.MAX_CALL):
            m = min(self.MAX_CALL, idxs.shape[0] - a)
            _lib.call("ssw_lknn_predict", self._h, ctypes.c_void_p(idxs[a:].ctypes.data), m, ctypes.c_void_p(out[a:].ctypes.data))
        return out

    def state(self) -> dict:
        """the resident state copied back: numerators, denominators, gamma (f64 [N]), seen (bool [N])"""
        num, den, gam = (np.empty(self.n, dtype=np.float64) for _ in range(3))
        seen = np.empty(self.n, dtype=np.uint8)
        _lib.call("ssw_lknn_state_fetch", self._h, *(ctypes.c_void_p(a.ctypes.data) for a in (num, den, gam, seen)))
        return dict(numerators=num, denominators=den, gamma=gam, seen=seen.astype(bool))

    def step_info(self) -> dict:
        out = np.zeros(4, dtype=np.int64)
        _lib.call("ssw_lknn_step_info", self._h, ctypes.c_void_p(out.ctypes.data))
        return dict(launches=int(out[0]), host_waits=int(out[1]), bytes_to_device=int(out[2]), bytes_to_host=int(out[3]))

    def step_times(self, enable: bool = True):
        """(selection ms, look-ahead ms) of the last step from device events, None where it was not timed; steps from now
        on are timed or not"""
        out = np.zeros(2, dtype=np.float64)
        _lib.call("ssw_lknn_step_times", self._h, int(bool(enable)), ctypes.c_void_p(out.ctypes.data))
        return None if out[0] < 0 else (float(out[0]), float(out[1]))


class _Handle:
    def __init__(self, h):
        self.h = h

    def close(self):
        if self.h is not None:
            h, self.h = self.h, None
            _lib.call("ssw_lknn_destroy", h)

    def __del__(self):
        try:
            _lib.load().ssw_lknn_destroy(self.h)
        except Exception:
            pass
