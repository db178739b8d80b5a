"""Session: one user's search -- text query, batches of results, labels back, refine.

Interface of seesaw/seesaw_session.py:12-245 (`set_text`, `next`, `update_state`, `refine`,
`get_state`, `make_session`); control flow only, every numeric step is in the index / loop.
"""
from __future__ import annotations

import os
import time

import numpy as np

from .basic_types import (ActivationData, BenchParams, Box, Imdata, LogEntry, SessionParams, SessionState,
                          is_image_accepted)
from .bitmap import BitMap
from .indices.interface import AccessMethod
from .labeldb import LabelDB
from .loops.registry import build_loop_from_params


class Session:
    """State kept per session: the batches returned so far (`acc_indices`, `acc_activations`), which images were
    seen / accepted, the label database of the query object (`q.label_db`, what the loops learn from), per-call
    timings and the action log.  The loop object (`self.loop`) owns the ranking state."""

    def __init__(self, gdm, dataset, hdb: AccessMethod, params: SessionParams, _y: np.ndarray = None):
        self.gdm, self.dataset, self.index, self.params = gdm, dataset, hdb, params
        self.acc_indices, self.acc_activations = [], []   # one entry per batch returned
        self.seen, self.accepted = BitMap([]), BitMap([])
        self.timing, self.image_timing = [], {}           # seconds per next(); UI intervals per image
        self.init_q = None                                 # the text of the query, once set
        self.q = hdb.new_query()
        if _y is not None:
            from .calibration import GroundTruthCalibrator
            assert self.index.vectors.shape[0] == _y.shape[0]
            self.q._calibrator = GroundTruthCalibrator(self.index.vectors, _y)
        self.label_db = LabelDB()  # optional prefill from ground truth (annotation_category)
        if params.annotation_category is not None:
            box_data, _ = dataset.load_ground_truth()
            df = box_data[box_data.category == params.annotation_category]
            if df.shape[0] == 0:
                print(f"warning, no entries found for category {params.annotation_category}")
            self.label_db.fill(df)
        self.loop = build_loop_from_params(gdm, self.q, params=params)
        self._log_raw = []  # (time, message, seen, accepted): LogEntry objects are built when somebody reads action_log
        self._last_change = None
        self._log("init")

    def get_totals(self):
        """counts shown by the UI header"""
        return dict(seen=len(self.seen), accepted=len(self.accepted))

    def get_method_stats(self):
        """whatever the loop wants recorded in the benchmark summary"""
        return self.loop.get_stats()

    def _log(self, message: str):
        self._log_raw.append((time.time(), message, len(self.seen), len(self.accepted)))

    @property
    def action_log(self):
        """the reference's list of LogEntry (seesaw_session.py:56-62), materialised on demand: five pydantic objects a
        round were a tenth of a `plain` round at LVIS-subset size"""
        raw = self._log_raw  # materialised in place and returned itself: a client's `session.action_log.append(...)` stays
        for i, e in enumerate(raw):
            if isinstance(e, tuple):
                raw[i] = LogEntry.model_construct(logger="server", time=e[0], message=e[1], seen=e[2], accepted=e[3])
        return raw

    @action_log.setter
    def action_log(self, entries):  # update_state: the client hands the log back with its own entries in it
        self._log_raw = list(entries)

    def next(self):
        """next batch of image ids from the loop; the batch and its activations are remembered for get_state"""
        self._log("next.start")
        start = time.time()
        r = self.loop.next_batch_external()
        self.timing.append(time.time() - start)
        self.acc_indices.append(r["dbidxs"])
        self.acc_activations.append(r["activations"])
        self._log("next.end")
        return r["dbidxs"]

    def set_text(self, key):
        """embed the text (CLIP text tower through the index) and hand the unit vector to the loop"""
        self._log("set_text")
        self.init_q = key
        self.loop.state.curr_str = key
        vec = self.index.string2vec(string=key)
        # as in the reference, LoopState.tvec is never assigned (seesaw_session.py:96-103 sets curr_str only),
        # so LogReg2 / PseudoLR build their scorers with regularizer_vector=None: no regulariser at all.
        # Setting it here would "repair" them and change every result of those two loops.
        self.loop.set_text_vec(vec)

    def update_state(self, state: SessionState):
        """take the client's view of the session (labels drawn on the returned images) as the new truth"""
        self._update_labeldb(state)
        self._log("update_state.end")
        reversal = self._check_reversals()
        # update_last_batch() keeps this state incrementally; a session may mix both entry points (a client un-accepting
        # an earlier image goes through here), so the full walk refreshes it
        shown = [int(i) for b in self.acc_indices for i in np.asarray(b).reshape(-1)]
        self._rev = [any(i not in self.accepted for i in shown), reversal or self._reversal_ignoring_totals(shown)]
        if reversal:
            self.loop.set_reversals()

    # ---- the last batch only ---------------------------------------------------------------------------------
    # benchmark_loop's simulated user labels the batch it was just shown and never revisits an earlier one, yet
    # get_state() / update_state() (the web client's protocol, kept above) rebuild every batch so far on every round:
    # O(rounds) records, bitmap copies and label-db writes per round.  These two do the same bookkeeping for the
    # last batch alone; every set / label / change list ends up identical (tests: the reference's session sequences).
    def last_batch(self):
        """the Imdata records of the batch next() just returned (what get_state().gdata[-1] holds)"""
        prefill = self.params.annotation_category is not None
        return self.get_panel_data(idxbatch=self.acc_indices[-1], activation_batch=self.acc_activations[-1], prefill=prefill)

    def update_last_batch(self, batch):
        """update_state() for a state in which only the last batch changed"""
        seen, accepted, put = self.seen, self.accepted, self.q.label_db.put
        change = []
        for imdata in batch:
            dbidx = imdata.dbidx
            self.image_timing[dbidx] = imdata.timing
            new_seen = dbidx not in seen
            if new_seen:
                seen.add(dbidx)
            acc = is_image_accepted(imdata)
            new_acc = acc and dbidx not in accepted
            if new_acc:
                accepted.add(dbidx)
            put(dbidx, imdata.boxes)
            if new_seen or new_acc:
                change.append((dbidx, 1 if new_acc else 0))
            # reversal = an accepted image shown after a rejected one (sticky: earlier verdicts do not change here)
            rev = self.__dict__.setdefault("_rev", [False, False])  # [a rejected image was shown, reversal seen]
            if acc and rev[0]:
                rev[1] = True
            elif not acc:
                rev[0] = True
        self._last_change = sorted(change)  # ascending dbidx, as the bitmap union of update_state() lists them
        self._log("update_state.end")
        if self.__dict__.get("_rev", [False, False])[1] and len(accepted) != 0 and len(accepted) != len(seen):
            self.loop.set_reversals()

    def _reversal_ignoring_totals(self, shown):
        """an accepted image shown after a rejected one, without _check_reversals()'s all / none shortcuts (those are
        re-applied by update_last_batch each round, on the totals of that round)"""
        rejected_before = False
        for i in shown:
            if i not in self.accepted:
                rejected_before = True
            elif rejected_before:
                return True
        return False

    def _check_reversals(self):
        """a reversal = some rejected image shown before an accepted one."""
        if len(self.accepted) == 0 or len(self.accepted) == len(self.seen):
            return False
        rejected_before = False
        for batch in self.acc_indices:
            for idx in np.asarray(batch).reshape(-1):
                if int(idx) not in self.accepted:
                    rejected_before = True
                elif rejected_before:
                    return True
        return False

    def refine(self):
        """let the loop learn from the labels that changed since the last call"""
        self._log("refine.start")
        self.loop.refine_external(self._last_change)
        self._log("refine.end")

    def get_state(self) -> SessionState:
        """every batch so far as Imdata records (boxes from the label database), plus log and timings"""
        gdata = []
        last = len(self.acc_indices) - 1
        for i, (indices, accs) in enumerate(zip(self.acc_indices, self.acc_activations)):
            prefill = (self.params.annotation_category is not None) and (i == last)
            gdata.append(self.get_panel_data(idxbatch=indices, activation_batch=accs, prefill=prefill))
        return SessionState.model_construct(action_log=self.action_log, gdata=gdata, timing=self.timing,
                                            reference_categories=[], params=self.params,
                                            query_string=self.loop.state.curr_str)

    def _static_panel(self, idxbatch, activation_batch):
        """url + activation records of one batch: they never change once returned, so they are
        converted from the index's DataFrames once (the reference redoes it for every batch on
        every get_state, seesaw_session.py:153-186)."""
        key = id(idxbatch)
        cache = self.__dict__.setdefault("_panel_cache", {})
        hit = cache.get(key)
        if hit is None:
            urls = self.dataset.get_urls(idxbatch)
            acts = []
            if hasattr(activation_batch, "records") and len(activation_batch) == len(idxbatch):
                # the index's own result object: numbers straight from its arrays, no DataFrame in between
                acts = [[ActivationData(box=Box(x1=v[0], y1=v[1], x2=v[2], y2=v[3]), score=v[4])]
                        for v in activation_batch.records()]
            else:
                for i in range(len(idxbatch)):
                    if activation_batch is None or len(activation_batch) == 0:
                        acts.append(None)
                        continue
                    vals = activation_batch[i][["x1", "y1", "x2", "y2", "score"]].to_numpy(dtype=np.float64).tolist()
                    acts.append([ActivationData(box=Box(x1=v[0], y1=v[1], x2=v[2], y2=v[3]), score=v[4]) for v in vals])
            hit = cache[key] = (idxbatch, urls, acts)  # keeps idxbatch alive so its id stays unique
        return hit[1], hit[2]

    def get_panel_data(self, *, idxbatch, activation_batch=None, prefill=False):
        urls, acts = self._static_panel(idxbatch, activation_batch)
        db = self.label_db if prefill else self.q.label_db
        out = []
        cache = self.__dict__.setdefault("_imdata_cache", {})
        for url, dbidx, activations in zip(urls, idxbatch, acts):
            dbidx = int(dbidx)
            boxes, timing = db.get(dbidx, format="box"), self.image_timing.get(dbidx, None)
            # get_state() is called every round and walks every batch so far: the record of an image whose
            # boxes / timing objects have not been replaced since the last call is reused as it is
            hit = cache.get((dbidx, prefill))
            if hit is not None and hit[0] is boxes and hit[1] is timing:
                out.append(hit[2])
                continue
            im = Imdata.model_construct(url=url, dbidx=dbidx, boxes=boxes, activations=activations,
                                        timing=[] if timing is None else timing)
            if boxes is not None:  # (None = never shown: db.get builds nothing to key on)
                cache[(dbidx, prefill)] = (boxes, timing, im)
            out.append(im)
        return out

    def _update_labeldb(self, state: SessionState):
        # rebuilt from scratch every time: the user may have un-accepted an image
        self.action_log = state.action_log
        old_accepted, old_seen = self.accepted.copy(), self.seen.copy()
        self.accepted.clear()
        self.seen.clear()
        for batch in state.gdata:
            for imdata in batch:
                self.image_timing[imdata.dbidx] = imdata.timing
                self.seen.add(imdata.dbidx)
                if is_image_accepted(imdata):
                    self.accepted.add(imdata.dbidx)
                self.q.label_db.put(imdata.dbidx, imdata.boxes)
        delta_accepted = self.accepted - old_accepted
        delta_seen = self.seen - old_seen
        self._last_change = [(idx, 1 if idx in delta_accepted else 0) for idx in delta_seen.union(delta_accepted)]


class SessionGroup:
    """Several sessions driven in lock step: `next()` then `refine()` for all of them, with the work the sessions
    have in common done once.  The reference spreads sessions over Ray actors (`parallel_run`, `make_bench_actors`);
    here one process serves them, so a round's two halves are batched instead:

    * `next()`: the sessions whose loop would answer through `LoopBase._next_batch_curr_vec` (a `PointBased` loop, or
      any loop whose start policy has not fired) and that share one index object and the same `batch_size`,
      `shortlist_size`, `agg_method` and `aug_larger` are served by ONE `index.query_batch` -- one pass over the rows;
      a started `MultiRegNeg` whose `next_batch` is the class's own joins that group with `vector = curr_vec` and
      `vector2 = confusion_vec if discount_neg else zeros(dim)` (`query_batch(vectors2=...)`: one more launch for all
      of them); the started `ActiveSearch` / `LKNNSearch` loops whose model is on the device (`planning_groups`, from the
      `MIN_LKNN_GROUP` / `MIN_ACTIVE_SEARCH_GROUP` members on; `None` = never) plan through ONE `next_batch_group` -- one pass of kernels,
      one host wait -- before the other sessions; every other session calls its own `next()`.
    * `refine()`: every session's start-policy gate runs as in `LoopBase.refine_external`; the started `MultiReg`
      loops go through ONE `MultiReg.refine_batch` -- one launch, one host wait -- and the started `MultiRegNeg` loops
      whose options say `fit_on_device` through ONE `MultiRegNeg.refine_batch`, a launch of their own; the started
      `KnnProp2` loops of one index and shortlist size (`propagation_groups`, from `MIN_PROPAGATION_GROUP` members on)
      through ONE `KnnProp2.refine_batch` -- their propagations, scores and selections in one device call; every other
      loop, a `MultiRegNeg` that did not opt in included, through its own `refine_external`.  The batches refine
      first, the remaining sessions after them in session order: loops that draw from torch's global generator (every
      `MultiRegNeg` refine draws its start weights) keep the draws of the one-by-one order when the opted-in loops
      stand before the others in `sessions`.

    Every session ends each call in the state its own `next()` / `refine()` would have left: `returned`, `timing`
    (the shared call's time for each member), `acc_indices`, `acc_activations`, the log, `curr_vec` -- bit for bit.
    `prune` is passed on to `query_batch`."""

    def __init__(self, sessions, prune: bool = False):
        self.sessions = list(sessions)
        self.prune = bool(prune)

    # ---- which sessions go together ---------------------------------------------------------------------------
    @staticmethod
    def batch_vector(loop):
        """the vector `loop.next_batch_external()` would hand to `_next_batch_curr_vec`, or None when the loop
        answers another way"""
        from .loops.loop_base import LoopBase
        from .loops.point_based import PointBased
        cls = type(loop)
        if cls.next_batch_external is not LoopBase.next_batch_external or \
                cls._next_batch_curr_vec is not LoopBase._next_batch_curr_vec:
            return None
        if not loop.started:
            return loop.curr_qvec
        if isinstance(loop, PointBased) and cls.next_batch is PointBased.next_batch:
            return loop.curr_vec
        if SessionGroup._asks_with_two_vectors(loop):
            return loop.curr_vec  # with `batch_vector2`: the two-vector query
        return None

    @staticmethod
    def _asks_with_two_vectors(loop):
        """a started `MultiRegNeg` whose `next_batch` is the class's own and that carries what that method reads
        (`options`, `confusion_vec`: a loop made without `MultiRegNeg.__init__` has neither and answers on its own)"""
        from .loops.multi_reg_neg import MultiRegNeg
        return loop.started and isinstance(loop, MultiRegNeg) and type(loop).next_batch is MultiRegNeg.next_batch and \
            hasattr(loop, "confusion_vec") and getattr(loop, "options", None) is not None

    @staticmethod
    def batch_vector2(loop):
        """the `vector2` a started `MultiRegNeg.next_batch` asks with (None: the loop asks with one vector)"""
        if SessionGroup.batch_vector(loop) is None or not SessionGroup._asks_with_two_vectors(loop):
            return None
        return loop.confusion_vec if loop.options["discount_neg"] else np.zeros(loop.q.index.vectors.shape[1])

    def query_groups(self):
        """[(session positions, ...)]: the positions that share one `query_batch`, in session order; a session that
        answers on its own is a group of one"""
        groups, by_key = [], {}
        for i, s in enumerate(self.sessions):
            p = s.loop.params
            if self.batch_vector(s.loop) is None:
                groups.append([i])
                continue
            key = (id(s.loop.q.index), p.batch_size, p.shortlist_size, p.agg_method, p.aug_larger)
            if key not in by_key:
                by_key[key] = []
                groups.append(by_key[key])
            by_key[key].append(i)
        return [tuple(g) for g in groups]

    def fit_groups(self):
        """([positions that refine through one refine_batch, ...], [positions that refine on their own]), for loops
        that have started; the gate is `refine()`'s.  A group holds `MultiReg` loops, or `MultiRegNeg` loops that opted
        in with `fit_on_device` -- never both: the two objectives take launches of their own -- of one (dim, device)."""
        from .loops.loop_base import LoopBase
        from .loops.multi_reg import MultiReg
        from .loops.multi_reg_neg import MultiRegNeg
        batched, alone = {}, []
        for i, s in enumerate(self.sessions):
            loop = s.loop
            cls = type(loop)
            own_gate = cls.refine_external is LoopBase.refine_external and loop.started
            if isinstance(loop, MultiReg) and cls.refine is MultiReg.refine and own_gate:
                batched.setdefault((MultiReg, loop._engine.dim, loop._engine.device), []).append(i)
            elif isinstance(loop, MultiRegNeg) and cls.refine is MultiRegNeg.refine and own_gate and \
                    getattr(loop, "fit_on_device", False):
                batched.setdefault((MultiRegNeg, loop._engine.dim, loop._engine.device), []).append(i)
            else:
                alone.append(i)
        return [tuple(g) for g in batched.values()], alone

    # A group of graph loops goes through KnnProp2.refine_batch from this many members on.  Read from
    # profiles/round_batch_ab.txt (tools/perf_round_batch.py, 1.56 M nodes): per session-round the batched round takes
    # 87.4 [5.2] us against the loop's 105.9 [3.5] at 3 sessions -- ahead by more than both spreads -- and 105.9 [6.5]
    # against 108.7 [5.0] at 2, which is not.
    MIN_PROPAGATION_GROUP = 3

    def propagation_groups(self):
        """[(session positions, ...)]: the started `KnnProp2` loops that refine through one `KnnProp2.refine_batch`,
        grouped by (index object, shortlist_size), in session order.  A member's `refine` and `refine_external` are the
        class's own, its model `can_fuse_round()`, its index holds its rows on the device (`_dev`) and is not a subset
        view (the batched round, ssw_labelprop_round_batch, takes none); SSW_NO_FUSED_ROUND empties the list.  A `PseudoLR`'s inner graph loop is not
        a session's loop and stays on its own path.  Groups of one are listed too; `refine()` leaves them alone."""
        from .loops.graph_based import KnnProp2
        from .loops.loop_base import LoopBase
        if os.environ.get("SSW_NO_FUSED_ROUND"):
            return []
        by_key = {}
        for i, s in enumerate(self.sessions):
            loop = s.loop
            cls = type(loop)
            if not (isinstance(loop, KnnProp2) and loop.started and cls.refine is KnnProp2.refine and
                    cls.refine_external is LoopBase.refine_external):
                continue
            index = loop.q.index
            dev = getattr(index, "_dev", None)
            if dev is None or getattr(dev, "is_view", False) or getattr(index, "is_view", False) or \
                    not callable(getattr(index, "topk_after_update_batch", None)):
                continue
            model = getattr(getattr(loop, "state", None), "knn_model", None)
            if not getattr(model, "can_fuse_round", lambda: False)():
                continue
            by_key.setdefault((id(index), loop.params.shortlist_size), []).append(i)
        return [tuple(g) for g in by_key.values()]

    # A group of active-search loops plans through `next_batch_group` from this many members on; None: never.  Per loop
    # class, read from profiles/lknn_step_batch_ab.txt (tools/perf_lknn_batch.py): the smallest S at which the batch is
    # ahead of the loop of single calls by more than both interquartile ranges at EVERY measured graph size (3000, 50 000,
    # 200 000 and 1.56 M nodes; us per session-step, median [interquartile range], loop against batch).
    # lknn at 2 sessions: 77.0 [1.6] / 56.7 [1.9] at 3000 nodes, 78.3 [2.1] / 57.1 [1.6], 83.7 [1.1] / 57.6 [1.1] and
    # 97.3 [1.5] / 72.1 [1.8] at 1.56 M -- the launches and the wait shared; 102.0 / 40.3 at 16 sessions.
    MIN_LKNN_GROUP = 2
    # active_search (horizon 5) at 2 sessions: 116.5 [3.4] / 81.9 [6.4] at 3000 nodes, 141.9 [1.0] / 105.1 [3.2],
    # 233.1 [2.8] / 199.2 [3.0] and, at 1.56 M nodes, 1582.2 [3.3] / 1574.2 [7.3]: ahead by 8.0 against a spread of 7.3, the
    # narrowest case of the sweep -- there the look-ahead kernel is 1.44 of the 1.58 ms and takes S times as long for S
    # slots, so what the batch saves (8 us a step at 2 sessions, 19 at 4, 52 at 16) is the launches and the wait alone.
    MIN_ACTIVE_SEARCH_GROUP = 2

    def min_planning_group(self, loop):
        """the smallest group of `loop`'s class that `next()` serves through `next_batch_group` (None: none)"""
        from .loops.active_search import LKNNSearch
        return self.MIN_LKNN_GROUP if type(loop) is LKNNSearch else self.MIN_ACTIVE_SEARCH_GROUP

    def planning_groups(self):
        """[(session positions, ...)]: the started loops that are exactly an `ActiveSearch` or an `LKNNSearch`, whose
        `next_batch` and `next_batch_external` are the class's own and whose `prob_model` is a `DeviceLKNNModel`, grouped
        by (class, device, node count, degree) in session order -- what one `next_batch_group` can serve.  Groups of one
        are listed too; `next()` serves a group from `min_planning_group` members on."""
        from .loops.active_search import ActiveSearch, LKNNSearch
        from .loops.LKNN_model import DeviceLKNNModel
        from .loops.loop_base import LoopBase
        by_key = {}
        for i, s in enumerate(self.sessions):
            loop = s.loop
            cls = type(loop)
            if cls not in (ActiveSearch, LKNNSearch) or not loop.started or \
                    cls.next_batch_external is not LoopBase.next_batch_external:
                continue
            model = getattr(loop, "prob_model", None)
            if not isinstance(model, DeviceLKNNModel):
                continue
            by_key.setdefault((cls, model.device, model.n, model.degree), []).append(i)
        return [tuple(g) for g in by_key.values()]

    def _next_planned(self, group, out):
        """one `next_batch_group` for the sessions of `group`, with `Session.next`'s bookkeeping for each"""
        members = [self.sessions[i] for i in group]
        for s in members:
            s._log("next.start")
            print("start met. next batch from custom method...")
        start = time.time()
        results = type(members[0].loop).next_batch_group([s.loop for s in members])
        elapsed = time.time() - start
        for i, s, r in zip(group, members, results):
            s.timing.append(elapsed)
            s.acc_indices.append(r["dbidxs"])
            s.acc_activations.append(r["activations"])
            s._log("next.end")
            out[i] = r["dbidxs"]

    # ---- the two halves of a round ----------------------------------------------------------------------------
    def next(self):
        """`[s.next() for s in sessions]`"""
        out = [None] * len(self.sessions)
        planned = set()
        for group in self.planning_groups():
            least = self.min_planning_group(self.sessions[group[0]].loop)
            if least is not None and len(group) >= max(2, least):
                self._next_planned(group, out)
                planned.update(group)
        for group in self.query_groups():
            if len(group) == 1:
                if group[0] in planned:
                    continue
                out[group[0]] = self.sessions[group[0]].next()
                continue
            members = [self.sessions[i] for i in group]
            vectors, vectors2 = [], []
            for s in members:
                s._log("next.start")
                print("start met. next batch from custom method..." if s.loop.started
                      else "start not yet met. next batch using default...")
                vec = self.batch_vector(s.loop)
                vec2 = self.batch_vector2(s.loop)
                if vec2 is None:  # (`_next_batch_curr_vec`'s check; `MultiRegNeg.next_batch` has none)
                    assert not np.isnan(vec).any(), f"NaN in query vector {vec=}"
                vectors.append(vec)
                vectors2.append(vec2)
            start = time.time()
            p = members[0].loop.params
            pair = {"vectors2": vectors2} if any(v2 is not None for v2 in vectors2) else {}
            results = members[0].loop.q.index.query_batch(
                topk=p.batch_size, vectors=vectors, excludes=[s.loop.q.returned for s in members], prune=self.prune,
                shortlist_size=p.shortlist_size, agg_method=p.agg_method, aug_larger=p.aug_larger, **pair)
            elapsed = time.time() - start
            for i, s, r in zip(group, members, results):
                s.loop.q.returned.update(np.asarray(r["dbidxs"], dtype=np.int64))
                s.timing.append(elapsed)
                s.acc_indices.append(r["dbidxs"])
                s.acc_activations.append(r["activations"])
                s._log("next.end")
                out[i] = r["dbidxs"]
        return out

    def refine(self):
        """`for s in sessions: s.refine()`"""
        from .loops.graph_based import KnnProp2
        from .loops.multi_reg import MultiReg
        from .loops.multi_reg_neg import MultiRegNeg
        for s in self.sessions:  # the gate of LoopBase.refine_external
            if not s.loop.started and (isinstance(s.loop, (MultiReg, KnnProp2)) or
                                       (isinstance(s.loop, MultiRegNeg) and getattr(s.loop, "fit_on_device", False))):
                s.loop.started = s.loop._start_condition()
        batched, alone = self.fit_groups()
        for group in self.propagation_groups():  # graph loops of one index: one batched round, from the minimum size on
            if len(group) >= max(2, self.MIN_PROPAGATION_GROUP):
                batched.append(group)
                alone = [i for i in alone if i not in group]
        for group in batched:
            members = [self.sessions[i] for i in group]
            if len(members) == 1:
                alone.append(group[0])
                continue
            for s in members:
                s._log("refine.start")
                print("start condition met... refinining custom method...")
            type(members[0].loop).refine_batch([s.loop for s in members])
            for s in members:
                s._log("refine.end")
        for i in sorted(alone):
            self.sessions[i].refine()


def make_session(gdm, p: SessionParams, b: BenchParams = None):
    ds = gdm.get_dataset(p.index_spec.d_name)
    if p.index_spec.c_name is not None:
        ds = ds.load_subset(p.index_spec.c_name)
    _y = None
    if p.pass_ground_truth:
        _, gt = ds.load_ground_truth()
        _y = gt[b.ground_truth_category]
    idx = ds.load_index(p.index_spec.i_name, options=p.index_options)
    session = Session(gdm, ds, idx, p, _y=_y)
    return {"session": session, "dataset": ds}
