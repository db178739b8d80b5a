"""Shared by the chunk-selection tests (test_chunk_select_gpu.py, test_chunk_select_edges_cpu.py / _gpu.py): the numpy
reference and the on / off driver, a numpy restatement of the selection's key and of what the chunk form must do with
a slot (`plan`, `route`, `predict` -- written from the comment block above k_chunk_level1 in select.hip, never by
calling the library), and the crafted cases both edge files iterate over.

Crafted slabs: rows that are zero except ONE column, queried with that column's unit vector, score bit for bit the
column's value (one product by 1.0 plus exact zeros).  Without an image map a case is a section of the parent and a
view of it (its own block of rows plus a shared pool of low "filler" rows); with a map a case is a column of an index
whose images have 1, 8, 9, 16 and 17 rows.  Every crafted value is positive and binary16-representable unless the case
says otherwise, so one table serves both dtypes; a 12-bit bin holds only 128 distinct binary16 values, so the counts are
reached with repeated values -- ties, which is wanted.  -0.0 is never crafted: numpy orders it equal to +0.0, the key
does not."""
import numpy as np

DIM = 256
STATS = ("chunks", "slots", "second_level", "per_slot", "deep_reruns", "launches")


def _reference(scores, row_start, excluded, k):
    """per-image maximum (lowest row on ties), excluded images removed, (score descending, image ascending), first k"""
    n_images = row_start.shape[0] - 1
    best = np.maximum.reduceat(scores, row_start[:-1])
    image = np.repeat(np.arange(n_images), np.diff(row_start))
    rows = np.minimum.reduceat(np.where(scores == best[image], np.arange(scores.shape[0]), scores.shape[0]), row_start[:-1])
    keep = np.ones(n_images, dtype=bool)
    keep[np.asarray(excluded, dtype=np.int64)] = False
    ids = np.nonzero(keep)[0]
    ids = ids[np.lexsort((ids, -best[ids].astype(np.float64)))][:k]
    return ids, best[ids], rows[ids]


def _same(got, want, where):
    assert len(got) == len(want), where
    for s, (g, w) in enumerate(zip(got, want)):
        for a, b in zip(g, w):
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape, (where, s, "count")
            assert a.tobytes() == b.tobytes(), (where, s)


def _index(rng, n_images, tiles, has_map, dtype, X=None):
    from seesaw_amd.device_index import DeviceIndex
    counts = np.full(n_images, tiles[0]) if tiles[0] == tiles[1] else rng.integers(tiles[0], tiles[1] + 1, n_images)
    n = int(counts.sum())
    if X is None:
        X = rng.standard_normal((n, DIM)).astype(np.float32)
    row2image = np.repeat(np.arange(n_images, dtype=np.int32), counts)
    idx = DeviceIndex.from_numpy(X, row2image=row2image if has_map else None, dtype=dtype)
    row_start = np.concatenate(([0], np.cumsum(counts))) if has_map else np.arange(n + 1)
    return idx, row_start


def _on_off(idx, call):
    """`call()` with the setting off, then on: (off, on, the counters' change over the on call)"""
    idx.chunk_select = False
    off = call()
    idx.chunk_select = True
    before = idx.chunk_select_stats()
    on = call()
    after = idx.chunk_select_stats()
    return off, on, {key: after[key] - before[key] for key in STATS}


# ---- the selection's key and the chunk form's rule, restated ---------------------------------------------------------
NBINS, LEVEL2_FROM, FINAL_CAP, SMALL_IMAGES, RANK_MAX, CHUNK_SLOTS = 4096, 1024, 8192, 8192, 4096, 16


def ord_key(s):
    """f32_to_ord (ssw_common.h): sign set gives ~u, otherwise u | 0x80000000 -- ascending keys, ascending floats"""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where((u & np.uint32(0x80000000)) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def bin1(s):
    return ord_key(s) >> np.uint32(20)


def bin2(s):
    return (ord_key(s) >> np.uint32(8)) & np.uint32(0xfff)


def _pick(bins, kk):
    """the bin that holds rank kk counted from the top bin downwards: (bin, keys above it, keys in it); with fewer than
    kk keys in all, bin 0 and everything above it"""
    h = np.bincount(np.asarray(bins, dtype=np.int64), minlength=NBINS)
    if h.sum() < kk:
        return 0, int(h.sum() - h[0]), int(h[0])
    cum = np.cumsum(h[::-1])
    top = int(np.searchsorted(cum, kk))
    b = NBINS - 1 - top
    return b, int(cum[top] - h[b]), int(h[b])


def plan(scores_per_image, excluded, k):
    """what the general chunk form does with a slot, from its per-image scores alone: the histograms count EVERY image
    (exclusions never reach them), level 1 picks the 12-bit bin of rank kk = k + distinct excluded ids, level 2 runs
    where more than LEVEL2_FROM keys lie at or above that bin and picks rank kk - above1 of the next 12 bits inside it,
    and the slot overflows into the deep rerun where more than FINAL_CAP keys lie at or above the 24-bit prefix"""
    s = np.ascontiguousarray(scores_per_image, dtype=np.float32)
    kk = int(k) + len(set(int(e) for e in excluded))
    b1, above1, cnt1 = _pick(bin1(s), kk)
    out = dict(kk=kk, b1=b1, at_or_above1=above1 + cnt1, level2=above1 + cnt1 > LEVEL2_FROM, b2=None, total2=None,
               overflow=False)
    if out["level2"]:
        b2, above2, cnt2 = _pick(bin2(s[bin1(s) == b1]), kk - above1)
        out.update(b2=b2, total2=above1 + above2 + cnt2, overflow=above1 + above2 + cnt2 > FINAL_CAP)
    return out


def route(n_images, excluded, k):
    """"small": at most 8192 images and at most 8192 ids as given -- one launch; "general": more images and at most
    4096 - k DISTINCT ids; "per_slot": everything else goes to the per-slot selection"""
    if n_images <= SMALL_IMAGES:
        return "small" if len(excluded) <= SMALL_IMAGES else "per_slot"
    return "general" if len(set(int(e) for e in excluded)) <= RANK_MAX - k else "per_slot"


def predict(slots):
    """the change of chunk_select_stats over one batched call: slots = [(scores per image, excluded, k), ...]"""
    d = dict.fromkeys(STATS, 0)
    for c0 in range(0, len(slots), CHUNK_SLOTS):
        chunk = slots[c0:c0 + CHUNK_SLOTS]
        forms = [route(len(s), e, k) for s, e, k in chunk]
        taken = [f for f in forms if f != "per_slot"]
        d["per_slot"] += len(forms) - len(taken)
        if taken:
            d["chunks"] += 1
            d["slots"] += len(taken)
            d["launches"] += 4 if "general" in taken else 1
        for (s, e, k), f in zip(chunk, forms):
            if f == "general":
                p = plan(s, e, k)
                d["second_level"] += int(p["level2"])
                d["deep_reruns"] += int(p["overflow"])
    return d


# ---- crafted values ----------------------------------------------------------------------------------------------------
B_ONE = 0xbf8       # the level-1 bin [1, 1.125): 1.0 is its lowest key
B_HIGH = 0xc00      # [2, 2.25)
B_LADDER = 0xc30    # [128, 144): where the long ladders start
FILL_TOP = 0xbdf    # the fillers lie below 0.125: bins 0xbdf downwards, binary16 normals all of them
POOL = 9000         # filler values a view can draw on: the upper half ahead of its block, the lower half behind it


def key_value(b1, b2=0, low=0):
    """the positive f32 whose key has level-1 bin b1 (>= 0x800), level-2 bin b2 and low byte `low`"""
    u = ((np.asarray(b1, dtype=np.uint32) & np.uint32(0x7ff)) << np.uint32(20)) | \
        (np.asarray(b2, dtype=np.uint32) << np.uint32(8)) | np.asarray(low, dtype=np.uint32)
    return np.atleast_1d(u.astype(np.uint32)).view(np.float32)


def ladder(count, top_b1, half=True, start=0):
    """entries start .. start + count of a strictly descending ladder that fills bin top_b1, then the next lower one,
    ...: 128 binary16-representable values a bin (half), else 1024 with low mantissa bits set.  The last value of a bin
    is the bin's edge itself (level-2 bin 0, low byte 0)."""
    cap = 128 if half else 1024
    j = np.arange(start, start + count, dtype=np.int64)
    sub = cap - 1 - j % cap
    return key_value(top_b1 - j // cap, sub * (NBINS // cap), 0 if half else (sub * 97) & 0xff)


def in_bin(b1, count, half=True):
    """count descending values inside ONE level-1 bin, none on its edge: distinct while the bin has room (127 values in
    binary16, 4095 level-2 bins in f32), repeated beyond that"""
    cap = 127 if half else 4095
    i = (np.arange(count, dtype=np.int64) * min(cap, count)) // count
    sub = cap - i
    return key_value(b1, sub * (32 if half else 1), 0 if half else (sub * 97) & 0xff)


def fillers(count):
    return ladder(count, FILL_TOP, half=True)


def best_ids(values, m):
    """the m best images of per-image values: (value descending, image ascending)"""
    values = np.asarray(values)
    return np.lexsort((np.arange(values.shape[0]), -values.astype(np.float64)))[:m]


MAP_COUNTS = (1, 8, 9, 16, 17)  # the `r += 8` loop's edges: one row, one full group, one over, two groups, one over


def map_rows(values):
    """per-image values -> (row values, row_start) of the mapped layout: image i has MAP_COUNTS[i % 5] rows, zero except
    its value in its LAST row and, from two rows on, once more in row c // 2 -- the lowest row must win"""
    values = np.asarray(values, dtype=np.float32)
    assert (values > 0).all(), "the other rows are zero: a mapped case is positive"
    counts = np.asarray(MAP_COUNTS)[np.arange(values.shape[0]) % len(MAP_COUNTS)]
    row_start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    rows = np.zeros(int(row_start[-1]), dtype=np.float32)
    rows[row_start[1:] - 1] = values
    rows[row_start[:-1] + counts // 2] = values
    return rows, row_start


class Case:
    """one slot: `top`, the block of crafted per-image values, with fillers around it up to n images (own: the block is
    the whole slot), selected with k and `excluded`; `sign` -1 queries with the negated unit vector"""

    def __init__(self, name, top, n, k, excluded=(), own=False, sign=1.0, **facts):
        self.name, self.top, self.k, self.own, self.sign = name, np.ascontiguousarray(top, dtype=np.float32), int(k), own, sign
        self.n = self.top.shape[0] if own else int(n)
        self.excluded = [int(e) for e in excluded]
        self.facts = facts
        assert self.n >= self.top.shape[0] and self.n - self.top.shape[0] <= POOL

    def ahead(self):
        return 0 if self.own else (self.n - self.top.shape[0]) // 2

    def behind(self):
        return 0 if self.own else self.n - self.top.shape[0] - self.ahead()

    def stored(self):
        """the per-image values as the parent stores them, in the slot's image order"""
        f = fillers(POOL)
        return np.concatenate((f[:self.ahead()], self.top, f[POOL // 2:POOL // 2 + self.behind()]))

    def values(self):
        """the per-image scores of the slot (sign * stored: exact)"""
        return (np.float32(self.sign) * self.stored()).astype(np.float32)

    def slot(self):
        return self.values(), self.excluded, self.k

    def __repr__(self):
        return self.name


def _shuffled(rng, *parts):
    v = np.concatenate([np.asarray(p, dtype=np.float32) for p in parts])
    return v[rng.permutation(v.shape[0])]


def tight_rank_cases(half, n=None):
    """excluded = exactly the best n_excl images, so the k-th survivor has overall rank kk = k + n_excl; `edge`: rank kk
    is the last key of its bin (the bin's edge value), rank kk + 1 the first of the next lower bin; "first": rank kk is
    the first key of its bin and rank kk - 1 the last of the bin above, where a pick one rank short loses the image"""
    rng, out, cap = np.random.default_rng(101), [], 128 if half else 1024
    for k in (1, 64, 65):
        for n_excl in (1, 100, RANK_MAX - k):
            for edge in (False, True, "first"):
                if edge == "first" and n_excl == RANK_MAX - k:
                    continue  # (two edges of the largest blocks fill the parent)
                kk = k + n_excl
                start = {False: cap // 2 - kk, True: -kk, "first": 1 - kk}[edge] % cap
                c = Case(f"tight k={k} n_excl={n_excl} edge={edge}", _shuffled(rng, ladder(kk + 40, B_LADDER, half, start)),
                         n or 8193 + kk % 4, k, edge=edge, n_excl=n_excl)
                order = best_ids(c.values(), kk)
                c.excluded, c.facts["want"] = order[:n_excl].tolist(), order[n_excl:]
                out.append(c)
    return out


def excl_cap_cases():
    """one block, k = 64, 4095, 4096: exactly 4096 - k distinct ids (the best ones: the rank bound is tight as well), one
    more, and the 4096 - k with 50 duplicates shuffled in"""
    rng, out = np.random.default_rng(102), []
    top = _shuffled(rng, ladder(4300, B_LADDER, True))
    for k in (64, 4095, 4096):
        cap = RANK_MAX - k
        base = Case("", top, 8200, k)
        order = best_ids(base.values(), cap + 1)
        out.append(Case(f"cap k={k} on", top, 8200, k, order[:cap], form="general"))
        out.append(Case(f"cap k={k} past", top, 8200, k, order[:cap + 1], form="per_slot"))
        if cap > 0:
            ids = np.concatenate((order[:cap], rng.choice(order[:cap], size=50)))
            out.append(Case(f"cap k={k} duplicates", top, 8200, k, ids[rng.permutation(ids.shape[0])], form="general"))
    return out


def level2_cases(half):
    """1024 and 1025 keys at or above the picked bin (10 above it), without exclusions and with 10 inside the bin"""
    rng, out = np.random.default_rng(103), []
    for total in (1024, 1025):
        top = _shuffled(rng, ladder(10, B_HIGH, half), in_bin(B_ONE, total - 10, half))
        base = Case("", top, 8193 + total % 4, 64)
        inside = best_ids(base.values(), 40)[30:]
        for excluded in ([], inside.tolist()):
            out.append(Case(f"level2 total={total} n_excl={len(excluded)}", top, base.n, 64, excluded, total=total))
    return out


def final_cap_cases(half, n=None):
    """8192 and 8193 keys in the 24-bit prefix of the cut: one tie group at 1.0 alone, or 100 distinct higher scores (50
    in a higher level-1 bin, 50 in higher level-2 bins of the tie's) and the group; the `alone` shape also with the 5
    lowest-numbered members excluded.  k = 128, so the cut lies inside the group.  Last: a slot that does not overflow."""
    rng, out = np.random.default_rng(104), []
    for total in (8192, 8193):
        alone = np.full(total, 1.0, dtype=np.float32)
        higher = _shuffled(rng, ladder(50, B_HIGH, half), in_bin(B_ONE, 50, half), np.full(total - 100, 1.0, dtype=np.float32))
        for shape, top, n_excl in (("alone", alone, 0), ("higher", higher, 0), ("alone", alone, 5)):
            c = Case(f"final total={total} {shape} n_excl={n_excl}", top, n or total + 8, 128, total=total)
            c.excluded = np.nonzero(c.values() == np.float32(1.0))[0][:n_excl].tolist()
            out.append(c)
    out.append(Case("final neighbour", _shuffled(rng, ladder(200, B_LADDER, half)), n or 8193, 128, total=None))
    return out


TIE_GROUP = 40


def tie_cases(half, n=None):
    """k = 64: a group of 40 equal scores of which every third member (by image) is excluded, 26 are left.  Behind 34
    distinct higher scores the group holds the raw ranks 35 .. 74, 30 of them above the cut, and all 26 come out; behind
    40 higher scores 24 of the 26 come out and 2 do not -- the group straddles the cut among the images that count.
    Each with nothing else in the group's level-1 bin (level 1 only) and with 1500 lower scores beside it (level 2)."""
    rng, out = np.random.default_rng(105), []
    tie = key_value(B_ONE, 64 << 5)[0]
    for higher in (34, 40):
        for level2 in (False, True):
            lower = key_value(B_ONE, (np.arange(1500) % 64) << 5) if level2 else np.zeros(0, dtype=np.float32)
            top = _shuffled(rng, ladder(higher, B_HIGH, half), np.full(TIE_GROUP, tie), lower)
            c = Case(f"ties higher={higher} level2={level2}", top, n or 8194, 64, level2=level2, tie=tie, higher=higher)
            v = c.values()
            group = np.nonzero(v == tie)[0]
            c.excluded = group[::3].tolist()
            left = np.setdiff1d(group, group[::3])
            below = np.nonzero(v < tie)[0]
            c.facts["want"] = np.concatenate((best_ids(v, higher), left, below[best_ids(v[below], 64)]))[:64]
            out.append(c)
    return out


def key_edge_cases():
    """k = 50, float32: an all-negative slot; 40 positive scores, +0.0 and negative ones (the cut lies below zero);
    30 normal scores above 8165 distinct subnormal ones; 2^-j and the float just under it, j = 0 .. 6, among fillers"""
    rng = np.random.default_rng(106)
    body = np.concatenate((ladder(4000, B_LADDER, False), fillers(4152)))
    powers = np.float32(2.0) ** -np.arange(7, dtype=np.float32)
    subnormal = (1000 + 500 * np.arange(8165)).astype(np.uint32).view(np.float32)
    return [Case("keys negative", _shuffled(rng, -body, -fillers(POOL)[4152:4193]), 0, 50, own=True),
            Case("keys around zero", _shuffled(rng, ladder(40, B_HIGH, False), [0.0], -body), 0, 50, own=True),
            Case("keys subnormal", _shuffled(rng, ladder(30, B_HIGH, False), subnormal), 0, 50, own=True),
            Case("keys powers of two", _shuffled(rng, powers, np.nextafter(powers, np.float32(0.0))), 8194, 50)]


def tail_cases():
    """8193 .. 8196 images without a map (n % 4 = 1, 2, 3, 0), k = 64: the best image is the last one, the 64th best the
    one before it, the 63rd the one before that"""
    rng, out = np.random.default_rng(107), []
    for n in (8193, 8194, 8195, 8196):
        v = _shuffled(rng, ladder(4000, B_LADDER, False), fillers(n - 4000))
        order = best_ids(v, 64)
        for rank, pos in ((0, n - 1), (63, n - 2), (62, n - 3)):
            at = int(np.nonzero(v == v[order[rank]])[0][0])
            v[[at, pos]] = v[[pos, at]]
        out.append(Case(f"tail n={n}", v, 0, 64, own=True))
    return out


def small_cases():
    """the small form, k = 64: every image of 64 excluded (count 0); all but three of 8192 excluded, the ids shuffled
    and three of them twice (8192 ids as given); 1000 images and no exclusion"""
    rng = np.random.default_rng(108)
    kept = rng.choice(8192, size=3, replace=False)
    ids = np.setdiff1d(np.arange(8192), kept)
    ids = np.concatenate((ids, ids[:3]))
    return [Case("small nothing left", _shuffled(rng, fillers(64)), 0, 64, range(64), own=True, count=0),
            Case("small three left", _shuffled(rng, fillers(8192)), 0, 64, ids[rng.permutation(8192)], own=True, count=3),
            Case("small plain", _shuffled(rng, fillers(1000)), 0, 64, own=True, count=64)]


def sequence_calls():
    """one view, many chunks: 12 000 images whose scores are plain at k = 5 (ten powers of two on top), take level 2 at
    k = 64 (2000 scores spread over [0.875, 1)) and, queried with the negated unit vector, overflow (8200 images at
    -1.0 come out on top).  -> [(what, [Case, ...])], the cases of a call sharing k; run twice on one handle."""
    rng = np.random.default_rng(109)
    top = _shuffled(rng, np.float32(2.0) ** np.arange(1, 11, dtype=np.float32), in_bin(0xbf6, 2000, False), fillers(1790),
                    np.full(8200, -1.0, dtype=np.float32))

    def case(kind, k, excluded=()):
        return Case(f"sequence {kind} k={k} n_excl={len(excluded)}", top, 0, k, excluded, own=True,
                    sign=-1.0 if kind == "overflow" else 1.0, kind=kind)

    many = rng.choice(12000, size=RANK_MAX - 64 + 1, replace=False)
    return [("plain", [case("plain", 5), case("plain", 5, [3, 4])]),
            ("level 2", [case("level2", 64), case("level2", 64, [7])]),
            ("one overflows", [case("overflow", 64, [1, 2]), case("level2", 64)]),
            ("plain again", [case("plain", 5, [9]), case("plain", 5)]),
            ("16 slots", [case("overflow" if s % 5 == 4 else "plain", 5, range(s % 5)) for s in range(16)]),
            ("one past the cap", [case("level2", 64), case("overflow", 64), case("per_slot", 64, many)]),
            ("plain at last", [case("plain", 5), case("plain", 5, [11])])]


MASKED_N, MASKED_FINITE = 8200, 30


def masked_labels(n=MASKED_N, finite=MASKED_FINITE):
    """the graph round's mask: every node but `finite` of n is labelled -> (labelled ids, the others), both ascending"""
    free = np.sort(np.random.default_rng(110).choice(n, size=finite, replace=False))
    return np.setdiff1d(np.arange(n), free), free


def masked_case(prior=None):
    """fewer than k finite, k = 50: a slot of 8200 images (one tile an image) whose labelled nodes score -inf -- real,
    nonzero keys (0x007fffff) that tie by image id; 30 finite scores (the prior's, uniform in (0.05, 0.95) here)"""
    labelled, free = masked_labels()
    if prior is None:
        prior = np.random.default_rng(111).uniform(0.05, 0.95, MASKED_N)
    v = np.asarray(prior, dtype=np.float64).astype(np.float32)
    v[labelled] = -np.inf
    return Case("masked all but 30", v, 0, 50, own=True, labelled=labelled, free=free)
