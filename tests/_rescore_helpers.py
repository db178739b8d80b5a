"""Seeded tile layouts for the `avg_score` aggregation at the edges of its kernel (csrc/rescore.hip), shared by the golden
generator (oracle/gen_golden.py, family `avg_score_edges`), tests/test_rescore_edges_cpu.py and tests/test_rescore_edges_gpu.py.

One image per tile count in TILE_COUNTS (the kernel has 256 threads and keeps at most 2048 tiles in LDS) plus one image of
8 zero-area tiles.  Box corners are multiples of 16 and sides come from {32, 64, 128, 224}: areas, intersections and unions
are small integers, exact in f32, so equal IoUs are exactly equal.  Zoom levels come from a per-image set cycling over
LEVEL_SETS (level 31 is the top bit of the kernel's presence mask).

Every image of at least 8 tiles carries, among its random tiles (x <= 400):
  * one zero-area box (IoU with itself 0/0: no partner, aggregate NaN);
  * tile 0's box once more on tile 0's level and once on another level of the set (equal IoUs: the first maximum wins);
  * two tiles with the same score;
and, in the strip x in [416, 480] that no random tile reaches, a group of identical boxes that holds the image's best tile:
  a0 (first level, score H) and a1 (first level, a small score): both aggregate to a0's value -- the FIRST maximum of equal
  IoUs picks a0's score, and the FIRST of equal aggregates is a0;  a2 (second level, if the set has one);  with three levels
  a2 / a3 carry +B / -B with B = 2**25 (2**54 for f64 scores) and H = 1001, for which the Kahan sum in ascending level
  order (H, B, -B) differs from the descending one.
The group sits at indexes >= 256 in the images of 257, 513 and 2048 tiles (the 257-tile image has room for a0 only), so the
second trip of the kernel's 256-thread loops decides the answer.

`loaded=True` gives the scores for the entries that take scores as they are (load_scores, the f64 tensor): also one NaN,
one +inf and one -inf.  NaN goes to a2 where the set has exactly two levels (pandas' group mean skips it), +inf to a0 in the
three-level images and in the three large ones (pandas resets the Kahan compensation after an infinity), the rest to random
tiles.
"""
import numpy as np

SEED = 20261
DIM = 256
TILE_COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1024, 2047, 2048]
LEVEL_SETS = [(0,), (31,), (0, 31), (0, 1, 2), (3, 4), (0, 5, 31), (0, 1, 2, 7, 31)]
SIDES = np.array([32, 64, 128, 224])
BEST_PAST_256 = (257, 513, 2048)   # tile counts whose best tile must sit at an index >= 256
N_ALL_NAN = 8                      # tiles of the last image: all zero-area, every aggregate NaN
AUGS = ("all", "greater", "adjacent")
STRIP_BOX = np.float32([416, 0, 480, 64])
H_SCORE = 1001.0


def big_score(dtype):
    return 2.0 ** 25 if np.dtype(dtype) == np.float32 else 2.0 ** 54


class Layout:
    """row2image int32 [n], boxes f32 [n, 4], zoom int32 [n], row_start int64 [n_images + 1], per image the level set and
    the rows of its planted tiles (`plants[p]`: dict name -> row inside the image)"""

    def __init__(self, tile_counts=TILE_COUNTS, seed=SEED, all_nan_image=True):
        rng = np.random.default_rng(seed)
        counts = list(tile_counts) + ([N_ALL_NAN] if all_nan_image else [])
        self.tile_counts = counts
        self.n_images = len(counts)
        self.all_nan_position = len(counts) - 1 if all_nan_image else None
        self.row_start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        self.n_rows = int(self.row_start[-1])
        self.row2image = np.repeat(np.arange(self.n_images), counts).astype(np.int32)
        self.boxes = np.zeros((self.n_rows, 4), dtype=np.float32)
        self.zoom = np.zeros(self.n_rows, dtype=np.int32)
        self.level_sets, self.plants = [], []
        self._base = rng.uniform(-1.0, 1.0, self.n_rows)  # f64 draws: rounded per dtype in scores()
        for p, T in enumerate(counts):
            levels = LEVEL_SETS[p % len(LEVEL_SETS)]
            self.level_sets.append(levels)
            r0 = int(self.row_start[p])
            w, h = rng.choice(SIDES, T), rng.choice(SIDES, T)
            x1 = 16 * rng.integers(0, (400 - w) // 16 + 1)
            y1 = 16 * rng.integers(0, (624 - h) // 16 + 1)
            b = np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(np.float32)
            z = np.asarray(levels)[rng.integers(0, len(levels), T)].astype(np.int32)
            z[:min(T, len(levels))] = levels[:min(T, len(levels))]  # every level of the set occurs (T permitting)
            plants = {}
            if p == self.all_nan_position:
                b[:, 2], b[:, 3] = b[:, 0], b[:, 1]
            elif T >= 8:
                group = 2 + min(len(levels) - 1, 2)          # a0, a1 (+ a2 (+ a3))
                if T in BEST_PAST_256:
                    a0 = max(256, T - group)
                    group = min(group, T - a0)
                else:
                    a0 = int(rng.integers(4, T - group + 1))
                strip = list(range(a0, a0 + group))
                free = [i for i in range(1, T) if i not in strip]
                assert len(free) >= 7, "an image with plants needs 7 rows outside the strip besides tile 0"
                picks = [int(i) for i in rng.choice(free, 7, replace=False)]
                names = ["zero_area", "dup_same_level", "dup_other_level", "tie_a", "tie_b", "nan", "neg_inf"]
                plants = dict(zip(names, picks))
                b[plants["zero_area"], 2] = b[plants["zero_area"], 0]
                b[plants["dup_same_level"]] = b[0]
                z[plants["dup_same_level"]] = z[0]
                b[plants["dup_other_level"]] = b[0]
                z[plants["dup_other_level"]] = levels[1] if len(levels) > 1 else levels[0]
                b[strip] = STRIP_BOX
                z[strip] = [levels[0], levels[0], *levels[1:3]][:group]
                plants["strip"] = strip
            self.boxes[r0:r0 + T], self.zoom[r0:r0 + T] = b, z
            self.plants.append(plants)
        self._inf_free = [int(i) for i in rng.integers(1, 1 << 30, self.n_images)]

    def rows(self, p):
        return slice(int(self.row_start[p]), int(self.row_start[p + 1]))

    def scores(self, dtype=np.float32, loaded=False):
        """one score per row in `dtype`; f64 scores are not f32 values (the f64 entry must not get away with f32 sums)"""
        dt = np.dtype(dtype)
        s = self._base.astype(np.float32).astype(np.float64)
        if dt == np.float64:
            s = s + self._base * 2.0 ** -30
        s = s.astype(dt)
        B = big_score(dt)
        for p, T in enumerate(self.tile_counts):
            pl = self.plants[p]
            if not pl:
                continue
            r0 = int(self.row_start[p])
            s[r0 + pl["tie_b"]] = s[r0 + pl["tie_a"]]
            strip, n_levels = pl["strip"], len(self.level_sets[p])
            s[r0 + strip[0]] = H_SCORE
            if n_levels >= 3 and len(strip) == 4:
                s[r0 + strip[2]], s[r0 + strip[3]] = B, -B
            if loaded:
                nan_at = strip[2] if n_levels == 2 and len(strip) > 2 else pl.get("nan")
                if nan_at is not None:
                    s[r0 + nan_at] = np.nan
                if "neg_inf" in pl:
                    s[r0 + pl["neg_inf"]] = -np.inf
                if n_levels >= 3 or T in BEST_PAST_256:
                    s[r0 + strip[0]] = np.inf
                else:  # a random tile outside the strip and the other plants
                    taken = set(strip) | {v for k, v in pl.items() if k != "strip"}
                    free = [i for i in range(T) if i not in taken]
                    s[r0 + free[self._inf_free[p] % len(free)]] = np.inf
        return s

    def minus(self):
        """a seeded `minus` vector: one f32 value per row (the vector2 form of the query subtracts it from the score)"""
        return np.random.default_rng(SEED + 1).uniform(-0.5, 0.5, self.n_rows).astype(np.float32)

    def vectors(self):
        """index rows s_i * e_0 for the finite f32 scores: against a query c * e_0 (c a power of two) the scan's dot
        product is s_i * c exactly, whatever its summation order"""
        X = np.zeros((self.n_rows, DIM), dtype=np.float32)
        X[:, 0] = self.scores(np.float32)
        return X

    @staticmethod
    def query(c=1.0):
        q = np.zeros(DIM, dtype=np.float32)
        q[0] = c
        return q


def cont_weighted_bound(P, A):
    """|f32-weight kernel - float64 reference| for one tile of P partners, A = sum_j w_ij |s_j|: every weight carries the
    rounding of expf's argument and result, one division and the P-term f32 sum `esum` (P + 3 roundings, padded to
    P + 8), the weighted sum adds P more: (2P + 8) * 2**-24 * A"""
    return (2.0 * np.asarray(P, dtype=np.float64) + 8.0) * 2.0 ** -24 * np.asarray(A, dtype=np.float64)
