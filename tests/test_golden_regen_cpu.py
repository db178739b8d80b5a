"""CPU: the committed generator of tests/golden/ and the committed fixtures name the same FIFTEEN families.

The fixtures themselves are regenerated from the reference with `python oracle/gen_golden.py --check` (all light
families; name `c5_sequence` for the heavy one), which needs a checkout of the reference beside the build and fails
on any byte of any array that differs.  That regeneration is a maintenance step, not part of the suite: the suite
runs on the committed fixtures alone."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIGHT = ("tiling", "sliding", "lknn", "scan_topk", "multiscale_query", "labelprop", "rank_loss", "logreg", "multireg", "bench_loop",
         "multiregneg", "contweighted", "multireg_det", "avg_score_edges")
HEAVY = ("c5_sequence",)


def test_the_generator_knows_exactly_these_families():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    try:
        import gen_golden
    finally:
        sys.path.pop(0)
    assert set(gen_golden.FAMILIES) == set(LIGHT) | set(HEAVY) and set(gen_golden.HEAVY) == set(HEAVY)
    have = {f[:-4] for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f.endswith(".npz")}
    assert set(LIGHT) | set(HEAVY) <= have, sorted((set(LIGHT) | set(HEAVY)) - have)
