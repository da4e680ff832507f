"""The host-side rules of the trunk feature pass (rfx.trunk_pass): when a shape gets a captured HIP graph and which captures are kept
(CapturePolicy), how images are dealt to grouped chains (balance_chains), how many streams the per-level passes use
(level_stream_count) and which pyramid level shares its pass with the target (pair_level_with_target).  No GPU.  The expected values
are written out from the rules -- second sighting, 64 remembered keys, MAX_GRAPHS captures least recently used first; largest first
to the lightest chain, ties to the lowest index; one stream per level up to four pairs, four above, one under a profiler."""
import pytest

from rfx.pipeline import AlignPipeline, resize_dims, scale_list
from rfx.trunk_pass import CapturePolicy, balance_chains, level_stream_count, pair_level_with_target

MAX_GRAPHS = 4


def test_the_constants_of_the_policy():
    assert AlignPipeline.MAX_GRAPHS == MAX_GRAPHS and CapturePolicy.SEEN_MAX == 64


def test_eager_then_capture_then_replay():
    p = CapturePolicy(MAX_GRAPHS)
    key = (((1, 3, 128, 160),), (1, 3, 128, 160))
    assert not p.entries
    assert p.decide(key) == "eager"
    assert not p.entries
    assert p.decide(key) == "capture"
    assert p.decide(key) == "capture"           # nothing stored (a failed capture): still due
    p.store(key, "graph")
    assert p.decide(key) == "replay" and p.entries[key] == "graph"
    assert p.decide(key) == "replay"
    assert p.decide("other") == "eager"


def test_a_key_pushed_out_of_the_seen_set_is_eager_again():
    p = CapturePolicy(MAX_GRAPHS)
    assert p.decide("a") == "eager"
    for k in range(63):
        assert p.decide(k) == "eager"
    assert p.decide("a") == "capture"           # 64 keys remembered: "a" is the oldest of them
    assert p.decide(63) == "eager"              # the 65th key pushes "a" out; a sighting does not make a key younger
    assert p.decide("a") == "eager"             # ... which in turn pushes key 0 out
    assert p.decide(0) == "eager"
    assert p.decide(2) == "capture"
    assert len(p.seen) == 64


def test_one_more_entry_than_the_bound_evicts_the_least_recently_used():
    p = CapturePolicy(MAX_GRAPHS)
    for k in range(MAX_GRAPHS + 1):
        p.decide(k), p.decide(k)
        p.store(k, "g%d" % k)
    assert list(p.entries) == [1, 2, 3, 4]
    assert p.decide(0) == "capture"             # evicted, but seen before: captured again at its next sighting


def test_a_replay_refreshes_recency():
    p = CapturePolicy(MAX_GRAPHS)
    for k in range(MAX_GRAPHS):
        p.store(k, "g%d" % k)
    assert p.decide(0) == "replay"
    p.store(4, "g4")
    assert list(p.entries) == [2, 3, 0, 4]      # 1 was the least recently used; 0 survived
    p.store(5, "g5")
    assert list(p.entries) == [3, 0, 4, 5]


def test_shape_keys_and_raw_keys_share_the_bound():
    p = CapturePolicy(MAX_GRAPHS)
    shape = lambda h: (((1, 3, h, 160),), (1, 3, h, 160))
    raw = lambda h: ("raw", (1, h, 160, 3), (1, h, 160, 3))
    keys = [shape(96), raw(96), shape(112), raw(112), raw(128)]
    for k in keys:
        assert p.decide(k) == "eager" and p.decide(k) == "capture"
        p.store(k, object())
    assert list(p.entries) == keys[1:]
    assert len(p.seen) == 5                     # one seen-set for both callers


def test_balance_chains_ties_go_to_the_lowest_index():
    # equal sizes keep their index order (0 before 2); equal loads (0 / 0, then 5 / 5) pick the lowest chain
    assert balance_chains([5, 3, 5, 2], 2) == [[0, 1], [2, 3]]
    assert balance_chains([8, 6, 6, 4, 2], 3) == [[0], [1, 3], [2, 4]]


def test_balance_chains_with_more_chains_than_items_leaves_empty_chains():
    assert balance_chains([4, 9], 4) == [[1], [0], [], []]
    assert balance_chains([], 2) == [[], []]


def test_balance_chains_one_chain_takes_everything_largest_first():
    assert balance_chains([1, 7, 3], 1) == [[1, 2, 0]]


@pytest.mark.parametrize("B, n_levels, want", [(1, 3, 3), (1, 7, 7), (4, 3, 3), (4, 7, 7), (5, 3, 3), (5, 7, 4)])
def test_level_stream_count(B, n_levels, want):
    assert level_stream_count(B, n_levels, None, False) == want
    assert level_stream_count(B, n_levels, "", False) == want          # an empty variable counts as unset
    assert level_stream_count(B, n_levels, "1", False) == 1
    assert level_stream_count(B, n_levels, "2", False) == 2
    assert level_stream_count(B, n_levels, "0", False) == 1            # clamped to at least one stream
    for env in (None, "1", "2", "0"):
        assert level_stream_count(B, n_levels, env, True) == 1         # always one stream under a profiler


def test_pair_level_with_target_first_match_wins():
    a, b, c = (2, 3, 144, 192), (2, 3, 128, 160), (2, 3, 96, 128)
    assert pair_level_with_target([a, b, c], b) == 1
    assert pair_level_with_target([a, b, b], b) == 1
    assert pair_level_with_target([b, a, b], b) == 0
    assert pair_level_with_target([a, b, c], (2, 3, 96, 160)) is None
    assert pair_level_with_target([], b) is None


def _shapes(src_hw, tgt_hw, nbScale=3, minSize=160, scaleR=1.2):
    dims = lambda hw, size: resize_dims(hw[1], hw[0], size, "max")[::-1]
    return [dims(src_hw, int(minSize * s)) for s in scale_list(nbScale, scaleR)], dims(tgt_hw, minSize)


def test_the_pair_sizes_of_the_gpu_test_cover_both_branches_of_the_pairing_rule():
    """tests/test_gpu_multih.py::test_trunk_pass_forms_equal_the_plain_form: a 128x160 source with a 128x160 target has its scale-1
    level at the target's shape; with a 96x160 target no level has."""
    src, tgt = _shapes((128, 160), (128, 160))
    assert src == [(144, 192), (128, 160), (96, 128)] and tgt == (128, 160)
    assert pair_level_with_target(src, tgt) == 1
    src, tgt = _shapes((128, 160), (96, 160))
    assert src == [(144, 192), (128, 160), (96, 128)] and tgt == (96, 160)
    assert pair_level_with_target(src, tgt) is None
