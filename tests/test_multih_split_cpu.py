"""How many lock-step groups the batched multi-homography drivers cut a batch into (rfx.rounds.split_policy), a pure function of the
batch size, the caller's ``split``, two environment switches and the reasons that force one group.  No GPU.  The expected values
are the drivers' behaviour before the policy became one function: 4 / 3 / 2 groups from 32 / 12 / 8 pairs (Hpatch), 2 from 16 (KITTI)."""
import pytest

from rfx.rounds import HPATCH_SPLIT, KITTI_SPLIT, split_policy


@pytest.mark.parametrize("B, want", [(1, 1), (7, 1), (8, 2), (11, 2), (12, 3), (31, 3), (32, 4), (64, 4)])
def test_hpatch_defaults(B, want):
    assert split_policy(B, None, HPATCH_SPLIT, env={}) == want


@pytest.mark.parametrize("B, want", [(8, 1), (15, 1), (16, 2)])
def test_kitti_defaults(B, want):
    assert split_policy(B, None, KITTI_SPLIT, env={}) == want


def test_argument_and_environment_win_over_the_default(monkeypatch):
    assert split_policy(64, 6, HPATCH_SPLIT, env={}) == 6
    assert split_policy(64, 1, HPATCH_SPLIT, env={}) == 1
    assert split_policy(64, None, HPATCH_SPLIT, env={"RFX_MULTIH_SPLIT": "6"}) == 6
    assert split_policy(16, None, KITTI_SPLIT, env={"RFX_MULTIH_SPLIT": "1"}) == 1
    assert split_policy(64, None, HPATCH_SPLIT, env={"RFX_MULTIH_SPLIT": "0"}) == 4          # 0 = unset
    assert split_policy(64, 2, HPATCH_SPLIT, env={"RFX_MULTIH_SPLIT": "6"}) == 2             # the argument wins over the variable
    monkeypatch.setenv("RFX_MULTIH_SPLIT", "5")                                              # without ``env``: the process environment
    assert split_policy(64, None, HPATCH_SPLIT) == 5
    monkeypatch.delenv("RFX_MULTIH_SPLIT")
    assert split_policy(64, None, HPATCH_SPLIT) == 4


@pytest.mark.parametrize("reason", ["host_draw", "trace", "host_filter", "profiled"])
def test_reasons_that_force_one_group(reason):
    for split, env in ((None, {}), (3, {}), (None, {"RFX_MULTIH_SPLIT": "4"})):
        assert split_policy(64, split, HPATCH_SPLIT, env=env, **{reason: True}) == 1
        assert split_policy(64, split, KITTI_SPLIT, env=env, **{reason: True}) == 1


def test_profiled_switch_lifts_only_the_profiler_rule():
    env = {"RFX_MULTIH_SPLIT_PROFILED": "1"}
    assert split_policy(64, None, HPATCH_SPLIT, profiled=True, env=env) == 4
    assert split_policy(64, 3, HPATCH_SPLIT, profiled=True, env=env) == 3
    assert split_policy(64, None, HPATCH_SPLIT, profiled=True, env={"RFX_MULTIH_SPLIT_PROFILED": "0"}) == 1
    for reason in ("host_draw", "trace", "host_filter"):
        assert split_policy(64, None, HPATCH_SPLIT, profiled=True, env=env, **{reason: True}) == 1


def test_result_is_clamped_to_the_batch():
    assert split_policy(3, 100, HPATCH_SPLIT, env={}) == 3
    assert split_policy(3, None, HPATCH_SPLIT, env={"RFX_MULTIH_SPLIT": "8"}) == 3
    assert split_policy(5, 0, HPATCH_SPLIT, env={}) == 1
    assert split_policy(5, -2, HPATCH_SPLIT, env={}) == 1
    assert split_policy(1, None, KITTI_SPLIT, env={}) == 1
