"""The hive's held-row kernels (the hive under the budgeted step) on the host: csrc/rr_hive.hpp compiled with g++, every lane-parallel
phase a loop over the virtual wave's lanes (tests/emu/rr_hive_held_emu.cpp).

What is checked is which cells each of the three may write -- a held arena's rows are the memory of the step it is in the middle of --
and that everything else is what the plain kernels write: the observer bit for bit against the emulated hive_observe, the commit
against a numpy restatement of include/roborugby_amd.h (rr_hive_commit)."""
import numpy as np
import pytest

import hive_emu_lib as he
import hive_held_emu_lib as hh
import oracle_lib as ol

THRUST = np.array(((1, 1), (-1, -1), (-1, 1), (1, -1), (0, 1), (1, 0), (-1, 0), (0, -1)), np.float32)  # RR_EnvBase.py:593-602


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("preset,vw", [("G", 8), ("G", 64), ("T", 2)])
@pytest.mark.parametrize("kind", [0, 1])
def test_observe_holds_the_rows_of_parked_arenas_and_is_hive_observe_elsewhere(preset, vw, kind):
    cfg = ol.PRESETS[preset]
    nr, nb = cfg["nr_h"] + cfg["nr_g"], cfg["nb_p"] + cfg["nb_n"]
    rng = np.random.default_rng(20 + vw)
    n = 64
    robots, balls = he.random_layouts(rng, n, nr, nb, cfg["W"], cfg["H"])
    parked = (np.arange(n) % 3 == 0).astype(np.uint8)
    for mask in ((1 << nr) - 1, 1):
        want_a, want_o = he.hive_observe(preset, robots, balls, mask, kind, vw)
        assign = np.full((n, nr), -7, np.int32)
        obs = np.full((n, nr, 11), np.nan)
        held = hh.hive_observe_held(preset, robots, balls, parked, mask, kind, vw, assign, obs)
        assert np.array_equal(held, parked)
        p = parked.astype(bool)
        assert np.all(assign[p] == -7) and np.all(np.isnan(obs[p]))  # untouched
        assert np.array_equal(assign[~p], want_a[~p])
        assert np.array_equal(_bits(obs[~p]), _bits(want_o[~p]))
        assert (want_a[~p] >= 0).any()  # (not vacuous: robots were given balls)
        # nobody parked: the plain observer, held all 0
        assign[:] = -7
        obs[:] = np.nan
        held = hh.hive_observe_held(preset, robots, balls, np.zeros(n, np.uint8), mask, kind, vw, assign, obs)
        assert not held.any() and np.array_equal(assign, want_a) and np.array_equal(_bits(obs), _bits(want_o))


def _commit_restated(nr, mask, fresh, assign, held, accepted, thrust):
    """include/roborugby_amd.h (rr_hive_commit), cell by cell"""
    accepted, thrust = accepted.copy(), thrust.copy()
    for a in range(fresh.shape[0]):
        for r in range(nr):
            if held[a] or not (mask >> r) & 1:
                continue
            accepted[a, r] = fresh[a, r]
            moves = assign[a, r] >= 0 and 0 <= fresh[a, r] < 8
            thrust[a, 2 * r:2 * r + 2] = THRUST[fresh[a, r]] if moves else 0
    return accepted, thrust


@pytest.mark.parametrize("mask", [3, 15, 4])
def test_commit_writes_only_the_cells_it_may_and_the_reference_table_there(mask):
    nr, nb, n = 4, 8, 203
    rng = np.random.default_rng(mask)
    fresh = rng.integers(-2, 10, (n, nr)).astype(np.int32)  # -2 .. 9: values outside 0..7 occur
    assign = np.where(rng.random((n, nr)) < .4, -1, rng.integers(0, nb, (n, nr))).astype(np.int32)
    held = (np.arange(n) % 4 == 0).astype(np.uint8)
    accepted0 = np.full((n, nr), -99, np.int32)
    thrust0 = np.full((n, 2 * nr), 7.5, np.float32)
    accepted, thrust = accepted0.copy(), thrust0.copy()
    hh.hive_commit(nr, mask, fresh, assign, held, accepted, thrust)
    want_a, want_t = _commit_restated(nr, mask, fresh, assign, held, accepted0, thrust0)
    assert np.array_equal(accepted, want_a) and np.array_equal(_bits(thrust), _bits(want_t))
    may = (held == 0)[:, None] & (((mask >> np.arange(nr)) & 1) == 1)[None, :]
    assert np.all(accepted[~may] == -99) and np.all(thrust.reshape(n, nr, 2)[~may] == 7.5)
    assert np.array_equal(accepted[may], fresh[may])
    t3 = thrust.reshape(n, nr, 2)
    out_of_range = may & ((fresh < 0) | (fresh >= 8))
    assert out_of_range.any() and np.all(t3[out_of_range] == 0)           # never an index
    assert np.all(t3[may & (assign < 0)] == 0)                             # a robot without a ball stands still
    moving = may & (assign >= 0) & (fresh >= 0) & (fresh < 8)
    assert moving.sum() > 20 and np.array_equal(t3[moving], THRUST[fresh[moving]])
    assert len({int(f) for f in fresh[moving]}) == 8                       # every direction of the table was looked up


def test_thrust_table_is_the_players_table():
    from roborugby_amd import players
    assert np.array_equal(THRUST, np.array(players._THRUST_FROM_DIRECTION, np.float32))
    fresh = np.arange(8, dtype=np.int32).reshape(8, 1)
    accepted, thrust = np.zeros((8, 1), np.int32), np.full((8, 2), 9, np.float32)
    hh.hive_commit(1, 1, fresh, np.zeros((8, 1), np.int32), np.zeros(8, np.uint8), accepted, thrust)
    assert np.array_equal(thrust, THRUST)


@pytest.mark.parametrize("preset,vw,nr", [("G", 8, 4), ("G", 64, 4), ("T", 2, 1)])
def test_idle_arenas_get_hive_transitions_zero_rows_and_stepped_arenas_nothing(preset, vw, nr):
    AFTER_DONE, WAS_RESET, NOT_READY = 64, 1024, 16384  # include/roborugby_amd.h: RR_STATUS_*
    n = 40
    status = np.zeros(n, np.int32)
    status[1::4] = NOT_READY
    status[2::8] = WAS_RESET
    status[3::8] = NOT_READY | (5 << 16)
    status[6::8] = AFTER_DONE
    status[7::8] = 3 << 16 | 256  # NaughtyBots bits and a warning only: the arena stepped
    next_obs = np.full((n, nr, 11), np.nan)
    reward = np.full((n, nr), np.nan)
    terminal = np.full((n, nr), 9, np.uint8)
    valid = np.full((n, nr), 9, np.uint8)
    wrote = hh.hive_idle(preset, vw, status, next_obs, reward, terminal, valid)
    idle = (status & (AFTER_DONE | WAS_RESET | NOT_READY)) != 0
    assert np.array_equal(wrote.astype(bool), idle)
    assert np.all(_bits(next_obs[idle]) == 0) and np.all(_bits(reward[idle]) == 0) and not terminal[idle].any() and not valid[idle].any()
    assert np.all(np.isnan(next_obs[~idle])) and np.all(np.isnan(reward[~idle])) and np.all(terminal[~idle] == 9) and np.all(valid[~idle] == 9)
