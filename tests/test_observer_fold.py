"""The step's fused two-team observer (observe_both) and the single observer (observe) are one body (csrc/rr_sim.hpp: lidar_task,
observe_scalars, observe_row): on the same state they give the same rows, bit for bit -- on the host-emulated wave and on the device."""
import numpy as np
import pytest

import emu_lib as el
import oracle_lib as ol

LAYOUTS = [(0, 0), (1, 0), (7, 3), (63, 1), (64, 2), (1000, 5)]  # (arena, episode) of the counter-based reset


def _fused_equals_single(preset, narrow, layouts, steps, exact=None):
    rng = np.random.default_rng(12)
    env = el.EmuEnv(preset, narrow=narrow, exact=exact)
    n = 0
    for arena, episode in layouts:
        env.reset(arena, episode)
        for _ in range(steps):
            r = env.step(rng.integers(0, 8, env.nr))
            assert np.array_equal(r["obs"], env.observe(1)), (preset, narrow, arena, episode, n)
            assert np.array_equal(r["obs_g"], env.observe(-1)), (preset, narrow, arena, episode, n)
            n += 1
    return n


@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("preset", ["G", "D"])
def test_step_rows_equal_single_observer_on_the_emulated_wave(preset, narrow):
    """G takes the fused path (both teams' lidar tasks in shared rounds, the tails in lanes 0 and 1), D the single path twice; narrow
    runs the task loops in several rounds.  After every step the step's rows are the single observer's on the post-step state."""
    assert _fused_equals_single(preset, narrow, LAYOUTS, 40) == 240


@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("preset", ["G", "D"])
def test_step_rows_equal_single_observer_in_the_parity_build(preset, narrow):
    assert _fused_equals_single(preset, narrow, LAYOUTS[2:4], 40, exact=True) == 80


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["G", "D"])
def test_step_rows_equal_single_observer_on_device(preset):
    """67 arenas: the last wavefront is ragged (8 resp. 16 arenas per wavefront).  fp64 rows and fp32 rows (the latter stage 11
    four-byte values in the array the minima came from); one arena of G also against the oracle, explicit indices, after steps."""
    torch = pytest.importorskip("torch")
    import roborugby_amd as rr
    n = 67
    env = rr.BatchedRoboRugbyEnv(n, preset=preset, seed=5, auto_reset=False, time_limit=False)
    env.reset()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(9)
    for f64 in (True, False):
        for step in range(8):
            acts = torch.randint(0, 8, (n, env.preset.nr), generator=gen, device="cuda", dtype=torch.int32)
            obs, _, _, info = env.step_f64(acts) if f64 else env.step(acts)
            assert obs.dtype == (torch.float64 if f64 else torch.float32)
            assert torch.equal(obs, env.get_game_state(1, f64=f64)), (preset, f64, step)
            assert torch.equal(info.adblGrumpyState, env.get_game_state(-1, f64=f64)), (preset, f64, step)
        if preset == "G" and f64:
            st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
            a = n - 1  # in the ragged wavefront
            o = ol.OracleEnv("G")
            o.set_state(st["robots"][a], st["robots_i"][a], st["balls"][a], None, st["step"][a])
            for c in [(1, 1, 2), (-1, 3, 5), (1, -1, -1), (-1, -1, -1)]:
                got = env.get_game_state(c[0], c[1], c[2], f64=True)[a].cpu().numpy()
                assert np.allclose(o.observe(*c), got, atol=1e-9, rtol=0), c
    env.close()
