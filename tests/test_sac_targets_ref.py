"""tests/sac_targets_ref.py held to its own yardsticks, without a GPU: the float64 restatement of the no-grad half of Agent.learn against
the reference trainer's own float64 run (tests/golden/sac_learn.npz, width 32 -- the restatement is width-agnostic), and the conditions
the GPU tests' inputs (case(A)) must meet for those tests to mean what they say."""
import numpy as np
import pytest

import sac_ref
import sac_targets_ref as tr
from test_agent_reference import ACTOR_KEYS, fixture

CASES = tuple(fixture("sac_learn.npz")[1]["cases"])
OUT = {"critic_1": "q", "critic_2": "q", "value": "v", "target_value": "v"}


def _fixture_nets(case):
    fx, _ = fixture("sac_learn.npz")
    nets = {net: tuple(fx[f"{case}.w.{net}.{k}"] for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", f"{o}.weight", f"{o}.bias"))
            for net, o in OUT.items()}
    nets["actor"] = tuple(fx[f"{case}.w.actor.{k}"] for k in ACTOR_KEYS)
    return nets


def test_there_are_four_cases():
    assert len(CASES) == 4


@pytest.mark.parametrize("case", CASES)
def test_targets64_reproduces_the_reference_learn_losses(case):
    fx, meta = fixture("sac_learn.npz")
    hp = meta["hyper"]
    nets = _fixture_nets(case)
    state, action, reward, new_state, done = (fx[f"{case}.{k}"] for k in ("state", "action", "reward", "new_state", "done"))
    B = state.shape[0]
    t = tr.targets64(nets, (state, new_state, action, reward, done), np.arange(B), fx[f"{case}.noise_value"], hp["gamma"], hp["reward_scale"],
                     meta["max_action"])
    value_loss = 0.5 * np.mean((tr.mlp64(nets["value"], state) - t["value_target"]) ** 2)
    critic_loss = 0.5 * np.mean((tr.critic64(nets["critic_1"], state, action) - t["q_hat"]) ** 2) \
        + 0.5 * np.mean((tr.critic64(nets["critic_2"], state, action) - t["q_hat"]) ** 2)
    ref = fx[f"{case}.losses64"]
    print(f"  {case}: value loss {value_loss:.15g} (reference {ref[0]:.15g}), critic loss {critic_loss:.15g} (reference {ref[2]:.15g})")
    assert abs(value_loss - ref[0]) <= 1e-12 * abs(ref[0])
    assert abs(critic_loss - ref[2]) <= 1e-12 * abs(ref[2])
    assert done.any() and not done.all()  # the masked term is exercised both ways


def test_closing_formulas_in_float32():
    f = np.float32
    q1, q2, lp = np.array([1.5, -2.0, 0.25], f), np.array([1.25, 3.0, 0.25], f), np.array([0.1, -0.7, 1e-3], f)
    assert np.array_equal(tr.value_target32(q1, q2, lp), np.array([f(1.25) - f(0.1), f(-2.0) - f(-0.7), f(0.25) - f(1e-3)], f))
    r, v, done = np.array([0.3, -1.7, 2.5], f), np.array([0.9, np.inf, -0.4], f), np.array([False, True, True])
    got = tr.q_hat32(2.0, r, 0.99, done, v)
    assert got[0] == f(f(2.0) * f(0.3)) + f(f(0.99) * f(0.9))
    assert got[1] == f(2.0) * f(-1.7) and got[2] == f(2.0) * f(2.5)  # terminal: exactly fl(reward_scale * r), whatever v is
    assert np.array_equal(tr.ring_row_ok([-1, 0, 299, 300], 300), [False, True, True, False])


def test_the_draw_is_another_stream_than_acting():
    n = 256
    assert tr.TARGETS_STREAM == 0x5A7A != sac_ref.SAC_STREAM
    assert not np.array_equal(tr.row_uniforms(2, n, 7), sac_ref.row_uniforms(2, n, 7))
    z = tr.draw64(2, 65536, 7)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01


@pytest.mark.parametrize("A", [2, 4])
def test_case_conditions(A):
    nets, rings, index = tr.case(A)
    state_m, new_state_m, action_m, reward_m, terminal_m = rings
    assert state_m.shape == (tr.M, 11) and new_state_m.shape == (tr.M, 11) and action_m.shape == (tr.M, A) and tr.M % 64 != 0
    assert np.array_equal(state_m, sac_ref.case(A)[1][:tr.M])
    assert np.array_equal(np.flatnonzero(terminal_m), np.arange(0, tr.M, 5))
    assert nets["critic_1"][0].shape == (256, 11 + A) and nets["target_value"][0].shape == (256, 11) and nets["critic_2"][4].shape == (1, 256)
    assert index.min() == 0 and index.max() == tr.M - 1 and np.array_equal(index[:4], (0, tr.M - 1, 0, tr.M - 1))
    head_m = sac_ref.actor_head64(nets["actor"], state_m)
    for seed, call, B in tr.GPU_DRAWS:
        idx = index[:B]
        assert 0 in idx and tr.M - 1 in idx and len(np.unique(idx)) < B  # both ends of the ring, repeats
        head = head_m[idx]
        a64, _, _ = sac_ref.squash64(head, tr.draw64(seed, B, call)[:, :A])
        well = sac_ref.well_conditioned_rows(a64)
        raw = head[:, A:]
        print(f"  A = {A} seed {seed:#x} call {call:#x} B = {B}: {well.mean():.4f} well-conditioned, sigma below {np.mean(raw < 1e-6):.2f} / "
              f"above {np.mean(raw > 1.0):.2f} of the clamp")
        assert well.mean() >= 0.90
        assert np.any(raw < 1e-6) and np.any(raw > 1.0) and np.any((raw > 1e-6) & (raw < 1.0))  # both arms of the clamp, and neither
        done = terminal_m[idx].reshape(-1, 64)
        assert np.all(done.any(1)) and not np.any(done.all(1))  # a terminal and a non-terminal row in every 64-row tile
