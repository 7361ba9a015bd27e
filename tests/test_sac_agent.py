"""roborugby_amd.sac.BatchedSACAgent on device "cpu" (the torch paths; no kernel runs): the target's initial copy and soft update, the three
losses against tests/sac_ref.py's float64 restatement, terminal rows, the replay ring and the checkpoint.  CPU only."""
import pytest

torch = pytest.importorskip("torch")

import sac_ref  # noqa: E402
from roborugby_amd.sac import ActorNetwork, BatchedSACAgent, CriticNetwork, ValueNetwork  # noqa: E402


def _agent(A=2, **kw):
    kw.setdefault("batch_size", 64)
    kw.setdefault("max_mem_size", 256)
    return BatchedSACAgent(n_actions=A, device="cpu", seed=3, **kw)


def _nets(ag):
    return {k: {n: p.detach().clone() for n, p in getattr(ag, k).state_dict().items()} for k in BatchedSACAgent._NETS}


def _batch(A, n=64, seed=0, terminal_every=5):
    g = torch.Generator().manual_seed(seed)
    state, state_ = torch.rand(n, 11, generator=g) * 2 - 1, torch.rand(n, 11, generator=g) * 2 - 1
    action = torch.rand(n, A, generator=g) * 2 - 1
    reward = torch.randn(n, generator=g)
    done = (torch.arange(n) % terminal_every) == 0
    return state, action, reward, state_, done


def test_defaults_are_the_references_and_shapes():
    ag = BatchedSACAgent(device="cpu", max_mem_size=128)
    assert (ag.gamma, ag.tau, ag.scale, ag.batch_size) == (0.99, 0.005, 2.0, 4096)
    assert all(g["lr"] == 1e-4 for o in (ag.actor_optimizer, ag.value_optimizer, ag.critic_optimizer) for g in o.param_groups)
    assert BatchedSACAgent.__init__.__defaults__[6] == 1 << 20  # max_mem_size
    assert ag.fused is False and ag._dqn is None  # no GPU: the torch path
    assert isinstance(ag.actor, ActorNetwork) and isinstance(ag.critic_1, CriticNetwork) and isinstance(ag.value, ValueNetwork)
    assert [tuple(p.shape) for p in ag.actor.parameters()] == [(256, 11), (256,), (256, 256), (256,), (2, 256), (2,), (2, 256), (2,)]
    assert ag.critic_1.fc1.weight.shape == (256, 13) and _agent(4).critic_2.fc1.weight.shape == (256, 15)
    assert ag.action_memory.shape == (128, 2) and ag.action_memory.dtype == torch.float32
    with pytest.raises(ValueError):
        BatchedSACAgent(device="cpu", max_mem_size=64, fused=True)


def test_construction_copies_value_into_target_and_soft_update_moves_it_by_tau():
    ag = _agent()
    for pt, pv in zip(ag.target_value.parameters(), ag.value.parameters()):
        assert pt is not pv and torch.equal(pt, pv)
    before = [p.detach().clone() for p in ag.target_value.parameters()]
    with torch.no_grad():
        for p in ag.value.parameters():
            p.add_(1.0)
    ag.update_network_parameters()
    for pt, pv, b in zip(ag.target_value.parameters(), ag.value.parameters(), before):
        assert torch.allclose(pt, b + ag.tau * 1.0, rtol=0, atol=1e-6)
        assert torch.allclose(pt, ag.tau * pv + (1 - ag.tau) * b, rtol=0, atol=1e-6)
    ag.update_network_parameters(tau=1)
    for pt, pv in zip(ag.target_value.parameters(), ag.value.parameters()):
        assert torch.allclose(pt, pv, rtol=0, atol=1e-6)


@pytest.mark.parametrize("A", [2, 4])
def test_losses_equal_the_float64_restatement(A):
    ag = _agent(A)
    with torch.no_grad():  # a target that differs from the value net, heads that use both arms of the clamp
        for p in ag.target_value.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(1)))
        ag.actor.sigma.weight.mul_(8.0)
        ag.actor.sigma.bias.add_(0.5)
    batch = _batch(A)
    g = torch.Generator().manual_seed(9)
    noise_v, noise_a = torch.randn(64, A, generator=g), torch.randn(64, A, generator=g)
    got = [float(x.detach()) for x in ag.losses(batch, noise_v, noise_a)]
    ref = sac_ref.losses64(_nets(ag), [t.numpy() for t in batch], noise_v.numpy(), noise_a.numpy(), ag.gamma, ag.scale, ag.max_action)
    raw = ag.actor.head(batch[0])[1]
    assert bool((raw < 1e-6).any()) and bool((raw > 1).any())
    for name, x, r in zip(("value", "actor", "critic"), got, ref):
        print(f"A = {A} {name} loss {x:.8g} (float64 {r:.8g})")
        assert abs(x - r) <= 1e-5 * max(1.0, abs(r)), (name, x, r)
    # the same function of the same noise: nothing else is drawn inside
    assert got == [float(x.detach()) for x in ag.losses(batch, noise_v, noise_a)]


def test_terminal_rows_contribute_scale_times_reward_only():
    ag = _agent()
    state, action, reward, state_, done = _batch(2)
    noise = torch.zeros(64, 2)
    all_terminal = torch.ones(64, dtype=torch.bool)
    c = float(ag.losses((state, action, reward, state_, all_terminal), noise, noise)[2].detach())
    with torch.no_grad():
        q_hat = ag.scale * reward
        ref = 0.5 * ((ag.critic_1(state, action).view(-1) - q_hat) ** 2).mean() + 0.5 * ((ag.critic_2(state, action).view(-1) - q_hat) ** 2).mean()
    assert abs(c - float(ref)) <= 1e-6 * max(1.0, abs(float(ref)))
    # ... whatever the next state is
    c2 = float(ag.losses((state, action, reward, state_ * 100.0, all_terminal), noise, noise)[2].detach())
    assert c2 == c
    c3 = float(ag.losses((state, action, reward, state_ * 100.0, done), noise, noise)[2].detach())
    assert c3 != c


def test_ring_write_keeps_valid_rows_in_order_and_wraps():
    A, M = 2, 10
    ag = _agent(A, max_mem_size=M, batch_size=4)
    def rows(lo, n):
        k = torch.arange(lo, lo + n, dtype=torch.float32)
        return k.view(-1, 1).repeat(1, 11), k.view(-1, 1).repeat(1, A) / 100, k, -k.view(-1, 1).repeat(1, 11), (k.long() % 3) == 0
    s, a, r, s2, d = rows(0, 8)
    valid = torch.tensor([1, 0, 1, 1, 0, 0, 1, 1], dtype=torch.bool)
    ag.remember(s, a, r, s2, d, valid=valid)
    assert ag.mem_cntr == 5
    assert ag.reward_memory[:5].tolist() == [0, 2, 3, 6, 7]
    assert torch.equal(ag.action_memory[:5], a[valid]) and torch.equal(ag.state_memory[:5], s[valid]) and torch.equal(ag.new_state_memory[:5], s2[valid])
    assert ag.terminal_memory[:5].tolist() == [True, False, True, True, False]
    s, a, r, s2, d = rows(100, 8)
    ag.remember(s, a, r, s2, d)  # all eight: positions 5..9, then 0..2
    assert ag.mem_cntr == 13
    assert ag.reward_memory.tolist() == [105, 106, 107, 6, 7, 100, 101, 102, 103, 104]
    assert torch.allclose(ag.action_memory[:, 0], ag.reward_memory / 100)
    ag.remember(*rows(0, 8), valid=torch.zeros(8, dtype=torch.bool))  # nothing valid: nothing moves
    assert ag.mem_cntr == 13
    with pytest.raises(ValueError):
        ag.remember(*rows(0, 11))


def test_learn_steps_every_network_in_order_and_returns_three_losses():
    ag = _agent(2, max_mem_size=128, batch_size=64)
    assert ag.learn() is None  # not a batch yet
    state, action, reward, state_, done = _batch(2, n=100, seed=4)
    ag.remember(state, action, reward, state_, done)
    before = {k: [p.detach().clone() for p in getattr(ag, k).parameters()] for k in BatchedSACAgent._NETS}
    losses = ag.learn()
    assert len(losses) == 3 and all(torch.isfinite(x) for x in losses) and ag.updates == 1
    for k in BatchedSACAgent._NETS:
        assert any(not torch.equal(p, b) for p, b in zip(getattr(ag, k).parameters(), before[k])), k
    for pt, pv, b in zip(ag.target_value.parameters(), ag.value.parameters(), before["target_value"]):
        assert torch.allclose(pt, ag.tau * pv + (1 - ag.tau) * b, rtol=0, atol=1e-7)


def test_torch_choose_action_shapes_and_deterministic():
    ag = _agent(4)
    obs = torch.rand(100, 11) * 2 - 1
    a = ag.choose_action(obs)
    assert a.shape == (100, 4) and a.dtype == torch.float32 and bool((a.abs() <= 1).all())
    d = ag.choose_action(obs, deterministic=True)
    assert torch.equal(d, ag.choose_action(obs, deterministic=True))
    assert torch.allclose(d, torch.tanh(ag.actor(obs)[0]))
    assert ag._act_calls == 0  # only fused calls count


def test_state_dict_round_trip_restores_act_calls_and_leaves_the_replay_out():
    ag = _agent(2, max_mem_size=128)
    ag.remember(*_batch(2, n=100, seed=4))
    ag.learn()
    ag._act_calls = 41
    sd = ag.state_dict()
    assert not any("memory" in k for k in sd) and sd["act_calls"] == 41 and sd["kind"] == "sac"
    other = BatchedSACAgent(n_actions=2, device="cpu", seed=99, batch_size=64, max_mem_size=128)
    other.load_state_dict(sd)
    assert other._act_calls == 41 and other.updates == 1 and other.mem_cntr == 0
    for k in BatchedSACAgent._NETS:
        for p, q in zip(getattr(ag, k).parameters(), getattr(other, k).parameters()):
            assert torch.equal(p, q), k
    assert other.actor_optimizer.state_dict()["state"][0]["exp_avg"].equal(ag.actor_optimizer.state_dict()["state"][0]["exp_avg"])
    with pytest.raises(ValueError):
        _agent(4).load_state_dict(sd)
