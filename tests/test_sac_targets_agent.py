"""BatchedSACAgent's split of losses() into targets() + losses_given_targets() and the fused_targets switch, on the CPU torch path: the
composition is today's losses() bit for bit, the switch is off by default and refuses what rr_sac_targets cannot take, and the learn
counter that keys the kernel's draws is checkpointed."""
import pytest

torch = pytest.importorskip("torch")

from roborugby_amd.sac import BatchedSACAgent, train_sac  # noqa: E402


def _agent_and_batch(A, B=96, seed=3):
    ag = BatchedSACAgent(n_actions=A, batch_size=B, max_mem_size=256, device="cpu", seed=seed, fc1_dims=32, fc2_dims=32)
    g = torch.Generator().manual_seed(100 + A)
    batch = (torch.rand(B, 11, generator=g) * 2 - 1, torch.rand(B, A, generator=g) * 2 - 1, torch.randn(B, generator=g),
             torch.rand(B, 11, generator=g) * 2 - 1, torch.arange(B) % 5 == 0)
    return ag, batch, torch.randn(B, A, generator=g), torch.randn(B, A, generator=g)


def _todays_losses(ag, batch, noise_value, noise_actor):
    """losses() as it stood before the split, statement by statement"""
    import torch.nn.functional as F
    state, action, reward, state_, done = batch
    value = ag.value(state).view(-1)
    with torch.no_grad():
        value_ = ag.target_value(state_).view(-1).masked_fill(done, 0.0)
        actions, log_probs = ag.actor.sample_normal(state, noise_value, reparameterize=False)
        value_target = torch.min(ag.critic_1(state, actions), ag.critic_2(state, actions)).view(-1) - log_probs
    value_loss = 0.5 * F.mse_loss(value, value_target)
    actions, log_probs = ag.actor.sample_normal(state, noise_actor, reparameterize=True)
    critic_value = torch.min(ag.critic_1(state, actions), ag.critic_2(state, actions)).view(-1)
    actor_loss = torch.mean(log_probs - critic_value)
    q_hat = ag.scale * reward + ag.gamma * value_
    critic_loss = 0.5 * F.mse_loss(ag.critic_1(state, action).view(-1), q_hat) + 0.5 * F.mse_loss(ag.critic_2(state, action).view(-1), q_hat)
    return value_loss, actor_loss, critic_loss


@pytest.mark.parametrize("A", [2, 4])
def test_targets_then_losses_given_targets_is_losses_bit_for_bit(A):
    ag, batch, nv, na = _agent_and_batch(A)
    whole = ag.losses(batch, nv, na)
    value_target, q_hat = ag.targets(batch, nv)
    assert value_target.shape == q_hat.shape == (batch[0].shape[0],) and not value_target.requires_grad and not q_hat.requires_grad
    parts = ag.losses_given_targets(batch[0], batch[1], value_target, q_hat, na)
    before = _todays_losses(ag, batch, nv, na)
    for a, b, c in zip(whole, parts, before):
        assert torch.equal(a, b) and torch.equal(a, c)
    # ... and the gradients of the composition are those of the statements it replaces
    params = [p for net in (ag.value, ag.actor, ag.critic_1, ag.critic_2) for p in net.parameters()]
    for a, c in zip(whole, before):
        for ga, gc in zip(torch.autograd.grad(a, params, allow_unused=True), torch.autograd.grad(c, params, allow_unused=True)):
            assert (ga is None) == (gc is None) and (ga is None or torch.equal(ga, gc))
    done = batch[4]
    assert torch.equal(q_hat[done], ag.scale * batch[2][done])  # terminal rows: reward_scale * r alone


def test_fused_targets_is_off_by_default_and_refused_where_the_kernel_cannot_run():
    ag = BatchedSACAgent(device="cpu", max_mem_size=64, batch_size=64)
    assert ag.fused_targets is False and ag._learn_calls == 0
    with pytest.raises(ValueError, match="fused_targets"):
        BatchedSACAgent(device="cpu", max_mem_size=64, batch_size=64, fused_targets=True)  # no GPU
    with pytest.raises(ValueError, match="fused_targets"):
        BatchedSACAgent(device="cpu", max_mem_size=256, batch_size=100, fused_targets=True)
    import inspect
    assert inspect.signature(BatchedSACAgent.__init__).parameters["fused_targets"].default is False
    assert inspect.signature(train_sac).parameters["fused_targets"].default is False
    assert list(inspect.signature(BatchedSACAgent.learn_on).parameters) == ["self", "batch", "noise_value", "noise_actor"]


def test_learn_calls_is_checkpointed_and_optional_on_load():
    ag, _, _, _ = _agent_and_batch(2)
    ag._learn_calls = 41
    sd = ag.state_dict()
    assert sd["learn_calls"] == 41
    other, _, _, _ = _agent_and_batch(2, seed=4)
    other.load_state_dict(sd)
    assert other._learn_calls == 41
    del sd["learn_calls"]
    other.load_state_dict(sd)  # a checkpoint from before the key
    assert other._learn_calls == 0


def test_cli_has_the_switch():
    import subprocess
    import sys
    run = subprocess.run([sys.executable, "-m", "roborugby_amd.sac", "--help"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "--fused-targets" in run.stdout
