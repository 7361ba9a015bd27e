"""BatchedSACAgent with fused_targets on the MI355X: targets through rr_sac_targets against the torch path of the same agent on a replay
filled through remember(), one learn() step, the checkpointed call counter, and train_sac end to end on presets T (A = 2) and G (A = 4)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sac_ref  # noqa: E402
import sac_targets_ref as tr  # noqa: E402
from roborugby_amd.sac import BatchedSACAgent, train_sac  # noqa: E402

DEV = "cuda:0"


def _filled_agent(A, B=128, rows=300, seed=5, **kw):
    """an agent whose actor and critics are tests/sac_targets_ref.py's case (sigma's clamp is taken both ways) and whose replay holds
    the case's `rows` transitions, stored in two remember() calls"""
    nets, rings, _ = tr.case(A)
    ag = BatchedSACAgent(n_actions=A, batch_size=B, max_mem_size=512, device=DEV, seed=seed, fused_targets=True, **kw)
    with torch.no_grad():
        for name in ("actor", "critic_1", "critic_2", "target_value"):
            for p, v in zip(getattr(ag, name).parameters(), nets[name]):
                p.copy_(torch.as_tensor(v.copy()))
    dev = [torch.as_tensor(r.copy()).to(DEV) for r in rings]
    for lo, hi in ((0, 200), (200, rows)):
        ag.remember(dev[0][lo:hi], dev[2][lo:hi], dev[3][lo:hi], dev[1][lo:hi], dev[4][lo:hi])
    assert ag.mem_cntr == rows
    return ag


@pytest.mark.parametrize("A", [2, 4])
def test_fused_targets_agree_with_the_torch_path(A):
    ag = _filled_agent(A)
    nets, rings, index = tr.case(A)
    B = ag.batch_size
    idx = torch.as_tensor(index[:B].copy()).to(DEV)
    noise = torch.as_tensor(tr.draw32(2, B, 7)[:, :A].copy()).to(DEV)
    win = {k: torch.full(s, float("nan"), device=DEV) for k, s in (("q1", (B,)), ("q2", (B,)), ("log_prob", (B,)), ("v_next", (B,)),
                                                                   ("policy_action", (B, A)))}
    vt, qh, state, action = ag.targets_fused(idx, noise, **win)
    batch = (ag.state_memory[idx], ag.action_memory[idx], ag.reward_memory[idx], ag.new_state_memory[idx], ag.terminal_memory[idx])
    vt_t, qh_t = ag.targets(batch, noise)
    assert torch.equal(state, batch[0]) and torch.equal(action, batch[1])
    # the float64 truth of both, and the torch path's own error as the yardstick (test_gpu_sac_targets.py's bars)
    t64 = tr.targets64(nets, rings, index[:B], noise.cpu().numpy(), ag.gamma, ag.scale, ag.max_action)
    well = sac_ref.well_conditioned_rows(t64["policy_action"], ag.max_action)
    assert well.mean() >= 0.9
    for label, got, torch_path, key in (("value_target", vt, vt_t, "value_target"), ("q_hat", qh, qh_t, "q_hat")):
        ref = t64[key]
        rows = well if key == "value_target" else np.ones(B, bool)
        err = float(np.abs(got.cpu().numpy() - ref)[rows].max())
        err32 = float(np.abs(torch_path.cpu().numpy() - ref)[rows].max())
        scale = float(np.abs(ref[rows]).max())
        print(f"  A = {A} {label}: fused err {err / scale:.2e}, torch path {err32 / scale:.2e} of scale {scale:.3g} (vs float64)")
        assert np.all(np.isfinite(got.cpu().numpy()))
        assert err <= max(1e-5 * scale, 1.25 * err32), (label, err, err32, scale)
    done = batch[4]
    assert bool(done.any()) and torch.equal(qh[done], torch.tensor(ag.scale, device=DEV) * batch[2][done])
    ag.close()


def test_construction_rules():
    with pytest.raises(ValueError, match="multiple of 64"):
        BatchedSACAgent(device=DEV, max_mem_size=256, batch_size=100, fused_targets=True)
    with pytest.raises(ValueError, match="fused_targets"):
        BatchedSACAgent(device=DEV, max_mem_size=256, batch_size=64, fc1_dims=128, fused=False, fused_targets=True)
    ag = BatchedSACAgent(device=DEV, max_mem_size=256, batch_size=64)
    assert ag.fused_targets is False and ag.fused is True
    ag.close()


@pytest.mark.parametrize("A", [2, 4])
def test_one_learn_step(A, tmp_path):
    ag = _filled_agent(A, B=64)
    trained = ("actor", "critic_1", "critic_2", "value")
    before = {n: [p.detach().clone() for p in getattr(ag, n).parameters()] for n in trained + ("target_value",)}
    gen_state = ag.gen.get_state()
    losses = ag.learn()
    assert losses is not None and all(bool(torch.isfinite(x)) for x in losses)
    assert ag._learn_calls == 1 and ag.updates == 1
    for n in trained:
        assert all(not torch.equal(p, q) for p, q in zip(getattr(ag, n).parameters(), before[n])), n
    for pt, pv, old in zip(ag.target_value.parameters(), ag.value.parameters(), before["target_value"]):
        want = old * (1.0 - ag.tau) + ag.tau * pv.detach()
        assert torch.allclose(pt, want, rtol=0, atol=2.0 ** -22 * float(want.abs().max())) and not torch.equal(pt, old)
    # the generator gave the batch rows and the actor loss's noise, not the value target's: one randint and ONE randn
    g = torch.Generator(device=DEV)
    g.set_state(gen_state)
    torch.randint(0, 300, (64,), generator=g, device=DEV)
    torch.randn((64, A), generator=g, device=DEV)
    assert torch.equal(g.get_state(), ag.gen.get_state())
    ck = str(tmp_path / "agent.pt")
    torch.save(ag.state_dict(), ck)
    other = BatchedSACAgent(n_actions=A, batch_size=64, max_mem_size=512, device=DEV, seed=9, fused_targets=True)
    other.load_state_dict(torch.load(ck, map_location=DEV))
    assert other._learn_calls == 1 and other.updates == 1
    for n in trained + ("target_value",):
        assert all(torch.equal(p, q) for p, q in zip(getattr(ag, n).parameters(), getattr(other, n).parameters())), n
    ag.close()
    other.close()


@pytest.mark.parametrize("preset,A", [("T", 2), ("G", 4)])
def test_train_sac_with_fused_targets(preset, A):
    res = train_sac(num_envs=64, steps=4, batch_size=64, preset=preset, fused_targets=True, log_every=0, mem_size=4096, seed=3)
    assert res["fused_targets"] is True and res["n_actions"] == A and res["mode"] == "train_sac"
    # learn() runs once per step from the step at which the replay holds a batch: 64 arenas store at most 64 rows a step, and the rows
    # of step 1 are all transitions (no arena has been reset yet), so every step learns
    assert res["mem_cntr"] == res["transitions"]
    assert res["transitions"] == 64 * 4 and res["learn_calls"] == 4 and res["target_syncs"] == 4  # (learn_calls: the agent's updates)
    for k in ("value_loss", "actor_loss", "critic_loss"):
        assert res[k] is not None and np.isfinite(res[k]), k
    off = train_sac(num_envs=64, steps=2, batch_size=64, preset=preset, log_every=0, mem_size=4096, seed=3)
    assert off["fused_targets"] is False
