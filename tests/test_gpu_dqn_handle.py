"""The one owner of an rr_dqn handle (_lib.DqnHandle) under its three users: a players.Hive that borrows a fused agent's handle acts as
one that owns its own, closing the borrower leaves the agent's handle alone, close() may be called twice everywhere, and fused=True
without a GPU is refused before anything is created."""
import pytest

torch = pytest.importorskip("torch")

DEV = "cuda:0"


@pytest.mark.gpu
def test_borrowed_and_owned_handles_agree_and_only_the_owner_destroys():
    import roborugby_amd as rr
    from roborugby_amd.dqn import BatchedDQNAgent
    from roborugby_amd.players import Hive
    agent = BatchedDQNAgent(device=DEV, seed=3, batch_size=64, max_mem_size=64)
    assert agent.fused and agent._fused_h
    envs = [rr.BatchedRoboRugbyEnv(64, preset="G", device=DEV, seed=9, action_mode="thrust") for _ in range(2)]
    borrower = Hive(envs[0], agent, robots=range(4), epsilon=0.3, seed=4)
    owner = Hive(envs[1], [p.detach() for p in agent.Q_eval.parameters()], robots=range(4), epsilon=0.3, seed=4)
    assert borrower._dqn_h.value == agent._fused_h.value and owner._dqn_h.value not in (None, agent._fused_h.value)
    for env in envs:
        env.reset()
    drawn = 0
    for k in range(3):
        for hive, env in ((borrower, envs[0]), (owner, envs[1])):
            env.step_thrust(hive.act())
        torch.cuda.synchronize()
        assert torch.equal(borrower.assign, owner.assign) and torch.equal(borrower.actions, owner.actions), k
        assert borrower.calls == owner.calls == k + 1
        with torch.no_grad():
            greedy = agent.Q_eval(borrower.obs.reshape(-1, 11)).argmax(dim=1).view(64, 4)
        drawn += int(((borrower.actions != greedy) & (borrower.assign >= 0)).sum())
    assert drawn > 0  # (epsilon 0.3 over 768 rows: the two agreed on draws, not only on greedy answers)
    # closing the borrower: the handle is the agent's
    borrower.close()
    assert agent._fused_h and borrower._dqn_h.value == agent._fused_h.value
    acts = agent.choose_action(torch.rand(64, 11, device=DEV))
    torch.cuda.synchronize()
    assert acts.dtype == torch.int32 and tuple(acts.shape) == (64,) and 0 <= int(acts.min()) and int(acts.max()) <= 7
    assert agent._act_calls == 1  # (the fused kernel answered)
    # closing twice
    for thing in (owner, agent):
        thing.close()
        thing.close()
    assert owner._dqn_h is None and agent._fused_h is None
    for env in envs:
        env.close()


@pytest.mark.gpu
def test_closing_a_fused_pixel_agent_twice():
    from roborugby_amd.dqn import PixelDQNAgent
    ag = PixelDQNAgent(channels=3, batch_size=8, max_mem_size=8, device=DEV, fused=True)
    assert ag._fused_h
    ag.close()
    ag.close()
    assert ag._fused_h is None


@pytest.mark.parametrize("name,kw", [("BatchedDQNAgent", dict(batch_size=64, max_mem_size=64)),
                                     ("PixelDQNAgent", dict(channels=3, batch_size=8, max_mem_size=8))])
def test_fused_without_a_gpu_is_refused_and_leaves_nothing_to_destroy(name, kw):
    from roborugby_amd import dqn
    made = []

    class Probe(getattr(dqn, name)):
        def __init__(self, *a, **k):
            made.append(self)
            super().__init__(*a, **k)

    with pytest.raises(ValueError, match="fused=True needs a GPU"):
        Probe(device="cpu", fused=True, **kw)
    assert made[0]._fused_h is None
    made[0].close()  # (what __del__ does)
    assert made[0]._fused_h is None
    assert getattr(dqn, name)(device="cpu", **kw)._fused_h is None  # fused=None: off without a GPU
