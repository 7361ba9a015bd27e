"""tests/sac_grads_ref.py held to its own yardsticks, without a GPU: the float64 restatement of the value and critic gradients of Agent.learn
(i) against the reference trainer's own float64 run (tests/golden/sac_learn.npz, width 32 -- the restatement is width-agnostic), (ii)
against torch float64 autograd of BatchedSACAgent.losses_given_targets at width 256, and (iii) the conditions the GPU tests' inputs
(case(A)) must meet for those tests to mean what they say.  The bar of (i) and (ii) is float64 agreement: err <= 1e-9 * scale per tensor,
scale = max |reference value| (two float64 evaluations of one formula in different summation orders differ by ~1e-13 of scale here)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sac_grads_ref as gr  # noqa: E402
import sac_targets_ref as tr  # noqa: E402
from test_agent_reference import ACTOR_KEYS, fixture  # noqa: E402

CASES = tuple(fixture("sac_learn.npz")[1]["cases"])
OUT = {"critic_1": "q", "critic_2": "q", "value": "v", "target_value": "v"}


def _agree64(label, got, ref):
    ref = np.asarray(ref, np.float64)
    scale, err = float(np.abs(ref).max()), float(np.abs(np.asarray(got, np.float64) - ref).max())
    print(f"  {label}: err {err / scale:.2e} of scale {scale:.3g}")
    assert scale > 0 and err <= 1e-9 * scale, (label, err, scale)


def _names(net):
    return ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", f"{OUT[net]}.weight", f"{OUT[net]}.bias")


def test_there_are_four_cases():
    assert len(CASES) == 4


@pytest.mark.parametrize("case", CASES)
def test_grads64_reproduces_the_reference_learn(case):
    fx, meta = fixture("sac_learn.npz")
    hp = meta["hyper"]
    nets = {net: tuple(fx[f"{case}.w.{net}.{k}"] for k in _names(net)) for net in OUT}
    nets["actor"] = tuple(fx[f"{case}.w.actor.{k}"] for k in ACTOR_KEYS)
    state, action, reward, new_state, done = (fx[f"{case}.{k}"] for k in ("state", "action", "reward", "new_state", "done"))
    t = tr.targets64(nets, (state, new_state, action, reward, done), np.arange(state.shape[0]), fx[f"{case}.noise_value"], hp["gamma"],
                     hp["reward_scale"], meta["max_action"])
    got = gr.grads64(nets, state, action, t["value_target"], t["q_hat"])
    for net in gr.NETS:
        for k, g in zip(_names(net), got[net]["grads"]):
            _agree64(f"{case} {net}.{k}", g, fx[f"{case}.g64.{net}.{k}"])
    ref = fx[f"{case}.losses64"]
    _agree64(f"{case} value_loss", got["value"]["loss"], ref[0])
    _agree64(f"{case} critic_loss", got["critic_1"]["loss"] + got["critic_2"]["loss"], ref[2])  # the critic loss is the sum of two


@pytest.mark.parametrize("A", [2, 4])
def test_grads64_is_float64_autograd_of_the_agents_losses(A):
    from roborugby_amd.sac import BatchedSACAgent
    nets, state, action, value_target, q_hat = gr.case(A)
    B = 640
    ag = BatchedSACAgent(n_actions=A, max_mem_size=64, batch_size=64, device="cpu", seed=0, fused=False)
    for name in gr.NETS:
        module = getattr(ag, name)
        module.load_state_dict({k: torch.from_numpy(p.copy()) for k, p in zip(module.state_dict(), nets[name])})
    for module in (ag.actor, ag.value, ag.critic_1, ag.critic_2):
        module.double()
    t64 = lambda a: torch.from_numpy(np.asarray(a[:B], np.float64))
    noise_actor = torch.zeros(B, A, dtype=torch.float64)
    value_loss, _, critic_loss = ag.losses_given_targets(t64(state), t64(action), t64(value_target), t64(q_hat), noise_actor)
    got = gr.case_grads64(A, B)
    for loss, names in ((value_loss, ("value",)), (critic_loss, ("critic_1", "critic_2"))):
        params = [p for n in names for p in getattr(ag, n).parameters()]
        auto = iter(torch.autograd.grad(loss, params))
        for n in names:
            for (k, _p), g in zip(getattr(ag, n).named_parameters(), got[n]["grads"]):
                _agree64(f"A = {A} {n}.{k}", g, next(auto).numpy())
    _agree64(f"A = {A} value_loss", got["value"]["loss"], float(value_loss.detach()))
    _agree64(f"A = {A} critic_loss", got["critic_1"]["loss"] + got["critic_2"]["loss"], float(critic_loss.detach()))
    ag.close()


@pytest.mark.parametrize("A", [2, 4])
@pytest.mark.parametrize("B", [64, 128, 320, 448, 576, 64 * 257])
def test_case_conditions(A, B):
    """on every prefix the GPU tests take: 64, 320, 448, 576 and 64 * (CUs + 1) = 16,448 rows in tests/test_gpu_sac_grads.py, 128 in
    tests/test_gpu_sac_grads_agent.py"""
    nets, state, action, value_target, q_hat = gr.case(A)
    assert state.shape == (gr.sac_ref.CASE_ROWS, 11) and action.shape == (gr.sac_ref.CASE_ROWS, A) and gr.sac_ref.CASE_ROWS >= 64 * 257
    assert nets["value"][0].shape == (256, 11) and nets["critic_1"][0].shape == nets["critic_2"][0].shape == (256, 11 + A)
    assert all(nets[n][4].shape == (1, 256) and nets[n][2].shape == (256, 256) for n in gr.NETS)
    assert np.abs(action).max() <= 1.0
    got = gr.case_grads64(A, B)
    for n, y in (("value", value_target[:B]), ("critic_1", q_hat[:B]), ("critic_2", q_hat[:B])):
        for k, g in zip(gr.KEYS, got[n]["grads"]):
            assert np.all(np.isfinite(g)) and np.abs(g).max() > 0, (n, k)  # a non-zero scale for every tensor's bar
        for layer in ("h1", "h2"):
            h = got[n][layer]
            assert np.any(h > 0) and np.any(h == 0), (n, layer)  # both arms of relu'
        assert np.all(got[n]["f"] != y), n  # the target differs from the output on every row
        assert got[n]["loss"] > 0
