"""roborugby_amd.sac on the GPU: BatchedSACAgent.choose_action through rr_sac_act next to the torch path on the same parameters, the row
counts that take the torch path, and train_sac end to end on presets T (A = 2) and G (A = 4), with a resume."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sac_ref  # noqa: E402
from roborugby_amd.sac import BatchedSACAgent, train_sac  # noqa: E402

DEV = "cuda:0"


def _agent(A, **kw):
    ag = BatchedSACAgent(n_actions=A, batch_size=64, max_mem_size=1024, device=DEV, seed=5, fused=True, **kw)
    with torch.no_grad():  # heads that take both arms of the clamp
        ag.actor.sigma.weight.mul_(8.0)
        ag.actor.sigma.bias.add_(0.5)
    return ag


@pytest.mark.parametrize("A", [2, 4])
def test_fused_choose_action_against_the_torch_paths_mu_and_sigma(A):
    ag = _agent(A)
    n = 64 * 5
    g = torch.Generator(device=DEV).manual_seed(A)
    obs = torch.rand(n, 11, generator=g, device=DEV) * 2 - 1
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    lp, head, noise = nan(n), nan(n, 2 * A), nan(n, A)
    ag._act_calls = 5
    chosen = ag.choose_action(obs)
    assert ag._act_calls == 6 and chosen.shape == (n, A) and chosen.dtype == torch.float32
    ag._act_calls = 5
    again = ag._act_fused(obs, False, lp, head, noise)  # the same call number: the same draws
    torch.cuda.synchronize()
    assert torch.equal(chosen, again)
    with torch.no_grad():
        mu32, raw32 = ag.actor.head(obs)
        _, sigma32 = ag.actor(obs)
    params = [p.detach().cpu().numpy() for p in ag.actor.parameters()]
    h64 = sac_ref.actor_head64(params, obs.cpu().numpy())
    t32 = torch.cat([mu32, raw32], 1).double().cpu().numpy()
    got = head.double().cpu().numpy()
    err, err32, scale = float(np.abs(got - h64).max()), float(np.abs(t32 - h64).max()), float(np.abs(h64).max())
    print(f"  A = {A}: fused head {err / scale:.2e}, torch fp32 forward {err32 / scale:.2e} of max |head| = {scale:.3g} (vs fp64 forward)")
    assert err <= max(1e-5 * scale, 1.25 * err32), (err, err32, scale)
    sig = np.clip(got[:, A:], 1e-6, 1.0)
    assert float(np.abs(sig - sigma32.double().cpu().numpy()).max()) <= err + err32  # each side carries its own forward's error
    assert (got[:, A:] < 1e-6).any() and (got[:, A:] > 1.0).any()
    # the returned actions are the squash of that head and those draws
    a64, lp64, _ = sac_ref.squash64(head.cpu().numpy(), noise.cpu().numpy(), ag.max_action)
    E_a, E_lp = sac_ref.squash_E(head.cpu().numpy(), noise.cpu().numpy(), ag.max_action)
    assert float(np.abs(chosen.cpu().numpy() - a64).max()) <= max(4 * E_a, 2.0 ** -22)
    rows = sac_ref.well_conditioned_rows(a64)
    assert float(np.abs(lp.cpu().numpy() - lp64)[rows].max()) <= 4 * E_lp
    # deterministic: tanh(mu), no call consumed twice
    det = ag.choose_action(obs, deterministic=True)
    assert float((det.double() - torch.tanh(mu32.double())).abs().max()) <= err + err32 + 2.0 ** -22
    ag.close()


def test_other_row_counts_and_layouts_take_the_torch_path():
    ag = _agent(2)
    obs = torch.rand(100, 11, device=DEV) * 2 - 1
    a = ag.choose_action(obs)
    assert ag._act_calls == 0 and a.shape == (100, 2) and a.dtype == torch.float32 and bool((a.abs() <= 1).all())
    wide = torch.rand(128, 22, device=DEV)[:, ::2]  # 128 rows, not contiguous
    assert ag.choose_action(wide).shape == (128, 2) and ag._act_calls == 0
    assert ag.choose_action(wide.contiguous()).shape == (128, 2) and ag._act_calls == 1
    off = BatchedSACAgent(n_actions=2, batch_size=64, max_mem_size=1024, device=DEV, seed=5, fused=False)
    assert off._dqn is None and off.choose_action(wide.contiguous()).shape == (128, 2) and off._act_calls == 0
    ag.close()


@pytest.mark.parametrize("preset,A", [("T", 2), ("G", 4)])
def test_train_sac_runs_and_counts_its_transitions(preset, A, tmp_path):
    ck = str(tmp_path / "sac.pt")
    res = train_sac(num_envs=256, steps=30, batch_size=64, preset=preset, mem_size=16384, checkpoint=ck, log_every=0, seed=3, fused=True)
    assert res["n_actions"] == A and res["fused_act"] is True and res["preset"] == preset and res["mode"] == "train_sac"
    assert res["mem_cntr"] == res["transitions"] and 0 < res["transitions"] <= 256 * 30
    assert res["act_calls"] == 30 and res["learn_calls"] == 30
    for k in ("value_loss", "actor_loss", "critic_loss"):
        assert res[k] is not None and np.isfinite(res[k]), k
    # a resumed agent continues the call counter (and the env its episodes)
    res2 = train_sac(num_envs=256, steps=10, batch_size=64, preset=preset, mem_size=16384, resume=ck, log_every=0, seed=3, fused=True)
    assert res2["act_calls"] == 40 and res2["learn_calls"] == 30 + 10
    assert res2["mem_cntr"] == res2["transitions"]
    for k in ("value_loss", "actor_loss", "critic_loss"):
        assert np.isfinite(res2[k]), k


def test_train_sac_refuses_a_step_budget():
    with pytest.raises(ValueError, match="budget"):
        train_sac(num_envs=64, steps=1, step_budget_clocks=1000)
