"""BatchedSACAgent with fused_grads on the MI355X: two agents from one seed and one state that differ in fused_grads alone (fused_targets
on both), a 128-row batch stored through remember(), one learn_on().  The float64 truth is CPU autograd of losses_given_targets on the
same rows and targets; E is the error of the unfused agent's float32 autograd against it.  The bars are the project's
(tests/test_agent_reference.py): gradients err <= max(1e-5 * scale, 1.25 * E); parameters after the step check_sac_step's rule against a
float64 Adam first step on the float64 gradients."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sac_grads_ref as gr  # noqa: E402
import sac_targets_ref as tr  # noqa: E402
from roborugby_amd.sac import BatchedSACAgent, train_sac  # noqa: E402

DEV = "cuda:0"
B = 128
TRAINED = ("actor", "critic_1", "critic_2", "value")


def _load_case(ag, A):
    """the actor, critics and target value net of tests/sac_targets_ref.py's case, the value net of tests/sac_grads_ref.py's"""
    nets, _, _ = tr.case(A)
    nets = dict(nets, value=gr.case(A)[0]["value"])
    with torch.no_grad():
        for name in ("actor", "critic_1", "critic_2", "target_value", "value"):
            for p, v in zip(getattr(ag, name).parameters(), nets[name]):
                p.copy_(torch.as_tensor(v.copy()))


def _agent(A, fused_grads, device=DEV, **kw):
    ag = BatchedSACAgent(n_actions=A, batch_size=B, max_mem_size=512, device=device, seed=5, fused_targets=device != "cpu",
                         fused_grads=fused_grads, **kw)
    _load_case(ag, A)
    return ag


@pytest.fixture(scope="module", params=[2, 4])
def step(request):
    """one learn_on() of the fused and of the torch agent on the same batch and draws, and the float64 truth: computed once per A"""
    A = request.param
    _, rings, _ = tr.case(A)
    dev = [torch.as_tensor(r[:B].copy()).to(DEV) for r in rings]
    fused, plain = _agent(A, True), _agent(A, False)
    for ag in (fused, plain):
        ag.remember(dev[0][:100], dev[2][:100], dev[3][:100], dev[1][:100], dev[4][:100])
        ag.remember(dev[0][100:], dev[2][100:], dev[3][100:], dev[1][100:], dev[4][100:])
        assert ag.mem_cntr == B
    g = torch.Generator(device=DEV).manual_seed(11)
    noise_value, noise_actor = torch.randn((B, A), generator=g, device=DEV), torch.randn((B, A), generator=g, device=DEV)
    before = {n: [p.detach().clone() for p in getattr(fused, n).parameters()] for n in TRAINED + ("target_value",)}
    batch = lambda ag: (ag.state_memory[:B], ag.action_memory[:B], ag.reward_memory[:B], ag.new_state_memory[:B], ag.terminal_memory[:B])
    value_target, q_hat = fused.targets(batch(fused), noise_value)  # the targets both agents' learn_on computes (the torch path's)
    # ---- the float64 truth: CPU autograd of losses_given_targets on the same rows and targets, before anything steps
    cpu = BatchedSACAgent(n_actions=A, batch_size=B, max_mem_size=64, device="cpu", seed=5, fused=False)
    _load_case(cpu, A)
    for n in TRAINED:
        getattr(cpu, n).double()
    d64 = lambda t: t.detach().cpu().double()
    losses64 = cpu.losses_given_targets(d64(fused.state_memory[:B]), d64(fused.action_memory[:B]), d64(value_target), d64(q_hat), d64(noise_actor))
    g64 = {}
    for loss, names in zip(losses64, (("value",), ("actor",), ("critic_1", "critic_2"))):
        got = iter(torch.autograd.grad(loss, [p for n in names for p in getattr(cpu, n).parameters()], retain_graph=True))
        for n in names:
            g64[n] = [next(got).numpy() for _ in getattr(cpu, n).parameters()]
    cpu.close()
    out = dict(A=A, fused=fused, plain=plain, before=before, g64=g64, losses64=[float(x.detach()) for x in losses64])
    out["losses_fused"] = fused.learn_on(batch(fused), noise_value, noise_actor)
    out["losses_plain"] = plain.learn_on(batch(plain), noise_value, noise_actor)
    torch.cuda.synchronize()
    yield out
    fused.close()
    plain.close()


def test_the_gradients_meet_the_bar(step):
    fused, plain, A = step["fused"], step["plain"], step["A"]
    assert fused.fused_grads is True and plain.fused_grads is False and fused.fused_targets and plain.fused_targets
    for n in TRAINED:  # the actor's too: its path is unchanged
        for (k, p), q, ref in zip(getattr(fused, n).named_parameters(), getattr(plain, n).parameters(), step["g64"][n]):
            scale = float(np.abs(ref).max())
            err = float(np.abs(p.grad.cpu().numpy() - ref).max())
            E = float(np.abs(q.grad.cpu().numpy() - ref).max())
            print(f"  A = {A} {n}.{k}: err {err / scale:.2e}, E {E / scale:.2e} of scale {scale:.3g}")
            assert scale > 0 and bool(torch.isfinite(p.grad).all()) and err <= max(1e-5 * scale, 1.25 * E), (n, k, err, E, scale)


def test_the_losses_agree_with_the_torch_agent(step):
    assert step["fused"].last_losses is step["losses_fused"] and len(step["losses_fused"]) == 3
    for name, a, b, ref in zip(("value_loss", "actor_loss", "critic_loss"), step["losses_fused"], step["losses_plain"], step["losses64"]):
        scale = abs(ref)
        print(f"  A = {step['A']} {name}: fused {float(a):.9g}, torch {float(b):.9g}, float64 {ref:.9g}")
        assert a.shape == () and abs(float(a) - float(b)) <= 1e-5 * scale, name


def test_the_parameters_after_the_step(step):
    """check_sac_step's rule against a float64 Adam first step (p - lr * g / (|g| + eps)) on the float64 gradients"""
    fused, A = step["fused"], step["A"]
    assert fused.updates == 1
    for n in TRAINED:
        opt = fused.actor_optimizer if n == "actor" else fused.value_optimizer if n == "value" else fused.critic_optimizer
        lr, eps = opt.param_groups[0]["lr"], opt.param_groups[0]["eps"]
        for (k, p), old, g in zip(getattr(fused, n).named_parameters(), step["before"][n], step["g64"][n]):
            p64 = old.cpu().numpy().astype(np.float64) - lr * g / (np.abs(g) + eps)
            p = p.detach().cpu().numpy().astype(np.float64)
            well = np.abs(g) >= 1e-3 * np.abs(g).max()
            d, ulp = np.abs(p - p64), 2.0 ** -23 * np.abs(p)
            print(f"  A = {A} {n}.{k}: well-conditioned {well.mean():.3f}, there max |p - p64| {d[well].max() / lr:.2e} lr; anywhere {d.max() / lr:.2e} lr")
            assert well.mean() >= 0.70, (n, k)
            assert np.all(d[well] <= 1e-3 * lr + ulp[well]), (n, k, float((d - ulp)[well].max()) / lr)
            assert np.all(d <= 2 * lr + ulp), (n, k, float((d - ulp).max()) / lr)


def test_the_soft_update_follows_the_value_step(step):
    fused = step["fused"]
    for pt, pv, old in zip(fused.target_value.parameters(), fused.value.parameters(), step["before"]["target_value"]):
        want = old.clone().mul_(1.0 - fused.tau).add_(pv.detach(), alpha=fused.tau)  # tau * value_new + (1 - tau) * target_old
        assert torch.equal(pt.detach(), want) and not torch.equal(pt.detach(), old)


def test_a_checkpoint_crosses_between_fused_and_unfused(step, tmp_path):
    fused, A = step["fused"], step["A"]
    ck = str(tmp_path / "fused.pt")
    torch.save(fused.state_dict(), ck)
    other = BatchedSACAgent(n_actions=A, batch_size=B, max_mem_size=512, device=DEV, seed=9)
    other.load_state_dict(torch.load(ck, map_location=DEV))
    assert other.updates == 1 and other.fused_grads is False
    for n in TRAINED + ("target_value",):
        assert all(torch.equal(p, q) for p, q in zip(getattr(fused, n).parameters(), getattr(other, n).parameters())), n
    back = str(tmp_path / "unfused.pt")
    torch.save(other.state_dict(), back)
    again = BatchedSACAgent(n_actions=A, batch_size=B, max_mem_size=512, device=DEV, seed=3, fused_targets=True, fused_grads=True)
    again.load_state_dict(torch.load(back, map_location=DEV))
    for n in TRAINED + ("target_value",):
        assert all(torch.equal(p, q) for p, q in zip(getattr(fused, n).parameters(), getattr(again, n).parameters())), n
    moments = lambda ag: [v for o in (ag.actor_optimizer, ag.value_optimizer, ag.critic_optimizer) for s in o.state_dict()["state"].values()
                          for v in (s["exp_avg"], s["exp_avg_sq"])]
    assert len(moments(again)) == len(moments(fused)) > 0 and all(torch.equal(x, y) for x, y in zip(moments(again), moments(fused)))
    other.close()
    again.close()


def test_grads_fused_returns_the_buffers_and_learn_runs(step):
    """grads_fused on an agent of its own (the fixture's have stepped): per net one tensor per parameter, and the three losses; then
    learn() end to end with both kernels"""
    A = step["A"]
    ag = _agent(A, True)
    nets, state, action, value_target, q_hat = gr.case(A)
    dev = lambda x: torch.as_tensor(x[:B].copy()).to(DEV)
    grads, loss = ag.grads_fused(dev(state), dev(action), dev(value_target), dev(q_hat))
    assert len(grads) == 3 and loss.shape == (3,)
    for gs, n in zip(grads, gr.NETS):
        assert [tuple(g.shape) for g in gs] == [tuple(p.shape) for p in getattr(ag, n).parameters()]
    ref = gr.case_grads64(A, B)["value"]  # the value net is sac_grads_ref's: its gradient on these rows is known
    for g, want in zip(grads[0], ref["grads"]):
        assert float(np.abs(g.cpu().numpy() - want).max()) <= 1e-4 * float(np.abs(want).max())
    assert abs(float(loss[0]) - ref["loss"]) <= 1e-5 * ref["loss"]
    _, rings, _ = tr.case(A)
    r = [torch.as_tensor(x[:B].copy()).to(DEV) for x in rings]
    ag.remember(r[0], r[2], r[3], r[1], r[4])
    losses = ag.learn()
    assert losses is not None and all(bool(torch.isfinite(x)) for x in losses) and ag.updates == 1 and ag._learn_calls == 1
    ag.close()


def test_construction_rules():
    with pytest.raises(ValueError, match="multiple of 64"):
        BatchedSACAgent(device=DEV, max_mem_size=256, batch_size=100, fused_grads=True)
    with pytest.raises(ValueError, match="fused_grads"):
        BatchedSACAgent(device=DEV, max_mem_size=256, batch_size=64, fc1_dims=128, fused=False, fused_grads=True)
    ag = BatchedSACAgent(device=DEV, max_mem_size=256, batch_size=64, fused_grads=True)  # works with fused_targets off
    assert ag.fused_grads is True and ag.fused_targets is False
    ag.close()


def test_train_sac_with_fused_grads():
    res = train_sac(num_envs=64, steps=3, batch_size=64, preset="T", fused_targets=True, fused_grads=True, log_every=0, mem_size=4096, seed=3)
    assert res["fused_grads"] is True and res["fused_targets"] is True and res["learn_calls"] == 3
    for k in ("value_loss", "actor_loss", "critic_loss"):
        assert res[k] is not None and np.isfinite(res[k]), k
    off = train_sac(num_envs=64, steps=2, batch_size=64, preset="T", log_every=0, mem_size=4096, seed=3)
    assert off["fused_grads"] is False
