"""The agents' kernels against the reference trainers' own programs, on the device: rr_sac_act against what the reference's
ActorNetwork.sample_normal returned, rr_dqn_grads against the gradient the reference's DQNAgent.learn left behind, both through the C
ABI, and the SAC losses' gradients and first step (autograd on the device, no kernel of ours) -- all from tests/golden/sac_act.npz,
dqn_learn.npz and sac_learn.npz (oracle/refgen/gen_agents.py: the float64 run of the unmodified trainers on given rows and given
draws).  tests/test_agent_reference.py states the bars and holds the torch paths and the restatements to the same files without a GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sac_ref  # noqa: E402
import test_agent_reference as ar  # noqa: E402
from test_gpu_dqn_kernels import _grads_flat, _split  # noqa: E402
from test_gpu_sac_act import Handle, _written_exactly  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def handle():
    h = Handle()
    yield h
    h.close()


@pytest.mark.parametrize("case", ar.ACT_CASES)
def test_rr_sac_act_matches_the_reference_sample_normal(handle, case):
    """The kernel draws its own z, so it cannot be handed the fixture's (sac_ref.draw32 of the same seed and call): with dz = |noise - z|
    per component, dz <= 4 E_z is required (E_z = draw32's error against draw64 on these rows: the existing noise rule), and the bars
    of the actions and of the log-probability grow by what dz can move them:
      actions    a = max_action * tanh(mu + sigma z): |da/dz| = max_action * sigma * (1 - tanh^2) <= max_action, so + max_action * dz;
      log_prob   component k's term is t(z) = -z^2 / 2 - log sigma - log(2 pi) / 2 - log(1 - a^2 + 1e-6), and
                 dt/dz = -z + 2 a (da/dz) / (1 - a^2 + 1e-6).  With m = max_action <= 1 and th = tanh(mu + sigma z):
                 da/dz = m sigma (1 - th^2) and 1 - th^2 <= 1 - m^2 th^2 + 1e-6 = 1 - a^2 + 1e-6, so the second term is at most
                 2 |a| m sigma <= 2 sigma <= 2: |dt/dz| <= |z| + 2, hence + sum_k (|z_k| + 2) dz_k (to first order in dz ~ 1e-7).
    The head -- mu and the raw sigma outputs before the clamp -- is held to the float64 run's under the hidden layers' usual rule, with
    the reference's own float32 run as err32."""
    c = ar.act_case(case)
    n, A = len(c["obs"]), c["A"]
    assert c["max_action"] <= 1.0 and n % 64 == 0
    params = [torch.from_numpy(p.copy()).to(DEV).contiguous() for p in c["params"]]
    obs = torch.from_numpy(c["obs"].copy()).to(DEV).contiguous()
    out = handle.act(params, obs, n, A, max_action=c["max_action"], seed=c["seed"], call=c["call"])
    _written_exactly(case, out, n)
    E_z = float(np.abs(c["z"].astype(np.float64) - sac_ref.draw64(c["seed"], n, c["call"])[:, :A]).max())
    dz = np.abs(out["noise"][:n].astype(np.float64) - c["z"])
    print(f"  rr_sac_act {case}: max |noise - z| {dz.max():.3g} (E_z {E_z:.3g}, bar {4 * E_z:.3g})")
    assert np.all(dz <= 4 * E_z), (case, float(dz.max()), E_z)
    ar.assert_within_E(f"rr_sac_act {case} head", out["head"][:n], c["head64"], c["E_head"])
    ar.assert_act(f"rr_sac_act {case}", c, out["actions"][:n], out["log_prob"][:n], slack_a=c["max_action"] * dz,
                  slack_lp=((np.abs(c["z"].astype(np.float64)) + 2.0) * dz).sum(1))
    assert np.all(np.abs(out["actions"][:n]) <= c["max_action"])


@pytest.mark.parametrize("wgs", [None, 1], ids=["default-grid", "wgs1"])
def test_rr_dqn_grads_matches_the_reference_learn(monkeypatch, wgs):
    if wgs is None:
        monkeypatch.delenv("RR_DQN_WGS", raising=False)
    else:
        monkeypatch.setenv("RR_DQN_WGS", str(wgs))  # read by getenv in rr_dqn_create
    ag = ar.dqn_agent(device=DEV, fused=None)
    assert ag.fused
    flat, loss = _grads_flat(ag, torch.arange(ag.batch_size, device=DEV))
    ar.assert_dqn_gradient(f"rr_dqn_grads WGS={wgs}", {k: v.cpu().numpy() for k, v in _split(ag, flat).items()}, loss)
    ag.close()


@pytest.mark.parametrize("case", ar.SAC_CASES)
def test_sac_gradients_on_the_device_match_the_reference_learn(case):
    ar.check_sac_gradients(case, DEV)


@pytest.mark.parametrize("case", ar.SAC_CASES)
def test_sac_parameters_after_learn_on_on_the_device_match_the_reference_learn(case):
    ar.check_sac_step(case, DEV)
