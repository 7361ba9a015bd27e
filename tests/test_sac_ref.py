"""tests/sac_ref.py held to facts, without a GPU: the draw's layout and moments, the log-probability against torch.distributions, the
float32 restatement's distance from the float64 formulas, and the conditions the GPU tests' inputs were built for."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dqn_ref  # noqa: E402
import sac_ref  # noqa: E402


def test_the_draw_is_the_act_streams_layout_with_another_stream_word():
    seed, call, row = 0x1234ABCD00000002, 7, 5
    w = sac_ref.words(seed, 8, call)
    one = dqn_ref.philox4x32_10((row, call, 0x5AC7, 0), (seed & 0xFFFFFFFF, seed >> 32))
    assert tuple(int(x[row]) for x in w) == one
    assert sac_ref.SAC_STREAM != dqn_ref.ACT_STREAM
    u1, u2 = sac_ref.uniforms(w[0], w[1])
    assert u1[row] == ((one[0] >> 8) + 1) / 2 ** 24 and u2[row] == (one[1] >> 8) / 2 ** 24


@pytest.mark.parametrize("seed,call,n", sac_ref.DRAW_SEEDS)
def test_draw_moments_and_ranges(seed, call, n):
    u = sac_ref.row_uniforms(seed, n, call)
    assert u[:, :, 0].min() > 0.0 and u[:, :, 0].max() <= 1.0      # u1 is never 0: log(u1) is finite
    assert u[:, :, 1].min() >= 0.0 and u[:, :, 1].max() < 1.0
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)  # exact in float32
    z = sac_ref.draw64(seed, n, call)
    m = z.size
    print(f"seed {seed:#x} call {call} n {n}: mean {z.mean():.4f} variance {z.var():.4f}")
    assert np.all(np.isfinite(z))
    assert abs(z.mean()) <= 5.0 / math.sqrt(m)
    assert abs(z.var() - 1.0) <= 5.0 * math.sqrt(2.0 / m)
    for k in range(4):  # every component on its own as well, and no pair of them moves together
        assert abs(z[:, k].mean()) <= 5.0 / math.sqrt(n)
    c = np.corrcoef(z.T)
    assert np.abs(c - np.eye(4)).max() <= 5.0 / math.sqrt(n)


def test_seed_high_word_and_call_change_the_draws():
    base = sac_ref.draw64(2, 256, 7)
    assert not np.array_equal(base, sac_ref.draw64(2 + (1 << 32), 256, 7))
    assert not np.array_equal(base, sac_ref.draw64(2, 256, 8))
    assert np.array_equal(base, sac_ref.draw64(2, 256, 7 + (1 << 32)))  # the call counter is its low 32 bits


def test_float32_restatement_of_the_draw_is_close():
    for seed, call, n in sac_ref.DRAW_SEEDS:
        E = float(np.abs(sac_ref.draw32(seed, n, call) - sac_ref.draw64(seed, n, call)).max())
        print(f"seed {seed:#x} call {call}: E = {E:.3g}")
        # 2 pi u2 rounded to float32 is off by up to 2^-22 (half an ulp at 4..8) and r is below sqrt(-2 log 2^-24) = 5.77: 1.4e-6, plus
        # the roundings of r, cos and the product
        assert 0.0 < E <= 4e-6


def test_log_prob_is_torch_distributions_normal():
    rng = np.random.default_rng(3)
    n, A, mx = 500, 4, 1.0
    head = np.concatenate([rng.normal(0, 0.5, (n, A)), rng.uniform(-0.5, 1.5, (n, A))], 1)
    z = rng.normal(0, 1, (n, A))
    a, lp, sigma = sac_ref.squash64(head, z, mx)
    mu = torch.as_tensor(head[:, :A])
    dist = torch.distributions.Normal(mu, torch.as_tensor(sigma))
    x = mu + torch.as_tensor(sigma) * torch.as_tensor(z)
    action = torch.tanh(x) * mx
    ref = (dist.log_prob(x) - torch.log(1 - action.pow(2) + 1e-6)).sum(1)
    assert np.allclose(a, action.numpy(), rtol=0, atol=1e-15)
    assert np.abs(lp - ref.numpy()).max() <= 1e-9 * np.abs(ref.numpy()).max()  # (x - mu)^2 / (2 sigma^2) against z^2 / 2 at sigma = 1e-6
    assert (sigma == 1e-6).any() and (sigma == 1.0).any()


def test_float32_squash_is_close_on_well_conditioned_rows():
    for A in (2, 4):
        head = sac_ref.case_head64(A)[:4096]
        z = sac_ref.draw64(2, 4096, 7)[:, :A]
        E_a, E_lp = sac_ref.squash_E(head.astype(np.float32), z.astype(np.float32))
        print(f"A = {A}: E(actions) = {E_a:.3g}, E(log_prob) = {E_lp:.3g}")
        assert 0.0 < E_a <= 4 * 2.0 ** -23   # x = mu + sigma z rounded twice, tanh's slope <= 1, tanhf itself
        assert 0.0 < E_lp <= 1e-3            # 1 - a^2 >= 2^-10 amplifies a^2's 2^-24 by at most 2^10 per component, a few times over


@pytest.mark.parametrize("A", [2, 4])
def test_gpu_case_inputs_meet_their_conditions(A):
    """>= 80 % of the rows keep every |a| <= 0.97 max_action under the float64 reference, and either arm of sigma's clamp is taken on
    >= 5 % of the components: the GPU tests compare mostly off tanh's flat ends and see both arms"""
    params, obs = sac_ref.case(A)
    assert [p.shape for p in params] == [(256, 11), (256,), (256, 256), (256,), (A, 256), (A,), (A, 256), (A,)]
    assert all(p.dtype == np.float32 for p in params) and obs.dtype == np.float32 and obs.shape == (sac_ref.CASE_ROWS, 11)
    head = sac_ref.case_head64(A)
    raw = head[:, A:]
    low, high = float((raw < 1e-6).mean()), float((raw > 1.0).mean())
    for seed, call in ((2, 7), (0x1234ABCD00000002, 0xFFFFFFFF)):
        z = sac_ref.draw64(seed, sac_ref.CASE_ROWS, call)[:, :A]
        a, lp, _ = sac_ref.squash64(head, z)
        inside = float(np.all(np.abs(a) <= 0.97, axis=1).mean())
        print(f"A = {A}: {inside:.1%} rows inside, sigma raw < 1e-6 on {low:.1%}, > 1 on {high:.1%} of the components")
        assert inside >= 0.80 and np.all(np.isfinite(lp))
        assert float(sac_ref.well_conditioned_rows(a).mean()) >= 0.80
    assert low >= 0.05 and high >= 0.05
    err32, scale = sac_ref.case_head_err32(A)
    assert 0.0 < err32 <= 1e-4 * scale


def test_losses64_terminal_rows_and_value_target():
    """the float64 losses on a tiny hand-made case: zero networks leave value = q = 0, so the losses are closed forms"""
    A, n = 2, 6
    def zeros(n_in, out):
        return {"fc1.weight": torch.zeros(256, n_in), "fc1.bias": torch.zeros(256), "fc2.weight": torch.zeros(256, 256), "fc2.bias": torch.zeros(256),
                **{f"{k}.weight": torch.zeros(o, 256) for k, o in out.items()}, **{f"{k}.bias": torch.zeros(o) for k, o in out.items()}}
    nets = dict(actor=zeros(11, {"mu": A, "sigma": A}), critic_1=zeros(11 + A, {"q": 1}), critic_2=zeros(11 + A, {"q": 1}),
                value=zeros(11, {"v": 1}), target_value=zeros(11, {"v": 1}))
    nets["actor"]["sigma.bias"] += 1.0
    nets["target_value"]["v.bias"] += 3.0
    rng = np.random.default_rng(0)
    batch = (rng.normal(size=(n, 11)), rng.uniform(-1, 1, (n, A)), np.arange(n, dtype=np.float64), rng.normal(size=(n, 11)),
             np.array([0, 1, 0, 0, 1, 0], bool))
    zero = np.zeros((n, A))
    v, a, c = sac_ref.losses64(nets, batch, zero, zero, gamma=0.5, scale=2.0)
    lp0 = A * (-0.5 * math.log(2 * math.pi) - math.log(1 + 1e-6))  # mu = 0, sigma = 1, z = 0, a = 0
    assert abs(v - 0.5 * lp0 ** 2) < 1e-12 and abs(a - lp0) < 1e-12
    q_hat = 2.0 * np.arange(n) + 0.5 * 3.0 * ~batch[4]  # terminal rows: scale * r only
    assert abs(c - np.mean(q_hat ** 2)) < 1e-9
