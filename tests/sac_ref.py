"""Host-only references for the SAC actor kernel (roborugby_amd/csrc/rr_sac.hip, rr_sac.hpp) and the SAC agent (roborugby_amd/sac.py):
numpy / torch-CPU, none of the project's kernel code.  tests/test_sac_ref.py checks these yardsticks themselves (no GPU);
tests/test_sac_emulated.py holds the g++ build of csrc/rr_sac.hpp to them and tests/test_gpu_sac_act.py the kernel;
tests/test_agent_reference.py holds actor_head64, squash64 and losses64 to the reference trainer's own float64 run (tests/golden/sac_*.npz).

  words / uniforms / draw64      rr_sac_act's draw as include/roborugby_amd.h specifies it, in float64
  actor_head64                   ActorNetwork.forward up to (mu, raw sigma) in float64
  squash64                       clamp, x = mu + sigma z, a = max_action tanh(x), the log-probability, in float64
  draw32 / squash32              the same formulas restated in float32 numpy, operation by operation: what float32 arithmetic alone costs.
                                 Their largest distance from the float64 versions is the "E" of the GPU tests' bars.
  losses64                       the three losses of Agent.learn (Training_SAC_pytorch.py:344-383) in float64
  case(A)                        the GPU tests' parameters and observations (test_sac_ref.py holds them to their conditions)"""
import functools
import math

import numpy as np
import torch

import dqn_ref

SAC_STREAM = 0x5AC7          # counter word 2 of the draws
SIGMA_MIN, SIGMA_MAX, LOG_EPS = 1e-6, 1.0, 1e-6
MASK32 = dqn_ref.MASK32
DRAW_SEEDS = ((0, 1, 65536), (2, 7, 65536), (0x1234ABCD00000002, 1, 4096))  # (seed, call, n) the draw is held to


def words(seed, n, call):
    """Philox4x32-10 of counter (row, call, SAC_STREAM, 0) under key (seed low, seed high) for rows 0..n-1: four uint64 arrays of words"""
    rows = np.arange(n, dtype=np.uint64)
    return dqn_ref.philox4x32_10_rows(rows, int(call) & MASK32, SAC_STREAM, 0, int(seed) & MASK32, (int(seed) >> 32) & MASK32)


def uniforms(wa, wb):
    """(u1 in (0, 1], u2 in [0, 1)) as float64; both are multiples of 2^-24 and exact in float32"""
    u1 = ((np.asarray(wa, np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (np.asarray(wb, np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def row_uniforms(seed, n, call):
    """[n, 2, 2] float64: (pair, (u1, u2)) of every row"""
    w = words(seed, n, call)
    return np.stack([np.stack(uniforms(w[0], w[1]), 1), np.stack(uniforms(w[2], w[3]), 1)], 1)


def draw64(seed, n, call):
    """z [n, 4] float64: Box-Muller of the pairs (w0, w1) -> z0, z1 and (w2, w3) -> z2, z3"""
    u = row_uniforms(seed, n, call)
    r, a = np.sqrt(-2.0 * np.log(u[:, :, 0])), 2.0 * math.pi * u[:, :, 1]
    return np.stack([r * np.cos(a), r * np.sin(a)], 2).reshape(n, 4)


def draw32(seed, n, call):
    """the same in float32, operation by operation as the specification writes it"""
    u = row_uniforms(seed, n, call).astype(np.float32)  # exact
    f = np.float32
    r, a = np.sqrt(f(-2.0) * np.log(u[:, :, 0])), f(2.0 * math.pi) * u[:, :, 1]
    z = np.stack([r * np.cos(a), r * np.sin(a)], 2).reshape(n, 4)
    assert z.dtype == np.float32
    return z


def actor_head64(params, x):
    """[n, 2A] float64: mu [0..A), then the raw sigma outputs; params = (fc1.weight, fc1.bias, fc2.weight, fc2.bias, mu.weight, mu.bias,
    sigma.weight, sigma.bias), torch.nn.Linear layouts"""
    w1, b1, w2, b2, wm, bm, ws, bs = (torch.as_tensor(np.asarray(p)).double() for p in params)
    x = torch.as_tensor(np.asarray(x)).double()
    h = torch.clamp(torch.clamp(x @ w1.t() + b1, min=0.0) @ w2.t() + b2, min=0.0)
    return torch.cat([h @ wm.t() + bm, h @ ws.t() + bs], 1).numpy()


def actor_head32(params, x):
    """the torch float32 forward on the CPU: what one float32 summation order differs from actor_head64"""
    w1, b1, w2, b2, wm, bm, ws, bs = (torch.as_tensor(np.asarray(p)).float() for p in params)
    x = torch.as_tensor(np.asarray(x)).float()
    h = torch.relu(torch.relu(x @ w1.t() + b1) @ w2.t() + b2)
    return torch.cat([h @ wm.t() + bm, h @ ws.t() + bs], 1).numpy()


def squash64(head, z, max_action=1.0):
    """(actions [n, A], log_prob [n], sigma [n, A]) in float64 from head [n, 2A] and the draws z [n, A]"""
    head, z = np.asarray(head, np.float64), np.asarray(z, np.float64)
    A = head.shape[1] // 2
    mu, sigma = head[:, :A], np.clip(head[:, A:], SIGMA_MIN, SIGMA_MAX)
    a = max_action * np.tanh(mu + sigma * z)
    lp = -0.5 * z * z - np.log(sigma) - 0.5 * math.log(2.0 * math.pi) - np.log(1.0 - a * a + LOG_EPS)
    return a, lp.sum(1), sigma


def squash32(head, z, max_action=1.0):
    """(actions, log_prob) in float32, operation by operation as the specification writes them (the sum over k in order, from 0)"""
    f = np.float32
    head, z = np.asarray(head, f), np.asarray(z, f)
    A = head.shape[1] // 2
    mu, raw = head[:, :A], head[:, A:]
    sigma = np.where(raw < f(SIGMA_MIN), f(SIGMA_MIN), np.where(raw > f(SIGMA_MAX), f(SIGMA_MAX), raw))
    a = f(max_action) * np.tanh(mu + sigma * z)
    term = f(-0.5) * z * z - np.log(sigma) - f(0.5 * math.log(2.0 * math.pi)) - np.log(f(1.0) - a * a + f(LOG_EPS))
    lp = np.zeros(head.shape[0], f)
    for k in range(A):
        lp = lp + term[:, k]
    assert a.dtype == f and lp.dtype == f
    return a, lp


def well_conditioned_rows(actions, max_action=1.0):
    """rows where every component has 1 - (a / max_action)^2 >= 2^-10: beyond, log(1 - a^2 + 1e-6) cancels catastrophically"""
    a = np.asarray(actions, np.float64) / max_action
    return np.all(1.0 - a * a >= 2.0 ** -10, axis=1)


def squash_E(head, z, max_action=1.0):
    """(E of the actions, E of log_prob over the well-conditioned rows): the float32 restatement's largest distance from squash64 on
    these very inputs"""
    a64, lp64, _ = squash64(head, z, max_action)
    a32, lp32 = squash32(head, z, max_action)
    rows = well_conditioned_rows(a64, max_action)
    return float(np.abs(a32 - a64).max()), float(np.abs(lp32 - lp64)[rows].max()) if rows.any() else 0.0


# ---- the agent's losses
def _mlp64(sd, prefix_out, x):
    h = torch.clamp(x @ sd["fc1.weight"].double().t() + sd["fc1.bias"].double(), min=0.0)
    h = torch.clamp(h @ sd["fc2.weight"].double().t() + sd["fc2.bias"].double(), min=0.0)
    return h @ sd[prefix_out + ".weight"].double().t() + sd[prefix_out + ".bias"].double()


def losses64(nets, batch, noise_value, noise_actor, gamma, scale, max_action=1.0):
    """(value_loss, actor_loss, critic_loss) of Agent.learn in float64.  nets: state_dicts keyed actor, critic_1, critic_2, value,
    target_value; batch = (state, action, reward, new_state, done)"""
    state, action, reward, state_, done = (torch.as_tensor(np.asarray(t)) for t in batch)
    state, action, reward, state_ = state.double(), action.double(), reward.double(), state_.double()
    A = action.shape[1]
    head = torch.cat([_mlp64(nets["actor"], "mu", state), _mlp64(nets["actor"], "sigma", state)], 1).numpy()

    def sample(noise):
        a, lp, _ = squash64(head, np.asarray(noise, np.float64), max_action)
        return torch.as_tensor(a), torch.as_tensor(lp)

    def q_min(a):
        sa = torch.cat([state, a], 1)
        return torch.minimum(_mlp64(nets["critic_1"], "q", sa), _mlp64(nets["critic_2"], "q", sa)).view(-1)

    value = _mlp64(nets["value"], "v", state).view(-1)
    value_ = _mlp64(nets["target_value"], "v", state_).view(-1)
    value_[done.bool()] = 0.0
    a_v, lp_v = sample(noise_value)
    value_loss = 0.5 * torch.mean((value - (q_min(a_v) - lp_v)) ** 2)
    a_p, lp_p = sample(noise_actor)
    actor_loss = torch.mean(lp_p - q_min(a_p))
    q_hat = scale * reward + gamma * value_
    sa = torch.cat([state, action], 1)
    critic_loss = 0.5 * torch.mean((_mlp64(nets["critic_1"], "q", sa).view(-1) - q_hat) ** 2) \
        + 0.5 * torch.mean((_mlp64(nets["critic_2"], "q", sa).view(-1) - q_hat) ** 2)
    assert A == head.shape[1] // 2
    return float(value_loss), float(actor_loss), float(critic_loss)


# ---- the GPU tests' inputs
CASE_ROWS = 64 * 300  # more rows than any GPU test shape takes (64 * (CUs + 1) at 256 CUs is 16,448)


@functools.lru_cache(maxsize=None)
def case(A):
    """(params: eight float32 arrays in rr_sac_act's order, obs float32 [CASE_ROWS, 11]) for n_actions = A.  torch.nn.Linear's initial
    ranges for the hidden layers; the mu head scaled so that most samples stay off tanh's flat ends, the sigma head scaled and shifted
    so that both arms of the clamp are taken often."""
    rng = np.random.default_rng(20260 + A)
    f = np.float32

    def linear(n_out, n_in, scale=1.0, shift=0.0):
        b = 1.0 / math.sqrt(n_in)
        return (rng.uniform(-b, b, (n_out, n_in)) * scale).astype(f), (rng.uniform(-b, b, n_out) * scale + shift).astype(f)

    w1, b1 = linear(256, 11)
    w2, b2 = linear(256, 256)
    wm, bm = linear(A, 256, scale=2.0)
    ws, bs = linear(A, 256)
    obs = rng.uniform(-1.0, 1.0, (CASE_ROWS, 11)).astype(f)
    # every raw sigma output gets mean 0.5 and standard deviation 1 over the rows: about 30 % of them below 1e-6, 30 % above 1
    raw = actor_head64((w1, b1, w2, b2, wm, bm, ws, np.zeros(A, f)), obs)[:, A:]
    gain = 1.0 / raw.std(0)
    ws, bs = (ws * gain[:, None]).astype(f), (0.5 - raw.mean(0) * gain).astype(f)
    return (w1, b1, w2, b2, wm, bm, ws, bs), obs


@functools.lru_cache(maxsize=None)
def case_head64(A):
    params, obs = case(A)
    return actor_head64(params, obs)


@functools.lru_cache(maxsize=None)
def case_head_err32(A):
    """largest distance of the torch float32 forward from the float64 one on the case's rows, and the head's scale"""
    params, obs = case(A)
    h64 = case_head64(A)
    return float(np.abs(actor_head32(params, obs).astype(np.float64) - h64).max()), float(np.abs(h64).max())
