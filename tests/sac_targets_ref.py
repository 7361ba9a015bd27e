"""Host-only reference for rr_sac_targets (roborugby_amd/csrc/rr_sac.hip k_sac_targets, rr_sac.hpp; include/roborugby_amd.h is the
specification): numpy / torch-CPU float64, none of the project's kernel code.  tests/test_sac_targets_ref.py checks this yardstick itself
(against the reference trainer's own float64 run, tests/golden/sac_learn.npz) and the GPU tests' inputs without a GPU;
tests/test_sac_targets_emulated.py holds the g++ build of csrc/rr_sac.hpp's per-row functions to it, tests/test_gpu_sac_targets.py the kernel.

  mlp64 / critic64                 a two-hidden-layer MLP with one output in float64 (any width), the critic on [s, a]
  targets64                        value_target, q_hat and every window of the kernel in float64
  value_target32 / q_hat32         the two closing formulas restated in float32 numpy, operation by operation
  ring_row_ok                      the gather's bounds rule
  words / row_uniforms / draw64 / draw32   the draw with stream word 0x5A7A
  case(A)                          the GPU tests' networks, rings and index vector"""
import functools
import math

import numpy as np
import torch

import dqn_ref
import sac_ref

TARGETS_STREAM = 0x5A7A  # counter word 2 of rr_sac_targets' draws (rr_sac_act: 0x5AC7)
MASK32 = dqn_ref.MASK32
M = 300                  # ring rows of case(A): not a multiple of 64
# (seed, call, B) of the GPU tests; B = 64 * (CUs + 1) is 16,448 on the MI355X's 256 CUs
GPU_DRAWS = ((2, 7, 64), (0x1234ABCD00000002, 0xFFFFFFFF, 16448), (0x1234ABCD00000002, 1, 576))


# ---- the draw
def words(seed, n, call):
    rows = np.arange(n, dtype=np.uint64)
    return dqn_ref.philox4x32_10_rows(rows, int(call) & MASK32, TARGETS_STREAM, 0, int(seed) & MASK32, (int(seed) >> 32) & MASK32)


def row_uniforms(seed, n, call):
    """[n, 2, 2] float64: (pair, (u1, u2)) of every batch row"""
    w = words(seed, n, call)
    return np.stack([np.stack(sac_ref.uniforms(w[0], w[1]), 1), np.stack(sac_ref.uniforms(w[2], w[3]), 1)], 1)


def draw64(seed, n, call):
    u = row_uniforms(seed, n, call)
    r, a = np.sqrt(-2.0 * np.log(u[:, :, 0])), 2.0 * math.pi * u[:, :, 1]
    return np.stack([r * np.cos(a), r * np.sin(a)], 2).reshape(n, 4)


def draw32(seed, n, call):
    u = row_uniforms(seed, n, call).astype(np.float32)  # exact
    f = np.float32
    r, a = np.sqrt(f(-2.0) * np.log(u[:, :, 0])), f(2.0 * math.pi) * u[:, :, 1]
    z = np.stack([r * np.cos(a), r * np.sin(a)], 2).reshape(n, 4)
    assert z.dtype == np.float32
    return z


# ---- the networks
def mlp64(params, x):
    """[n] float64: Linear -> ReLU -> Linear -> ReLU -> Linear(1) with params = (fc1.weight, fc1.bias, fc2.weight, fc2.bias, out.weight
    [1, W], out.bias [1]), torch.nn.Linear layouts, any width"""
    w1, b1, w2, b2, wo, bo = (torch.as_tensor(np.array(p)).double() for p in params)
    x = torch.as_tensor(np.array(x)).double()
    h = torch.clamp(torch.clamp(x @ w1.t() + b1, min=0.0) @ w2.t() + b2, min=0.0)
    return (h @ wo.t() + bo).view(-1).numpy()


def mlp32(params, x):
    """the torch float32 forward on the CPU"""
    w1, b1, w2, b2, wo, bo = (torch.as_tensor(np.array(p)).float() for p in params)
    x = torch.as_tensor(np.array(x)).float()
    return (torch.relu(torch.relu(x @ w1.t() + b1) @ w2.t() + b2) @ wo.t() + bo).view(-1).numpy()


def critic64(params, state, action):
    return mlp64(params, np.concatenate([np.asarray(state, np.float64), np.asarray(action, np.float64)], 1))


def ring_row_ok(i, mem_rows):
    i = np.asarray(i, np.int64)
    return (i >= 0) & (i < mem_rows)


# ---- the closing formulas
def value_target32(q1, q2, log_prob):
    f = np.float32
    q1, q2, log_prob = np.asarray(q1, f), np.asarray(q2, f), np.asarray(log_prob, f)
    out = np.minimum(q1, q2) - log_prob
    assert out.dtype == f
    return out


def q_hat32(reward_scale, reward, gamma, done, v_next):
    """fl(fl(reward_scale * r) + fl(gamma * (done ? 0 : v)))"""
    f = np.float32
    reward, v_next = np.asarray(reward, f), np.asarray(v_next, f)
    out = f(reward_scale) * reward + f(gamma) * np.where(np.asarray(done, bool), f(0.0), v_next)
    assert out.dtype == f
    return out


def targets64(nets, rings, index, noise, gamma, scale, max_action=1.0):
    """Everything rr_sac_targets writes, in float64, as a dict: value_target, q_hat, state, action, policy_action, log_prob, head,
    noise_out, q1, q2, v_next.  nets: dict actor (eight arrays, rr_sac_act's order), critic_1, critic_2, target_value (six each);
    rings = (state_memory, new_state_memory, action_memory, reward_memory, terminal_memory); index: ring rows [B], every one inside the
    rings; noise [B, A]."""
    state_m, new_state_m, action_m, reward_m, terminal_m = (np.asarray(r) for r in rings)
    index = np.asarray(index, np.int64)
    assert np.all(ring_row_ok(index, state_m.shape[0]))
    s, s_, a, r, done = state_m[index], new_state_m[index], action_m[index], reward_m[index].astype(np.float64), terminal_m[index].astype(bool)
    head = sac_ref.actor_head64(nets["actor"], s)
    z = np.asarray(noise, np.float64)
    pa, lp, _ = sac_ref.squash64(head, z, max_action)
    q1, q2 = critic64(nets["critic_1"], s, pa), critic64(nets["critic_2"], s, pa)
    v = mlp64(nets["target_value"], s_)
    return dict(value_target=np.minimum(q1, q2) - lp, q_hat=scale * r + gamma * np.where(done, 0.0, v), state=s, action=a, policy_action=pa,
                log_prob=lp, head=head, noise_out=z, q1=q1, q2=q2, v_next=v)


# ---- the GPU tests' inputs
@functools.lru_cache(maxsize=None)
def case(A):
    """(nets, rings, index): sac_ref.case(A)'s actor; critics and the target value net at width 256 from a seeded generator in
    torch.nn.Linear's ranges; rings of M = 300 rows whose state_memory is the first 300 of sac_ref.case(A)'s observations, every fifth row
    terminal; index: 19,200 ring rows that begin 0, M - 1, 0, M - 1 (repeats) and go on drawn with replacement, so that any prefix the
    GPU tests take holds both ends of the ring and repeats."""
    actor, obs = sac_ref.case(A)
    rng = np.random.default_rng(7300 + A)
    f = np.float32

    def linear(n_out, n_in):
        b = 1.0 / math.sqrt(n_in)
        return rng.uniform(-b, b, (n_out, n_in)).astype(f), rng.uniform(-b, b, n_out).astype(f)

    def mlp(n_in):
        return (*linear(256, n_in), *linear(256, 256), *linear(1, 256))

    nets = dict(actor=tuple(actor), critic_1=mlp(11 + A), critic_2=mlp(11 + A), target_value=mlp(11))
    state_m = np.ascontiguousarray(obs[:M])
    new_state_m = rng.uniform(-1.0, 1.0, (M, 11)).astype(f)
    action_m = rng.uniform(-1.0, 1.0, (M, A)).astype(f)
    reward_m = rng.normal(0.0, 2.0, M).astype(f)
    terminal_m = (np.arange(M) % 5 == 0)
    index = rng.integers(0, M, sac_ref.CASE_ROWS).astype(np.int64)
    index[:4] = (0, M - 1, 0, M - 1)
    for arr in (*nets["critic_1"], *nets["critic_2"], *nets["target_value"], state_m, new_state_m, action_m, reward_m, terminal_m, index):
        arr.setflags(write=False)
    return nets, (state_m, new_state_m, action_m, reward_m, terminal_m), index
