"""Host-only reference for rr_sac_grads (roborugby_amd/csrc/rr_sac.hip k_sac_grads; include/roborugby_amd.h is the specification): numpy
float64, none of the project's kernel code.  tests/test_sac_grads_ref.py checks this yardstick itself (against the reference trainer's own
float64 run, tests/golden/sac_learn.npz, and against torch float64 autograd of the agent's losses) and the GPU tests' inputs without a GPU;
tests/test_gpu_sac_grads.py holds the kernel to it.

  net_grads64(params, x, y)        forward, 0.5 * mse loss and the six gradients of one Linear K -> W -> W -> 1 ReLU MLP regressed onto the
                                   constant vector y, any width W
  grads64(nets, state, action, value_target, q_hat)   the three nets of rr_sac_grads: value on s / value_target, the critics on [s, a] / q_hat
  case(A)                          the GPU tests' networks, rows and targets (width 256)"""
import functools
import math

import numpy as np

import sac_ref

NETS = ("value", "critic_1", "critic_2")  # rr_sac_grads' order: loss[0], loss[1], loss[2]
KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "out.weight", "out.bias")  # a net's six tensors, torch.nn.Linear layouts


def net_grads64(params, x, y):
    """-> dict(grads: six float64 arrays in params' shapes, loss, f [B], h1, h2 [B, W]).  params = (fc1.weight [W, K], fc1.bias, fc2.weight
    [W, W], fc2.bias, out.weight [1, W], out.bias [1]); x [B, K]; y [B].  loss = 0.5 * mean((f - y)^2); the output gradient of a row is
    (f - y) / B; relu' = h > 0 (0 at h == 0, as torch has it)."""
    w1, b1, w2, b2, wo, bo = (np.asarray(p, np.float64) for p in params)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    B = x.shape[0]
    h1 = np.maximum(x @ w1.T + b1, 0.0)
    h2 = np.maximum(h1 @ w2.T + b2, 0.0)
    f = h2 @ wo[0] + bo[0]
    d = (f - y) / B
    dh2 = d[:, None] * wo[0][None, :] * (h2 > 0.0)
    dh1 = (dh2 @ w2) * (h1 > 0.0)
    grads = (dh1.T @ x, dh1.sum(0), dh2.T @ h1, dh2.sum(0), (d @ h2)[None, :], np.array([d.sum()]))
    assert all(g.shape == np.shape(p) for g, p in zip(grads, params))
    return dict(grads=grads, loss=0.5 * float(np.mean((f - y) ** 2)), f=f, h1=h1, h2=h2)


def grads64(nets, state, action, value_target, q_hat):
    """{net: net_grads64(...)} for value (on state, onto value_target) and critic_1, critic_2 (on [state, action], onto q_hat):
    value_loss = ["value"]["loss"], critic_loss = ["critic_1"]["loss"] + ["critic_2"]["loss"]"""
    sa = np.concatenate([np.asarray(state, np.float64), np.asarray(action, np.float64)], 1)
    return dict(value=net_grads64(nets["value"], state, value_target), critic_1=net_grads64(nets["critic_1"], sa, q_hat),
                critic_2=net_grads64(nets["critic_2"], sa, q_hat))


# ---- the GPU tests' inputs
@functools.lru_cache(maxsize=None)
def case(A):
    """(nets, state, action, value_target, q_hat): the value net and the two critics at width 256 from a seeded generator in
    torch.nn.Linear's ranges (as sac_targets_ref.case draws its nets); state = sac_ref.case(A)'s observations [CASE_ROWS, 11], action
    uniform in [-1, 1], the two target vectors standard normal (the nets' outputs are a few tenths: no row's target is its output)."""
    _, obs = sac_ref.case(A)
    rng = np.random.default_rng(7400 + A)
    f = np.float32

    def linear(n_out, n_in):
        b = 1.0 / math.sqrt(n_in)
        return rng.uniform(-b, b, (n_out, n_in)).astype(f), rng.uniform(-b, b, n_out).astype(f)

    def mlp(n_in):
        return (*linear(256, n_in), *linear(256, 256), *linear(1, 256))

    nets = dict(value=mlp(11), critic_1=mlp(11 + A), critic_2=mlp(11 + A))
    n = sac_ref.CASE_ROWS
    action = rng.uniform(-1.0, 1.0, (n, A)).astype(f)
    value_target, q_hat = rng.normal(0.0, 1.0, n).astype(f), rng.normal(0.0, 1.0, n).astype(f)
    for arr in (*nets["value"], *nets["critic_1"], *nets["critic_2"], action, value_target, q_hat):
        arr.setflags(write=False)
    return nets, obs, action, value_target, q_hat


@functools.lru_cache(maxsize=None)
def case_grads64(A, B):
    """grads64 of the first B rows of case(A), computed once per (A, B) and left unchanged"""
    nets, state, action, value_target, q_hat = case(A)
    return grads64(nets, state[:B], action[:B], value_target[:B], q_hat[:B])
