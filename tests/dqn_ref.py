"""Host-only references for the fused DQN kernels (roborugby_amd/csrc/rr_dqn.hip): numpy / torch-CPU, none of the project's kernel
code.  tests/test_dqn_ref.py checks these yardsticks themselves (no GPU); tests/test_gpu_dqn_kernels.py holds the kernels to them.

  philox4x32_10 / act_draw   the epsilon draw of rr_dqn_act as the kernel lays it out today (checkpoints carry `act_calls`, so the
                             layout is part of what a resumed run depends on)
  ring_store                 DQNAgent.store_transition (Training_DQN_pytorch.py:126-136) row by row
  forward64 / adam64         the network's forward and torch.optim.Adam's step (no weight decay, no amsgrad) in float64
  learn_grads64              the loss of DQNAgent.learn (Training_DQN_pytorch.py:166-184) and its gradient in float64
                             (tests/test_agent_reference.py holds it to the reference trainer's own float64 run)"""
import numpy as np
import torch

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57   # Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC'11): philox4x32
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85   # key schedule: golden ratio, sqrt(3) - 1
ACT_STREAM = 0x0AC7                             # counter word 2 of the act kernel's draws
MASK32 = 0xFFFFFFFF

MEMORIES = ("state_memory", "new_state_memory", "action_memory", "reward_memory", "terminal_memory")


def philox4x32_10(counter, key):
    """philox4x32 with ten rounds on plain Python integers: counter = 4 words, key = 2 words -> 4 words"""
    c0, c1, c2, c3 = (int(x) & MASK32 for x in counter)
    k0, k1 = (int(x) & MASK32 for x in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c0, c1, c2, c3


def philox4x32_10_rows(c0, c1, c2, c3, k0, k1):
    """the same over numpy arrays of counters (uint64 arithmetic: a 32 x 32-bit product fits); returns four uint64 arrays of 32-bit words"""
    m, s = np.uint64(MASK32), np.uint64(32)
    c0, c1, c2, c3 = (x.copy() & m for x in np.broadcast_arrays(*(np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3))))
    k0, k1 = np.uint64(int(k0) & MASK32), np.uint64(int(k1) & MASK32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ k0, p1 & m, (p0 >> s) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & m, (k1 + np.uint64(PHILOX_W1)) & m
    return c0, c1, c2, c3


def _u_from_word(w):
    # float32(word) rounds to nearest even (as the kernel's conversion does); the product with 2^-32 is exact
    return np.asarray(w).astype(np.uint32).astype(np.float32) * np.float32(2.0 ** -32)


def act_draw(seed, row, call):
    """(u, action) of row `row` in call `call` under `seed` (64 bits): explore iff u <= epsilon (compared in fp32), then take `action`"""
    w = philox4x32_10((row, call, ACT_STREAM, 0), (seed & MASK32, (seed >> 32) & MASK32))
    return np.float32(_u_from_word(w[0])), int(w[1] & 7)


def act_draw_rows(seed, n, call):
    """act_draw for rows 0..n-1: (u float32 [n], action int32 [n])"""
    rows = np.arange(n, dtype=np.uint64)
    w = philox4x32_10_rows(rows, int(call) & MASK32, ACT_STREAM, 0, int(seed) & MASK32, (int(seed) >> 32) & MASK32)
    return _u_from_word(w[0]), (w[1] & np.uint64(7)).astype(np.int32)


def first_argmax(q):
    """index of the first maximum of each row (torch.argmax's promise), written out rather than borrowed"""
    q = np.asarray(q)
    best, mx = np.zeros(q.shape[0], dtype=np.int32), q[:, 0].copy()
    for a in range(1, q.shape[1]):
        better = q[:, a] > mx
        best[better], mx[better] = a, q[better, a]
    return best


def ring_store(mem, mem_cntr, mem_size, rows, valid=None):
    """The reference's store_transition applied row by row, in row order, to copies of the five memories.
    mem = dict of numpy arrays keyed by MEMORIES; rows = (state, action, reward, new_state, done).  Returns (new mem, new mem_cntr)."""
    out = {k: np.array(mem[k], copy=True) for k in MEMORIES}
    state, action, reward, new_state, done = rows
    cntr = int(mem_cntr)
    for i in range(len(action)):
        if valid is not None and not valid[i]:
            continue
        q = cntr % int(mem_size)
        out["state_memory"][q] = state[i]
        out["new_state_memory"][q] = new_state[i]
        out["action_memory"][q] = action[i]
        out["reward_memory"][q] = reward[i]
        out["terminal_memory"][q] = bool(done[i])
        cntr += 1
    return out, cntr


def forward64(params, x):
    """Q values [n, 8] in float64: params = (fc1.weight, fc1.bias, fc2.weight, fc2.bias, fc3.weight, fc3.bias), torch.nn.Linear layout"""
    w1, b1, w2, b2, w3, b3 = (torch.as_tensor(p).detach().cpu().double() for p in params)
    x = torch.as_tensor(x).detach().cpu().double()
    h1 = torch.clamp(x @ w1.t() + b1, min=0.0)
    h2 = torch.clamp(h1 @ w2.t() + b2, min=0.0)
    return h2 @ w3.t() + b3


def learn_grads64(eval_params, target_params, batch, gamma):
    """(loss, [gradient per eval parameter, in their order]) of DQNAgent.learn's loss in float64.  batch = (state, action, reward,
    new_state, done): q_eval = Q_eval(state)[row, action]; q_next = Q_target(new_state) with the whole ROW of a terminal sample set to
    0 before the max; q_target = reward + gamma * max_a q_next, a constant; loss = the mean over the batch of (q_target - q_eval)^2"""
    state, action, reward, new_state, done = (torch.as_tensor(np.asarray(t)) for t in batch)
    leaves = [torch.as_tensor(np.asarray(p)).double().clone().requires_grad_(True) for p in eval_params]
    w1, b1, w2, b2, w3, b3 = leaves
    h = torch.clamp(torch.clamp(state.double() @ w1.t() + b1, min=0.0) @ w2.t() + b2, min=0.0)
    q_eval = (h @ w3.t() + b3)[torch.arange(state.shape[0]), action.long()]
    q_next = forward64(target_params, new_state)
    q_next[done.bool()] = 0.0
    q_target = reward.double() + gamma * q_next.max(dim=1)[0]
    loss = ((q_target - q_eval) ** 2).mean()
    return float(loss.detach()), [g.numpy() for g in torch.autograd.grad(loss, leaves)]


def adam64(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's step number `step` (1-based) in float64: returns (p, m, v) after it"""
    p, g, m, v = (torch.as_tensor(t).detach().cpu().double() for t in (p, g, m, v))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = v.sqrt() / (bc2 ** 0.5) + eps
    return p - (lr / bc1) * (m / denom), m, v
