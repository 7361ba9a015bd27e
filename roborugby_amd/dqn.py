"""Batched DQN trainer: the vectorised counterpart of the reference's Training_DQN_pytorch.py (BASELINE.json config 5).

Same agent as the reference (`DeepQNetwork` Training_DQN_pytorch.py:25-67: Linear 11->256->256->8 with ReLU, Adam
lr 5e-4, MSE; `DQNAgent` :70-197: gamma .99, epsilon-greedy, target network, uniform replay) and the same call pattern as
its main loop (:317-377: choose_action -> env.step -> store_transition (+ the grumpy team's transition when it has robots)
-> learn()), but every tensor -- observations, replay memory, networks -- stays on the MI355X and one call handles all N
arenas.

What "one learn() per env.step" becomes when a step delivers N transitions (the reference: N = 1).  Every schedule the
reference ties to its step counter is kept PER TRANSITION, so it means the same at any N:
  * epsilon:  eps <- max(eps * eps_dec ** n_new, eps_end) for the n_new transitions stored since the last update
              (reference: one factor eps_dec per learn() = per transition, :186-191; 1.0 -> 0.2 after 5.4e5 transitions);
  * target:   Q_target <- Q_eval whenever `target_update_freq` more transitions have been stored (reference :187; in the
              reference that is also 100,000 gradient updates -- its target network is nearly frozen -- so train() scales
              it with the batch: max(100,000, target_sync_vector_steps * N) transitions);
  * replay:   `replay_vector_steps` vector steps deep (at least the reference's 500,000 transitions);
  * update-to-data: the reference draws 2,500 samples per transition, which at 65,536 transitions per step would be
              1.6e8 samples per step.  Here `updates_per_step` (k) gradient steps of `batch_size` (B) samples follow every
              vector step: k * B / N samples per transition (defaults k = 4, B = 32,768: 2 per transition at 65,536 arenas).

    python -m roborugby_amd.dqn --num-envs 65536 --steps 3000 --eval-every 300 --out profiles/r02/dqn_T_65536.json
"""
import argparse
import copy
import ctypes as C
import json
import math
import os
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .env import STATUS_NOT_READY, STATUS_WAS_RESET


class _WideBatchLinear(torch.autograd.Function):
    """y = x W^T + b for a batch far wider than the layer (32,768 samples against 8..256 features).  The forward is F.linear.
    In the backward the weight gradient g^T x is a GEMM with a tiny output and a 32,768-long reduction, which the GEMM library
    runs on a handful of workgroups (139 / 65 / 63 us for the three layers on an MI355X -- 40 % of a learn() step): here the
    batch is cut into slices, one batched GEMM forms the partial products on more of the chip and a small reduction adds them
    (config 5: 14.7 -> 20.4 M env-steps/s over 2,000 vector steps)."""
    SLICE = int(os.environ.get("RR_DQN_SLICE", "1024"))  # samples per slice (0: plain layers); 512 / 1024 / 2048 / 4096 measured: 18.0 / 20.4 / 20.3 / 19.5 M env-steps/s

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = g @ w if ctx.needs_input_grad[0] else None
        S = _WideBatchLinear.SLICE
        if S <= 0 or x.shape[0] % S:  # (_linear only routes whole multiples here; anything else takes the plain GEMM)
            return gx, g.t() @ x, g.sum(0)
        n = x.shape[0] // S
        gw = torch.bmm(g.reshape(n, S, -1).transpose(1, 2), x.reshape(n, S, -1)).sum(0)  # reshape: g may arrive non-contiguous
        return gx, gw, g.sum(0)


def _linear(layer, x):
    if _WideBatchLinear.SLICE > 0 and x.dim() == 2 and x.shape[0] >= 8 * _WideBatchLinear.SLICE and x.shape[0] % _WideBatchLinear.SLICE == 0 and torch.is_grad_enabled():
        return _WideBatchLinear.apply(x, layer.weight, layer.bias)
    return layer(x)


class DeepQNetwork(nn.Module):
    def __init__(self, lr, input_dims, fc1_dims, fc2_dims, n_actions):
        super().__init__()
        self.fc1 = nn.Linear(input_dims, fc1_dims)
        self.fc2 = nn.Linear(fc1_dims, fc2_dims)
        self.fc3 = nn.Linear(fc2_dims, n_actions)
        # (the fused single-kernel Adam step where the parameters live on the GPU: the learn() call is launch-bound)
        self.optimizer = torch.optim.Adam(self.parameters(), lr=lr)
        self._lr = lr
        self.loss = nn.MSELoss()

    def forward(self, state):
        x = F.relu(_linear(self.fc1, state.float()))
        x = F.relu(_linear(self.fc2, x))
        return _linear(self.fc3, x)


class _ReplayAgent:
    """What BatchedDQNAgent and PixelDQNAgent share: hyper-parameters, counters, the seeded generator, the replay ring, the rr_dqn handle,
    the torch paths of acting / storing / learning, the per-transition schedules (module docstring) and the checkpoint.  A subclass
    builds its network (`make_net`, called after the seeding), names the shape and dtype of an observation, sets `self.optimizer`
    (attribute or property) and calls _open_handle once it knows whether its kernels apply."""
    PERMUTE_LIMIT = 1 << 20  # sample without replacement (reference: np.random.choice(replace=False)) while a permutation is cheap

    def __init__(self, make_net, obs_shape, obs_dtype, gamma, epsilon, batch_size, n_actions, max_mem_size, eps_end, eps_dec,
                 target_update_freq, device, seed, dense_memory=True):
        self.gamma, self.epsilon, self.eps_end, self.eps_dec = gamma, epsilon, eps_end, eps_dec
        self.n_actions, self.mem_size, self.batch_size = n_actions, int(max_mem_size), int(batch_size)
        self.target_update_freq = int(target_update_freq)
        self.device = torch.device(device)
        self.mem_cntr = 0            # transitions stored so far (the reference's mem_cntr)
        self._eps_cntr = 0           # ... of which the epsilon schedule has already been charged
        self._next_target_sync = self.target_update_freq
        self.target_syncs, self.updates, self.last_loss = 0, 0, None
        self._act_calls = 0  # fused choose_action calls so far: keys the kernel's epsilon draws (checkpointed)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)
        self._seed = int(seed)
        torch.manual_seed(seed)
        self.Q_eval = make_net()
        self.Q_target = copy.deepcopy(self.Q_eval)
        m, d = self.mem_size, self.device
        self.state_memory = self.new_state_memory = self.action_memory = self.reward_memory = self.terminal_memory = None
        if dense_memory:  # (a subclass with a replay of its own asks for none)
            self.state_memory = torch.zeros((m,) + tuple(obs_shape), dtype=obs_dtype, device=d)
            self.new_state_memory = torch.zeros((m,) + tuple(obs_shape), dtype=obs_dtype, device=d)
            self.action_memory = torch.zeros(m, dtype=torch.int64, device=d)
            self.reward_memory = torch.zeros(m, dtype=torch.float32, device=d)
            self.terminal_memory = torch.zeros(m, dtype=torch.bool, device=d)
        self._dqn = None

    def _open_handle(self, fused, can_fuse, needs):
        """self.fused (None: on whenever the kernels apply) and, when it is on, the rr_dqn handle (_lib.DqnHandle)"""
        self.fused = can_fuse if fused is None else bool(fused)
        if self.fused and not can_fuse:
            raise ValueError(f"fused=True needs {needs}")
        if self.fused:
            self._dqn = _lib.DqnHandle(self.device)

    _fused_h = property(lambda self: self._dqn.h if self._dqn else None)  # the C-ABI's handle and library, as tests and tools drive them
    _rrlib = property(lambda self: self._dqn.lib)

    def close(self):
        """rr_dqn_destroy: the handle holds the per-workgroup partial gradients and the Adam moments (~73 MB of device memory)."""
        if getattr(self, "_dqn", None):
            self._dqn.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _epsilon_greedy(self, greedy, eps):
        """the torch path of choose_action (Training_DQN_pytorch.py:138-149): int32 [n] from the greedy actions"""
        if eps <= 0:
            return greedy.to(torch.int32)
        n = greedy.shape[0]
        rand = torch.randint(0, self.n_actions, (n,), generator=self.gen, device=self.device)
        explore = torch.rand(n, generator=self.gen, device=self.device) <= eps
        return torch.where(explore, rand, greedy).to(torch.int32)

    @staticmethod
    def _compact(state, action, reward, state_, done, valid):
        """the rows with valid=True (None: all), in row order"""
        action, reward, done = action.reshape(-1), reward.reshape(-1), done.reshape(-1)
        if valid is not None:
            idx = valid.reshape(-1).nonzero(as_tuple=True)[0]
            state, action, reward, state_, done = state[idx], action[idx], reward[idx], state_[idx], done[idx]
        return state, action, reward, state_, done

    def _ring_write(self, state, action, reward, state_, done):
        """the torch path of store_transition (Training_DQN_pytorch.py:126-136) for n rows at once"""
        n = state.shape[0]
        if n == 0:
            return
        pos = (self.mem_cntr + torch.arange(n, device=self.device)) % self.mem_size
        self.state_memory[pos] = state.to(self.state_memory.dtype)
        self.new_state_memory[pos] = state_.to(self.state_memory.dtype)
        self.action_memory[pos] = action.long()
        self.reward_memory[pos] = reward.float()
        self.terminal_memory[pos] = done.bool()
        self.mem_cntr += n

    def _sample(self, max_mem):
        if max_mem <= self.PERMUTE_LIMIT:
            return torch.randperm(max_mem, generator=self.gen, device=self.device)[:self.batch_size]  # replace=False
        # a multi-million-entry memory: independent draws (two of B draws coincide with probability ~B^2 / 2 max_mem per batch)
        return torch.randint(0, max_mem, (self.batch_size,), generator=self.gen, device=self.device)

    def _learn_core(self, max_mem):
        """sampling + TD target + one Adam step (Training_DQN_pytorch.py:156-186); everything on the device, no host sync"""
        self.optimizer.zero_grad(set_to_none=False)
        batch = self._sample(max_mem)
        q_eval = self.Q_eval(self.state_memory[batch]).gather(1, self.action_memory[batch].view(-1, 1)).squeeze(1)
        with torch.no_grad():
            q_next = self.Q_target(self.new_state_memory[batch]).masked_fill(self.terminal_memory[batch].view(-1, 1), 0.0)
            q_target = self.reward_memory[batch] + self.gamma * q_next.max(dim=1)[0]
        loss = F.mse_loss(q_eval, q_target)
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    _learn_step = _learn_core  # what learn() runs: a subclass with kernels or a captured graph chooses here

    def learn(self):
        """One gradient step (Training_DQN_pytorch.py:151-191) + the per-transition schedules (module docstring)."""
        if self.mem_cntr < self.batch_size:
            return None
        loss = self._learn_step(min(self.mem_size, self.mem_cntr))
        self.updates += 1
        # the reference syncs when mem_cntr hits a multiple of target_update_freq; with N transitions per call the
        # counter jumps, so sync whenever a multiple has been crossed
        if self.mem_cntr >= self._next_target_sync:
            with torch.no_grad():  # in place: a captured graph keeps reading these very tensors
                for pt, pe in zip(self.Q_target.parameters(), self.Q_eval.parameters()):
                    pt.copy_(pe)
            self._next_target_sync = (self.mem_cntr // self.target_update_freq + 1) * self.target_update_freq
            self.target_syncs += 1
        # one factor eps_dec per transition stored since the schedule was last charged (reference: per learn() = per transition)
        n_new = self.mem_cntr - self._eps_cntr
        if n_new > 0:
            self.epsilon = max(self.epsilon * math.pow(self.eps_dec, n_new), self.eps_end)
            self._eps_cntr = self.mem_cntr
        self.last_loss = loss
        return self.last_loss

    # whole-agent checkpoint like the reference's pickle (Training_DQN_pytorch.py:373-376), without the replay
    def state_dict(self):
        return dict(q_eval=self.Q_eval.state_dict(), q_target=self.Q_target.state_dict(), optimizer=self.optimizer.state_dict(),
                    epsilon=self.epsilon, mem_cntr=self.mem_cntr, updates=self.updates, target_syncs=self.target_syncs,
                    act_calls=self._act_calls, fused=self.fused)

    def load_state_dict(self, sd):
        self.Q_eval.load_state_dict(sd["q_eval"])
        self.Q_target.load_state_dict(sd["q_target"])
        self.optimizer.load_state_dict(sd["optimizer"])
        self._act_calls = int(sd.get("act_calls", 0))
        self.epsilon = sd["epsilon"]
        self.updates, self.target_syncs = sd.get("updates", 0), sd.get("target_syncs", 0)
        # The replay memory is not checkpointed (the reference pickles it with the agent), so the transition counter
        # restarts at what this process has stored: the sync cadence is re-anchored to THAT counter -- a sync within
        # target_update_freq transitions of the resume, as in an uninterrupted run -- never to the old run's total.
        self._eps_cntr = self.mem_cntr
        self._next_target_sync = (self.mem_cntr // self.target_update_freq + 1) * self.target_update_freq


class BatchedDQNAgent(_ReplayAgent):
    """DQNAgent (Training_DQN_pytorch.py:70-197) with [N]-batched choose_action/store_transition and device replay."""

    def __init__(self, gamma=.99, epsilon=1.0, lr=.0005, input_dims=11, batch_size=2500, n_actions=8,
                 max_mem_size=500000, eps_end=0.2, eps_dec=.999997, fc1_dims=256, fc2_dims=256,
                 target_update_freq=100000, device="cpu", seed=0, use_graph=True, fused=None):
        def make_net():
            net = DeepQNetwork(lr, input_dims, fc1_dims, fc2_dims, n_actions).to(device)
            if torch.device(device).type == "cuda":
                net.optimizer = torch.optim.Adam(net.parameters(), lr=lr, fused=True, capturable=True)
            return net
        super().__init__(make_net, (input_dims,), torch.float32, gamma, epsilon, batch_size, n_actions, max_mem_size, eps_end, eps_dec,
                         target_update_freq, device, seed)
        self.use_graph = bool(use_graph)
        self._lr, self._betas, self._adam_eps = lr, (0.9, 0.999), 1e-8
        # The fused learn step (include/roborugby_amd.h: rr_dqn_update; csrc/rr_dqn.hip): forward of both nets, TD target,
        # backward, weight-gradient reduction and Adam in two launches on the fp32 matrix cores -- for exactly this network
        # (11 -> 256 -> 256 -> 8) on the GPU, batch a multiple of 64.  Default: on whenever it applies.  Off: the PyTorch path
        # (autograd + torch.optim.Adam), which is also the reference the fused step is tested against.
        can_fuse = (self.device.type == "cuda" and (input_dims, fc1_dims, fc2_dims, n_actions) == (11, 256, 256, 8)
                    and self.batch_size % 64 == 0)
        self._open_handle(fused, can_fuse, "a GPU, the reference's 11-256-256-8 network and a batch that is a multiple of 64")
        if self.fused:
            self._fused_loss = torch.zeros(1, device=self.device)

    optimizer = property(lambda self: self.Q_eval.optimizer)  # (where the reference keeps it)

    @torch.no_grad()
    def choose_action(self, observation, epsilon_override=None):
        """[N,11] -> int32 [N]: epsilon-greedy per arena (Training_DQN_pytorch.py:138-149)."""
        eps = self.epsilon if epsilon_override is None else epsilon_override
        n = observation.shape[0]
        if self.fused and n % 64 == 0 and observation.dtype == torch.float32 and observation.shape[1] == 11:
            return self._act_fused(observation, eps)  # one launch: tiled forward on the matrix cores + argmax + epsilon draw
        return self._epsilon_greedy(self.Q_eval(observation).argmax(dim=1), eps)

    @torch.no_grad()
    def store_transition(self, state, action, reward, state_, done, valid=None):
        """Appends N transitions to the ring (Training_DQN_pytorch.py:126-136); rows with valid=False are skipped
        (the dummy transition of an arena that was only re-placed by auto-reset)."""
        if (self.fused and state.dtype == torch.float32 and state_.dtype == torch.float32 and reward.dtype == torch.float32
                and state.shape[0] <= self.mem_size):
            return self._store_fused(state, action, reward, state_, done, valid)
        self._ring_write(*self._compact(state, action, reward, state_, done, valid))

    def _store_fused(self, state, action, reward, state_, done, valid):
        """rr_dqn_store: the compaction of the valid rows and the five ring writes in one launch"""
        n = state.shape[0]
        s, s2, r = state.contiguous(), state_.contiguous(), reward.contiguous()
        a = action.to(torch.int32).contiguous()
        d = done.to(torch.bool).contiguous()
        v = valid.to(torch.bool).contiguous() if valid is not None else None
        if not hasattr(self, "_store_count"):
            self._store_count = torch.zeros(1, dtype=torch.int32, device=self.device)
        p = _lib.ptr
        self._dqn.launch("rr_dqn_store", p(s), p(a), p(r), p(s2), p(d), p(v), n, self.mem_cntr, self.mem_size, p(self.state_memory),
                         p(self.new_state_memory), p(self.action_memory), p(self.reward_memory), p(self.terminal_memory), p(self._store_count))
        self.mem_cntr += n if v is None else int(self._store_count.item())  # (the one host read of the call, as in the PyTorch path)

    def _act_fused(self, observation, eps):
        obs = observation.contiguous()
        n = obs.shape[0]
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        self._act_calls += 1
        self._dqn.act(self.Q_eval.parameters(), obs, n, eps, self._seed, self._act_calls, out)
        self._keep_obs = obs  # read asynchronously
        return out

    def _fused_args(self, batch):
        a =_lib.RRDqnArgs()
        a.struct_size, a.batch = C.sizeof(_lib.RRDqnArgs), int(batch.shape[0])
        for k, (pe, pt) in enumerate(zip(self.Q_eval.parameters(), self.Q_target.parameters())):
            assert pe.is_contiguous() and pt.is_contiguous() and pe.dtype == torch.float32
            a.eval_params[k], a.target_params[k] = pe.data_ptr(), pt.data_ptr()
        a.state_memory, a.new_state_memory = self.state_memory.data_ptr(), self.new_state_memory.data_ptr()
        a.action_memory, a.reward_memory = self.action_memory.data_ptr(), self.reward_memory.data_ptr()
        a.terminal_memory, a.batch_index = self.terminal_memory.data_ptr(), batch.data_ptr()
        a.gamma, a.lr = self.gamma, self._lr
        a.beta1, a.beta2, a.eps = self._betas[0], self._betas[1], self._adam_eps
        a.loss_out = self._fused_loss.data_ptr()
        return a

    def _learn_fused(self, max_mem):
        """sampling in PyTorch (one or two kernels), everything else in rr_dqn_update's two launches"""
        batch = self._sample(max_mem).contiguous()
        self._dqn.launch("rr_dqn_update", C.byref(self._fused_args(batch)))
        self._keep = batch  # the launch reads it asynchronously
        return self._fused_loss[0]

    def fused_grads(self, batch):
        """gradient of the loss on the given replay rows as rr_dqn_grads computes it, as a dict keyed like Q_eval's parameters"""
        n = self._rrlib.rr_dqn_param_count()
        flat = torch.empty(n, device=self.device)
        args = self._fused_args(batch.contiguous())
        self._dqn.launch("rr_dqn_grads", C.byref(args), _lib.ptr(flat))
        torch.cuda.current_stream(self.device).synchronize()
        names = ["fc2.weight", "fc1.weight", "fc3.weight", "fc1.bias", "fc2.bias", "fc3.bias"]  # the handle's flat order
        shapes = dict(self.Q_eval.named_parameters())
        out, off = {}, 0
        for nm in names:
            k = shapes[nm].numel()
            out[nm] = flat[off:off + k].view_as(shapes[nm]).clone()
            off += k
        return out, float(self._fused_loss[0])

    def _try_capture(self, max_mem):
        """Once the replay memory is full the learn step has a fixed shape: capture it into a HIP graph (the step is ~25
        small kernels and launch-bound).  Any failure leaves the eager path in place.  The warm-up iterations PyTorch wants
        before a capture are REAL Adam steps on a side stream; afterwards the parameters, the optimizer state (moments, step
        count) and the sampling generator are restored from the copies taken on entry, so a graph run makes exactly the updates
        -- and the random draws -- an eager run makes."""
        self._graph_tried = True
        opt = self.Q_eval.optimizer
        saved_opt = copy.deepcopy(opt.state_dict())
        saved_gen = self.gen.get_state()
        saved_params = [p.detach().clone() for p in self.Q_eval.parameters()]
        try:
            g = torch.cuda.CUDAGraph()
            if hasattr(g, "register_generator_state"):
                g.register_generator_state(self.gen)
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                for _ in range(2):
                    self._learn_core(max_mem)
            torch.cuda.current_stream(self.device).wait_stream(side)
            with torch.no_grad():  # undo the warm-up: parameters, Adam moments / step count, generator
                for p, q in zip(self.Q_eval.parameters(), saved_params):
                    p.copy_(q)
            opt.load_state_dict(saved_opt)
            self.gen.set_state(saved_gen)
            with torch.cuda.graph(g):
                self._graph_loss = self._learn_core(max_mem)
            self._graph, self._graph_mem = g, max_mem
        except Exception as ex:  # noqa: BLE001 -- eager is always available
            self._graph = None
            with torch.no_grad():
                for p, q in zip(self.Q_eval.parameters(), saved_params):
                    p.copy_(q)
            opt.load_state_dict(saved_opt)
            self.gen.set_state(saved_gen)
            print(f"[dqn] learn() stays eager (graph capture failed: {type(ex).__name__}: {ex})", flush=True)

    def _learn_step(self, max_mem):
        if self.fused:
            return self._learn_fused(max_mem)
        if self.use_graph and self.device.type == "cuda" and max_mem == self.mem_size and not getattr(self, "_graph_tried", False):
            self._try_capture(max_mem)
        if getattr(self, "_graph", None) is not None and self._graph_mem == max_mem:
            self._graph.replay()
            return self._graph_loss
        return self._learn_core(max_mem)

    def _fused_adam(self, state=None):
        """the fused step's Adam moments + step count out of (state=None) or into the handle"""
        n = self._rrlib.rr_dqn_param_count()
        if state is None:
            m1, m2 = torch.empty(n, device=self.device), torch.empty(n, device=self.device)
            step = C.c_int64(0)
        else:
            m1, m2 = state["exp_avg"].to(self.device).contiguous(), state["exp_avg_sq"].to(self.device).contiguous()
            step = C.c_int64(int(state["step"]))
        self._dqn.launch("rr_dqn_adam_state", _lib.ptr(m1), _lib.ptr(m2), C.byref(step), 0 if state is None else 1)
        torch.cuda.current_stream(self.device).synchronize()
        return dict(exp_avg=m1, exp_avg_sq=m2, step=step.value)

    # flat layout of the fused step's Adam moments (csrc/rr_dqn.hip: OFF_W2, OFF_W1, OFF_W3, OFF_B1, OFF_B2, OFF_B3) as indices
    # into Q_eval.parameters() = fc1.weight, fc1.bias, fc2.weight, fc2.bias, fc3.weight, fc3.bias
    _FUSED_ORDER = (2, 0, 4, 1, 3, 5)

    def _flat_from_torch_adam(self, opt_sd):
        """torch.optim.Adam state_dict -> the fused layout; None if the optimizer was never stepped"""
        st = opt_sd.get("state", {})
        if len(st) < 6:
            return None
        params = list(self.Q_eval.parameters())
        cat = lambda key: torch.cat([st[k][key].detach().to(self.device, torch.float32).reshape(-1) for k in self._FUSED_ORDER])
        step = int(torch.as_tensor(st[0]["step"]).item())
        assert sum(params[k].numel() for k in self._FUSED_ORDER) == cat("exp_avg").numel()
        return dict(exp_avg=cat("exp_avg"), exp_avg_sq=cat("exp_avg_sq"), step=step)

    def _torch_adam_from_flat(self, flat):
        """the fused layout -> the `state` part of a torch.optim.Adam state_dict for Q_eval's parameters"""
        params = list(self.Q_eval.parameters())
        state, off = {}, 0
        for k in self._FUSED_ORDER:
            n = params[k].numel()
            state[k] = dict(step=torch.tensor(float(flat["step"]), device=self.device),
                            exp_avg=flat["exp_avg"][off:off + n].reshape(params[k].shape).clone(),
                            exp_avg_sq=flat["exp_avg_sq"][off:off + n].reshape(params[k].shape).clone())
            off += n
        return state

    def state_dict(self):
        """Both optimizer representations travel, so a checkpoint written by the fused agent resumes under --no-fused and the
        other way round: `optimizer` (torch.optim.Adam's) and `fused_adam` (flat moments + step) describe the same Adam state."""
        sd = dict(super().state_dict(), next_target_sync=self._next_target_sync)
        opt = sd["optimizer"]
        if self.fused:
            sd["fused_adam"] = self._fused_adam()
            if sd["fused_adam"]["step"] > 0:  # the torch optimizer is never stepped in fused mode: write the moments in its format too
                opt = dict(opt, state=self._torch_adam_from_flat(sd["fused_adam"]))
        else:
            flat = self._flat_from_torch_adam(opt)
            if flat is not None:
                sd["fused_adam"] = flat
        sd["optimizer"] = opt
        return sd

    def load_state_dict(self, sd, lr_override=0.0, epsilon_override=0.0, eps_dec_override=0.0):
        super().load_state_dict(sd)
        if self.fused:
            flat = sd.get("fused_adam") or self._flat_from_torch_adam(sd["optimizer"])
            if flat is not None:
                self._fused_adam(flat)
            elif sd.get("updates", 0) > 0:
                import warnings
                warnings.warn("checkpoint carries no Adam moments for the fused learn step: Adam restarts from zero moments")
        if lr_override > 0:  # Training_DQN_pytorch.py:297-303
            self._lr = lr_override
            for g in self.Q_eval.optimizer.param_groups:
                g["lr"] = lr_override
        if epsilon_override > 0:
            self.epsilon = epsilon_override
        if eps_dec_override > 0:
            self.eps_dec = eps_dec_override


class PixelQNetwork(nn.Module):
    """The fixed convolutional Q network of the pixel agent (include/roborugby_amd.h: rr_cnn_act): uint8 [n, C, 64, 64] -> conv 8x8 / 4 (16)
    -> conv 4x4 / 2 (32) -> 1152 -> 256 -> n_actions, ReLU between.  The input is pixel * 2^-8 (not / 255): exact in every precision."""

    def __init__(self, channels, n_actions=8):
        super().__init__()
        self.conv1 = nn.Conv2d(channels, 16, 8, stride=4)
        self.conv2 = nn.Conv2d(16, 32, 4, stride=2)
        self.fc1 = nn.Linear(32 * 6 * 6, 256)
        self.fc2 = nn.Linear(256, n_actions)

    def forward(self, x):
        x = x.to(self.conv1.weight.dtype) * (1 / 256)
        x = F.relu(self.conv1(x))
        x = F.relu(self.conv2(x))
        x = F.relu(self.fc1(x.flatten(1)))
        return self.fc2(x)


class PixelDQNAgent(_ReplayAgent):
    """BatchedDQNAgent's surface on the pixels of PixelObservation(size=64, stack=channels / 3).  Acting -- every row, every step -- is
    rr_cnn_act (one HIP kernel on the bf16 matrix cores, csrc/rr_cnn.hip) where it applies: on the GPU, contiguous uint8 rows, channels
    in {3, 6, 9, 12}, 8 actions; anything else, and fused=False, goes through the torch module.  Learning is PyTorch autograd on the same
    parameters (MSE on r + gamma max Q_target, Adam, target sync and the epsilon schedule: _ReplayAgent's).
    replay="dense" (the default): the replay ring holds both stacked observations of a transition as uint8 frames and is written with torch
    indexing (store_transition): 2 * channels * 4096 + 13 bytes per transition.
    replay="frames": a FrameReplay (frame_replay.py; rr_frames_push / rr_frames_sample) of `replay_rows` rows x `replay_slots` vector steps
    that holds every frame once, 12,298 bytes per transition; no dense observation memory is allocated.  The loop calls
    store_step(pixels, action, reward, done, valid, first) once per vector step (and once without a transition after a reset); learn()
    draws its batch with rr_frames_sample and averages the same TD loss over the rows the sampler found a transition for.  mem_size is the
    replay's capacity.  mem_cntr advances by `replay_rows` per push that carries transitions: re-placement rows -- at most one per episode
    and row -- are COUNTED, because telling them apart would take a host read per step (the schedules run that little ahead)."""
    FUSED_CHANNELS = (3, 6, 9, 12)
    PERMUTE_LIMIT = math.inf  # always a permutation: a ring of frames never grows to where one costs

    def __init__(self, channels=12, gamma=.99, epsilon=1.0, lr=.0005, batch_size=256, n_actions=8, max_mem_size=65536, eps_end=0.2,
                 eps_dec=.999997, target_update_freq=100000, device="cpu", seed=0, fused=None, replay="dense", replay_rows=None,
                 replay_slots=None):
        self.channels = int(channels)
        if replay not in ("dense", "frames"):
            raise ValueError("PixelDQNAgent(replay=...): 'dense' or 'frames'")
        self.replay_kind, self.replay = replay, None
        super().__init__(lambda: PixelQNetwork(self.channels, n_actions).to(device), (self.channels, 64, 64), torch.uint8, gamma, epsilon,
                         batch_size, n_actions, max_mem_size, eps_end, eps_dec, target_update_freq, device, seed, dense_memory=replay == "dense")
        self.optimizer = torch.optim.Adam(self.Q_eval.parameters(), lr=lr)
        can_fuse = self.device.type == "cuda" and self.channels in self.FUSED_CHANNELS and n_actions == 8
        self._open_handle(fused, can_fuse, "a GPU, 3 / 6 / 9 / 12 channels and 8 actions")
        if replay == "frames":
            from .frame_replay import FrameReplay
            if self.device.type != "cuda" or self.channels % 3 or replay_rows is None or replay_slots is None:
                raise ValueError("PixelDQNAgent(replay='frames') needs a GPU, channels = 3 * stack, replay_rows and replay_slots")
            self.replay = FrameReplay(replay_rows, replay_slots, self.channels // 3, device=self.device, seed=seed, dqn=self._dqn)
            self.mem_size = self.replay.capacity
            self._sampled = None

    def close(self):
        if self.replay is not None:
            self.replay.close()
        super().close()

    def _rows(self, pixels):
        if pixels.dim() == 5:  # PixelObservation with several robots: [N, R, C, 64, 64], a row per (arena, robot)
            pixels = pixels.reshape(-1, *pixels.shape[2:])
        if pixels.dim() != 4 or tuple(pixels.shape[1:]) != (self.channels, 64, 64):
            raise ValueError(f"pixels: [n, {self.channels}, 64, 64] or [N, R, {self.channels}, 64, 64], not {tuple(pixels.shape)}")
        return pixels

    @torch.no_grad()
    def choose_action(self, pixels, epsilon_override=None, qvalues=None):
        """[n, C, 64, 64] (or [N, R, C, 64, 64]) -> int32 [n]: epsilon-greedy per row.  qvalues: a float32 [n, 8] tensor the fused path
        fills with the Q-values it acted on (None: not written)."""
        eps = self.epsilon if epsilon_override is None else epsilon_override
        pixels = self._rows(pixels)
        n = pixels.shape[0]
        if (self.fused and pixels.dtype == torch.uint8 and pixels.is_contiguous() and pixels.data_ptr() % 16 == 0 and 1 <= n <= 1 << 22
                and pixels.device == self.Q_eval.fc2.weight.device):
            return self._act_fused(pixels, eps, qvalues)
        q = self.Q_eval(pixels)
        if qvalues is not None:
            qvalues.copy_(q)
        return self._epsilon_greedy(q.argmax(dim=1), eps)

    def _act_fused(self, pixels, eps, qvalues=None):
        n = pixels.shape[0]
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        params = list(self.Q_eval.parameters())
        assert all(p.is_contiguous() and p.dtype == torch.float32 for p in params)
        if qvalues is not None:
            assert qvalues.dtype == torch.float32 and qvalues.is_contiguous() and tuple(qvalues.shape) == (n, 8)
        ptrs = (C.c_void_p * 8)(*[p.data_ptr() for p in params])
        self._act_calls += 1
        self._dqn.launch("rr_cnn_act", C.byref(ptrs), _lib.ptr(pixels), n, self.channels, float(min(max(eps, 0.0), 1.0)), int(self._seed),
                         self._act_calls & 0xFFFFFFFF, _lib.ptr(out), _lib.ptr(qvalues))
        return out

    @torch.no_grad()
    def store_step(self, pixels, action=None, reward=None, done=None, valid=None, first=None):
        """replay="frames": one vector step into the FrameReplay -- the observation AFTER the step (its newest frame is stored), the action
        that led to it, reward, done, valid (the rows whose step was a transition) and first (the rows whose stack restarted: WAS_RESET).
        With only `pixels`: the observation after a reset / restart, which ends no transition and starts every stack over."""
        if self.replay is None:
            raise RuntimeError("store_step belongs to replay='frames'; the dense replay takes store_transition")
        if action is None:
            self.replay.restart()
        self.replay.push(pixels, first, action, reward, done, valid)
        if action is not None:
            self.mem_cntr += self.replay.rows

    def _learn_frames(self, max_mem):
        """_learn_core on a batch of rr_frames_sample: the TD loss averaged over the rows with ok, sum(ok * err^2) / max(sum(ok), 1) --
        F.mse_loss whenever every row is ok"""
        self._sampled = self.replay.sample(self.batch_size, out=self._sampled)
        state, state_, action, reward, terminal, ok = self._sampled
        self.optimizer.zero_grad(set_to_none=False)
        q_eval = self.Q_eval(state).gather(1, action.long().view(-1, 1)).squeeze(1)
        with torch.no_grad():
            q_next = self.Q_target(state_).masked_fill(terminal.view(-1, 1), 0.0)
            q_target = reward + self.gamma * q_next.max(dim=1)[0]
            w = ok.float()
        loss = (w * (q_eval - q_target) ** 2).sum() / w.sum().clamp(min=1.0)
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    def _learn_step(self, max_mem):
        return self._learn_frames(max_mem) if self.replay is not None else self._learn_core(max_mem)

    @torch.no_grad()
    def store_transition(self, state, action, reward, state_, done, valid=None):
        """Appends the rows with valid=True (None: all) to the ring, in row order"""
        if self.replay is not None:
            raise RuntimeError("PixelDQNAgent(replay='frames') stores whole vector steps: call store_step(pixels, action, reward, done, "
                               "valid, first), not store_transition")
        rows = self._compact(self._rows(state), action, reward, self._rows(state_), done, valid)
        if rows[0].shape[0] > self.mem_size:
            raise ValueError(f"{rows[0].shape[0]} transitions in one call do not fit a replay ring of {self.mem_size}")
        self._ring_write(*rows)

    def state_dict(self):
        """the agent without its replay (as BatchedDQNAgent's)"""
        return dict(super().state_dict(), kind="pixel", channels=self.channels)

    def load_state_dict(self, sd):
        if sd.get("kind") != "pixel" or int(sd["channels"]) != self.channels:
            raise ValueError(f"not a checkpoint of a pixel agent with {self.channels} channels")
        super().load_state_dict(sd)


@torch.no_grad()
def evaluate(env, policy, episodes=1):
    """Mean return per episode of `policy(obs) -> int32 [N]` over every arena of `env` (auto-reset env, time_limit rule):
    resets, then plays `episodes` full episodes; steps that only re-place an arena carry reward 0."""
    obs = env.reset()
    total = torch.zeros(env.num_envs, device=env.device, dtype=torch.float64)
    T = env.spec.max_episode_steps
    n_steps = episodes * T + (episodes - 1)  # one re-placing call between consecutive episodes
    for _ in range(n_steps):
        obs, reward, done, info = env.step(policy(obs).view(-1, 1))
        total += reward.double()
    return float(total.mean() / episodes), float(total.std() / episodes)


def _log_progress(step, agent, env):
    """the progress line of train() / train_pixels()"""
    torch.cuda.synchronize()
    lr_, _, _, cnt = env.episode_stats()
    fin = cnt > 0
    avg = float(lr_[fin].mean()) if bool(fin.any()) else float("nan")
    print(f"step {step} epsilon {agent.epsilon:.6f} updates {agent.updates} target-syncs {agent.target_syncs} finished-episodes "
          f"{int(cnt.sum())} avg-last-return {avg:.1f} loss {float(agent.last_loss) if agent.last_loss is not None else float('nan'):.4f}", flush=True)


def _save_checkpoint(path, agent, **rest):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(dict(agent=agent.state_dict(), **rest), path)


def _write_result(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def _train_result(agent, env, env_steps, seconds, steps, transitions, step_budget_clocks, updates_per_step, rows_per_step, overlap,
                  eps_dec, eps_end, fused_learn_step, mean_step_reward, preset, dtype, curve):
    """what train() and train_pixels() both report; updates_per_step: 0 where nothing was learnt"""
    return dict(env_steps_per_sec=env_steps / seconds, seconds=seconds, num_envs=env.num_envs, steps=steps, transitions=transitions,
                step_budget_clocks=step_budget_clocks, learn_calls=agent.updates, updates_per_step=updates_per_step,
                batch_size=agent.batch_size, samples_per_transition=updates_per_step * agent.batch_size / rows_per_step if updates_per_step else 0.0,
                overlap_learn=overlap, replay_transitions=agent.mem_size, target_update_freq=agent.target_update_freq,
                target_syncs=agent.target_syncs, epsilon=agent.epsilon, eps_dec=eps_dec, eps_end=eps_end,
                finished_episodes=int(env.episode_stats()[3].sum()), fused_learn_step=fused_learn_step, mean_step_reward=mean_step_reward,
                preset=preset, dtype=dtype, curve=curve)


def train(num_envs=65536, steps=300, preset="T", device="cuda:0", seed=0, checkpoint=None, resume=None,
          log_every=50, learn=True, mem_size=None, dtype="f64", updates_per_step=4, batch_size=None,
          replay_vector_steps=32, target_sync_vector_steps=64, eps_dec=.999997, eps_end=0.2, eval_every=0,
          eval_envs=16384, out=None, overlap_learn=True, step_budget_clocks=0, fused=None):
    """The main loop of Training_DQN_pytorch.py:317-377 over a batched env.  Returns a dict of throughput / score /
    the return curve (greedy policy vs the random policy on a separate evaluation batch, every `eval_every` steps).

    overlap_learn: the k gradient steps that follow a vector step run on a second HIP stream WHILE the simulator steps the
    next one (under a contact-seeking policy `k_step` is one long launch bound by its slowest arenas and leaves most CUs idle).
    Stream-ordered, deterministic: choose_action(t) -> [side: learn x k on the replay up to t-1] || [main: env.step(t)] ->
    store_transition(t) waits for the side stream -> choose_action(t+1).  The updates see the replay one vector step later
    than in the serial order (same number of updates, same schedules)."""
    import roborugby_amd as rr
    # step_budget_clocks > 0: the budgeted step (include/roborugby_amd.h) -- an arena whose step is still in progress reports
    # NOT_READY; its row is no transition yet, and the transition it completes later carries the action it ACCEPTED
    env = rr.make("RoboRugbySimpleDuel-v3", num_envs=num_envs, preset=preset, device=device, seed=seed, dtype=dtype,
                  step_budget_clocks=step_budget_clocks)
    p = env.preset
    if p.game_mode:  # Training_DQN_pytorch.py:233-234
        raise Exception("Game mode settings are enabled in RR_Constants.")
    n_teams = 2 if p.nr_grumpy > 0 else 1
    B = int(batch_size or min(32768, max(env.spec.max_episode_steps * 8 + 100, num_envs // 2)))
    agent = BatchedDQNAgent(input_dims=env.observation_space.shape[0], batch_size=B, n_actions=env.action_space.n, device=device,
                            seed=seed, max_mem_size=mem_size or max(500000, replay_vector_steps * num_envs * n_teams),
                            target_update_freq=max(100000, target_sync_vector_steps * num_envs * n_teams),
                            eps_dec=eps_dec, eps_end=eps_end, fused=fused)
    if resume:
        ck = torch.load(resume, map_location=device)
        agent.load_state_dict(ck["agent"])
        env.load_checkpoint_state(ck)  # state, episode bookkeeping (the episode index keys the reset RNG), parity build: the scratch rect
        observation = env.get_game_state()
    else:
        observation = env.reset()
    grumpy = p.nr_grumpy > 0
    obs_grumpy = env.get_game_state(int_team=-1) if grumpy else None
    eval_env, curve = None, []
    if eval_every:
        eval_env = rr.make("RoboRugbySimpleDuel-v3", num_envs=eval_envs, preset=preset, device=device, seed=seed + 1000003, dtype=dtype)
        gen = torch.Generator(device=device)
        gen.manual_seed(seed + 7)
        rand_ret, rand_std = evaluate(eval_env, lambda o: torch.randint(0, 8, (o.shape[0],), generator=gen, device=o.device, dtype=torch.int32))
        curve.append(dict(env_steps=0, vector_steps=0, greedy_return=None, random_return=rand_ret, epsilon=agent.epsilon))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t_eval = 0.0
    score_sum = torch.zeros(num_envs, device=device)
    real_rows = torch.zeros((), dtype=torch.int64, device=device)  # rows that were transitions (not re-placements, not NOT_READY)
    overlap = bool(overlap_learn and learn and torch.device(device).type == "cuda")
    main_stream = torch.cuda.current_stream(torch.device(device))
    side = torch.cuda.Stream(device=torch.device(device)) if overlap else None
    parked = None  # budgeted step: arenas whose step was still in progress after the last call
    for i in range(steps):
        action = agent.choose_action(observation)
        if grumpy:
            action_grumpy = agent.choose_action(obs_grumpy)
        if parked is not None:  # a parked arena ignores the new action: the transition it will complete belongs to the one it accepted
            action = torch.where(parked, accepted, action)
            if grumpy:
                action_grumpy = torch.where(parked, accepted_g, action_grumpy)
        acts = action.view(-1, 1)
        learned = None
        if overlap:  # the gradient steps on what the replay holds so far, next to the simulator's step
            chosen = torch.cuda.Event()
            chosen.record(main_stream)
            with torch.cuda.stream(side):
                side.wait_event(chosen)  # choose_action has read Q_eval
                for _ in range(updates_per_step):
                    agent.learn()
                learned = torch.cuda.Event()
                learned.record(side)
        if step_budget_clocks and checkpoint and i == steps - 1:
            # a checkpoint must not catch an arena parked mid-step (rr_set_state on resume would drop the rest of that step and
            # the action it accepted): the last call before it runs synchronously -- parked arenas finish, nobody parks
            env.set_step_budget(0)
        observation_, reward, done, info = env.step(acts)
        real = (info.status & (STATUS_WAS_RESET | STATUS_NOT_READY)) == 0  # a call that only re-placed the arena, or left its step unfinished, is not a transition
        if step_budget_clocks:
            parked, accepted = (info.status & STATUS_NOT_READY) != 0, action
            if grumpy:
                accepted_g = action_grumpy
        score_sum += reward
        real_rows += real.sum()
        if learn:
            if learned is not None:
                main_stream.wait_event(learned)  # the sampled rows are read, Q_eval is written: the ring and the net are ours again
            agent.store_transition(observation, action, reward, observation_, done, valid=real)
            if grumpy:
                agent.store_transition(obs_grumpy, action_grumpy, info.dblGrumpyScore, info.adblGrumpyState, done, valid=real)
            if not overlap:
                for _ in range(updates_per_step):
                    agent.learn()
        observation = observation_
        obs_grumpy = info.adblGrumpyState
        if log_every and (i + 1) % log_every == 0:
            _log_progress(i + 1, agent, env)
        if eval_every and (i + 1) % eval_every == 0:
            torch.cuda.synchronize()
            te = time.perf_counter()
            g_ret, g_std = evaluate(eval_env, lambda o: agent.choose_action(o, epsilon_override=0.0))
            curve.append(dict(env_steps=(i + 1) * num_envs, vector_steps=i + 1, greedy_return=g_ret, greedy_return_std=g_std,
                              random_return=rand_ret, epsilon=agent.epsilon, updates=agent.updates, target_syncs=agent.target_syncs))
            print(f"[eval] after {(i + 1) * num_envs:,} env-steps: greedy return {g_ret:.1f} (random policy {rand_ret:.1f})", flush=True)
            torch.cuda.synchronize()
            t_eval += time.perf_counter() - te
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0 - t_eval
    if checkpoint:
        _save_checkpoint(checkpoint, agent, **env.checkpoint_state())
    n_real = int(real_rows.item())
    # env steps = the rows that stepped an arena (auto-reset calls count, as in bench.py's random line they are subtracted only there;
    # NOT_READY rows of the budgeted step never count)
    env_steps = num_envs * steps if not step_budget_clocks else n_real
    res = _train_result(agent, env, env_steps, dt, steps, n_real, step_budget_clocks, updates_per_step if learn else 0, num_envs * n_teams,
                        overlap, eps_dec, eps_end, bool(agent.fused), float(score_sum.mean() / steps), preset, dtype, curve)
    if eval_every:
        # throughput of the rollout alone under the policy training converged to (greedy, contact-seeking), next to the random policy's
        for name, pol in (("greedy", lambda o: agent.choose_action(o, epsilon_override=0.0)),
                          ("random", lambda o: torch.randint(0, 8, (o.shape[0],), device=o.device, dtype=torch.int32))):
            o = env.reset()
            torch.cuda.synchronize()
            ts = time.perf_counter()
            for _ in range(200):
                o, _, _, _ = env.step(pol(o).view(-1, 1))
            torch.cuda.synchronize()
            res[f"rollout_env_steps_per_sec_{name}_policy"] = num_envs * 200 / (time.perf_counter() - ts)
        eval_env.close()
    env.close()
    if out:
        _write_result(out, res)
    return res


@torch.no_grad()
def play_hive(checkpoint, num_envs=4096, steps=300, device="cuda:0", seed=0, epsilon=0.2, preset="G", step_budget_clocks=0,
              record=None, record_arenas=16, record_size=96, record_every=1, record_view="field"):
    """A checkpoint written by train() plays the full game: the happy team is the hive (players.Hive: the reference's
    DQN_pytorch_player.Stephen -- one policy, one ball per robot), the grumpy team is OG_Twitchy, the line-up of the reference's
    main.py without its human.  Returns mean return per team over the steps played (per finished episode when any finished) and
    env-steps/s (HIP events around the loop: policy + step).  step_budget_clocks > 0: the budgeted step -- the hive holds the rows of
    arenas parked mid-step (players.Hive), a call's rewards count for the arenas whose step completed in it, and env-steps are the rows
    that stepped an arena (neither re-placed nor NOT_READY), as in train().
    record: path of an animated GIF of the run -- after every `record_every`-th step one render_batch of the first `record_arenas` arenas,
    `record_size` pixels wide (a multiple of 4; the height keeps the arena's aspect); the frames stay on the device until the loop ends,
    then one contact sheet per recorded step goes into the GIF.  None: nothing is rendered.
    record_view: "field" -- the whole arena --, or "ego": what the first hive robot of each recorded arena sees (render_ego: the robot
    in the centre, its front up, 400 arena units across, `record_size` x `record_size` pixels)."""
    import roborugby_amd as rr
    from .players import Hive, og_twitchy
    env = rr.BatchedRoboRugbyEnv(num_envs, preset=preset, device=device, seed=seed, action_mode="thrust",
                                 step_budget_clocks=step_budget_clocks)
    p = env.preset
    agent = BatchedDQNAgent(batch_size=64, max_mem_size=64, device=device, seed=seed)
    agent.load_state_dict(torch.load(checkpoint, map_location=device)["agent"])
    hive = Hive(env, agent, epsilon=epsilon, seed=seed)
    gen = torch.Generator(device=env.device)
    gen.manual_seed(seed + 1)
    env.reset()
    thrust = torch.zeros(num_envs, 2 * p.nr, dtype=torch.float32, device=env.device)
    total_h = torch.zeros(num_envs, dtype=torch.float64, device=env.device)
    total_g = torch.zeros(num_envs, dtype=torch.float64, device=env.device)
    real_rows = torch.zeros((), dtype=torch.int64, device=env.device)
    parked_rows = torch.zeros((), dtype=torch.int64, device=env.device)
    if record_view not in ("field", "ego"):
        raise ValueError("play_hive(record_view=...): 'field' or 'ego'")
    if record is not None:
        rec_n, rec_every = min(int(record_arenas), num_envs), max(int(record_every), 1)
        rec_w, rec_h = int(record_size), max(int(round(record_size * p.arena_h / p.arena_w)), 1)
        if record_view == "ego":
            rec_h = rec_w
        rec_idx = torch.arange(rec_n, dtype=torch.int32, device=env.device)
        clip = torch.empty((len(range(rec_every - 1, steps, rec_every)), rec_n, rec_h, rec_w, 3), dtype=torch.uint8, device=env.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(steps):
        if p.nr_grumpy:
            thrust[:, 2 * p.nr_happy:] = og_twitchy(num_envs, p.nr_grumpy, generator=gen, device=env.device)
        hive.act(out=thrust)
        _, reward, _, info = env.step_thrust(thrust)
        if record is not None and (k + 1) % rec_every == 0:
            if record_view == "ego":
                env.render_ego(rec_idx, int(hive.robots[0]), rec_w, rec_h, span=400.0, out=clip[(k + 1) // rec_every - 1])
            else:
                env.render_batch(rec_idx, rec_w, rec_h, out=clip[(k + 1) // rec_every - 1])
        if step_budget_clocks:  # (a NOT_READY row's reward is not written by the step)
            ready = (info.status & STATUS_NOT_READY) == 0
            total_h += torch.where(ready, reward, 0.0)
            total_g += torch.where(ready, info.dblGrumpyScore, 0.0)
            parked_rows += (~ready).sum()
            real_rows += ((info.status & (STATUS_WAS_RESET | STATUS_NOT_READY)) == 0).sum()
        else:
            total_h += reward
            total_g += info.dblGrumpyScore
    t1.record()
    torch.cuda.synchronize(env.device)
    secs = t0.elapsed_time(t1) / 1e3
    lr, lrg, _, cnt = env.episode_stats()
    done = cnt > 0
    res = dict(mode="play_hive", preset=preset, num_envs=num_envs, steps=steps, epsilon=epsilon, hive_robots=list(hive.robots),
               return_happy=float(total_h.mean()), return_grumpy=float(total_g.mean()), episodes_finished=int(cnt.sum()),
               episode_return_happy=float(lr[done].mean()) if bool(done.any()) else None,
               episode_return_grumpy=float(lrg[done].mean()) if bool(done.any()) else None,
               env_steps_per_s=(int(real_rows) if step_budget_clocks else num_envs * steps) / secs,
               step_budget_clocks=step_budget_clocks, stepped_rows=int(real_rows) if step_budget_clocks else num_envs * steps,
               not_ready_share=int(parked_rows) / max(num_envs * steps, 1))
    if record is not None:
        from .render import contact_sheet, save_gif
        sheets = [contact_sheet(f).cpu().numpy() for f in clip]
        for k, sheet in enumerate(sheets):  # a progress bar in the top margin (it also keeps a step in which nothing moved a frame of its own)
            sheet[:2, :max(((k + 1) * sheet.shape[1]) // len(sheets), 1)] = 0
        save_gif(record, sheets, fps=env.metadata["video.frames_per_second"])
    hive.close()
    env.close()
    return res


def train_hive(num_envs=65536, steps=300, preset="G", robots=None, opponents="og_twitchy", resume=None, checkpoint=None,
               updates_per_step=4, device="cuda:0", seed=0, dtype="f64", batch_size=None, mem_size=None, replay_vector_steps=32,
               target_sync_vector_steps=64, eps_dec=.999997, eps_end=0.2, epsilon=None, learn=True, log_every=50, out=None,
               observer=None, step_budget_clocks=0):
    """Training the hive mind IN the full game: one agent, one transition per hive robot and step.  Per vector step, serial on one
    stream: hive.epsilon = agent.epsilon -> `opponents` ('og_twitchy' or None = stand still) fill the other robots' thrust columns ->
    hive.act -> env.step_thrust -> hive.store (rr_hive_transition + one rr_dqn_store over the N * NR rows) -> updates_per_step x
    agent.learn().  The reward of a row is the per-robot reward of include/roborugby_amd.h (rr_hive_transition), its next state the
    robot's view of the ball it was going for; rows without a ball / of re-placed arenas are no transitions.
    robots: the hive (None: the happy team).  resume: a checkpoint of train() or of this function -- the AGENT is taken from it (a policy
    trained in preset T is fine-tuned in G), the env starts fresh.  The checkpoint written is one play_hive reads.  Returns a dict like
    train()'s: throughput (HIP events around the loop), transitions stored, valid share, epsilon, mean per-robot reward.
    step_budget_clocks > 0: the budgeted step.  A call no longer waits for its slowest arena; an arena whose step is still in progress
    reports NOT_READY, the hive holds its rows (players.Hive) and the transition is stored by the call that completes the step, with the
    observation and the action the arena accepted.  env-steps are then the rows that stepped an arena, as in train()."""
    import roborugby_amd as rr
    from .players import Hive, og_twitchy
    if opponents not in ("og_twitchy", None):
        raise ValueError("opponents: 'og_twitchy' or None")
    env = rr.BatchedRoboRugbyEnv(num_envs, preset=preset, device=device, seed=seed, dtype=dtype, action_mode="thrust",
                                 step_budget_clocks=step_budget_clocks)  # (refuses dtype 'f32_state' with a budget)
    env.track_prior_step()  # the rewards look back on every robot's and ball's position at the step's begin
    p = env.preset
    members = tuple(range(p.nr_happy)) if robots is None else tuple(sorted({int(r) for r in robots}))
    rows = num_envs * len(members)
    B = int(batch_size or min(32768, max(64, rows // 2 // 64 * 64)))
    agent = BatchedDQNAgent(input_dims=11, batch_size=B, n_actions=8, device=device, seed=seed,
                            max_mem_size=mem_size or max(500000, replay_vector_steps * rows),
                            target_update_freq=max(100000, target_sync_vector_steps * rows), eps_dec=eps_dec, eps_end=eps_end)
    if resume:
        agent.load_state_dict(torch.load(resume, map_location=device)["agent"])
    if epsilon is not None:
        agent.epsilon = float(epsilon)
    hive = Hive(env, agent, robots=members, epsilon=agent.epsilon, seed=seed, observer=observer)
    gen = torch.Generator(device=env.device)
    gen.manual_seed(seed + 1)
    env.reset()
    thrust = torch.zeros(num_envs, 2 * p.nr, dtype=torch.float32, device=env.device)
    valid_rows = torch.zeros((), dtype=torch.int64, device=env.device)
    reward_sum = torch.zeros((), dtype=torch.float64, device=env.device)
    real_rows = torch.zeros((), dtype=torch.int64, device=env.device)  # rows that stepped an arena (not re-placed, not NOT_READY)
    parked_rows = torch.zeros((), dtype=torch.int64, device=env.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        hive.epsilon = agent.epsilon
        if opponents and len(members) < p.nr:
            thrust.copy_(og_twitchy(num_envs, p.nr, generator=gen, device=env.device))  # (the hive's columns are overwritten by act)
        hive.act(out=thrust)
        _, _, done, info = env.step_thrust(thrust)
        if learn:
            hive.store(agent, done, info.status)
            for _ in range(updates_per_step):
                agent.learn()
        else:
            hive.transition(done, info.status)
        valid_rows += hive._valid.sum()
        reward_sum += hive._reward.sum(dtype=torch.float64)  # (invalid rows carry 0)
        if step_budget_clocks:
            real_rows += ((info.status & (STATUS_WAS_RESET | STATUS_NOT_READY)) == 0).sum()
            parked_rows += ((info.status & STATUS_NOT_READY) != 0).sum()
        if log_every and (i + 1) % log_every == 0:
            torch.cuda.synchronize(env.device)
            print(f"step {i + 1} epsilon {agent.epsilon:.6f} stored {agent.mem_cntr} updates {agent.updates} mean-robot-reward "
                  f"{float(reward_sum) / max(int(valid_rows), 1):.4f} loss "
                  f"{float(agent.last_loss) if agent.last_loss is not None else float('nan'):.4f}", flush=True)
    t1.record()
    torch.cuda.synchronize(env.device)
    secs = t0.elapsed_time(t1) / 1e3
    if checkpoint:
        _save_checkpoint(checkpoint, agent, mode="train_hive", preset=preset, hive_robots=list(members))
    n_valid = int(valid_rows.item())
    res = dict(mode="train_hive", preset=preset, dtype=dtype, num_envs=num_envs, steps=steps, hive_robots=list(members), opponents=opponents,
               env_steps_per_sec=(int(real_rows) if step_budget_clocks else num_envs * steps) / secs, seconds=secs,
               ms_per_vector_step=1e3 * secs / max(steps, 1), step_budget_clocks=step_budget_clocks, stepped_rows=int(real_rows) if step_budget_clocks else num_envs * steps,
               not_ready_share=int(parked_rows) / max(num_envs * steps, 1),
               transitions=int(agent.mem_cntr) if learn else 0, valid_rows=n_valid, valid_share=n_valid / max(rows * steps, 1),
               epsilon=agent.epsilon, mean_robot_reward=float(reward_sum.item()) / max(n_valid, 1), learn_calls=agent.updates,
               updates_per_step=updates_per_step if learn else 0, batch_size=B, replay_transitions=agent.mem_size,
               loss=float(agent.last_loss) if agent.last_loss is not None else None, fused_learn_step=bool(agent.fused),
               resumed_from=resume)
    hive.close()
    agent.close()
    env.close()
    if out:
        _write_result(out, res)
    return res


def train_pixels(num_envs=4096, steps=300, stack=4, span=400.0, mem_size=65536, device="cuda:0", seed=0, checkpoint=None, resume=None,
                 log_every=50, learn=True, updates_per_step=1, batch_size=256, dtype="f64", eps_dec=.999997, eps_end=0.2,
                 target_sync_vector_steps=64, out=None, step_budget_clocks=0, fused=None, replay="dense"):
    """train()'s loop on pixels: preset T seen through PixelObservation(env, robots=0, size=64, stack=stack, span=span), the agent a
    PixelDQNAgent.  Per vector step, serial on one stream: choose_action (rr_cnn_act: one launch for every arena) -> env.step + the new
    frames -> store_transition of the rows that were transitions (not re-placements, as in train()) -> updates_per_step x learn()
    (PyTorch autograd).  Returns train()'s result dict (+ stack, span, fused_act, loss).
    The replay ring holds both observations of a transition as uint8 frames: 2 * 3 * stack * 4096 bytes = 96 KB per transition at
    stack 4, 6.4 GB at the default mem_size of 65,536 (24 KB and 1.6 GB at stack 1).  The observation before the step is copied once per
    step (PixelObservation overwrites its buffer): num_envs * 48 KB at stack 4.
    replay="frames": the FrameReplay instead (PixelDQNAgent) -- every frame stored once, 12,298 bytes per transition, slots =
    ceil(mem_size / num_envs) + stack so that mem_size keeps meaning "transitions held"; a vector step is one rr_frames_push of the new
    frames (no copy of the observation before the step, no compaction, no host read) and learn() draws with rr_frames_sample.  The
    result also names replay, replay_bytes_per_transition and replay_capacity.
    The budgeted step is not wired to pixels: step_budget_clocks != 0 is refused."""
    import roborugby_amd as rr
    from .pixels import PixelObservation
    if step_budget_clocks:
        raise ValueError("train_pixels: the budgeted step (step_budget_clocks) is not supported on pixel observations; use 0")
    if not 1 <= int(stack) <= 4:
        raise ValueError("train_pixels: stack in 1..4 (the network takes 3, 6, 9 or 12 channels)")
    env = rr.make("RoboRugbySimpleDuel-v3", num_envs=num_envs, preset="T", device=device, seed=seed, dtype=dtype)
    B = int(batch_size)
    if replay not in ("dense", "frames"):
        raise ValueError("train_pixels(replay=...): 'dense' or 'frames'")
    frames = replay == "frames"
    agent = PixelDQNAgent(channels=3 * int(stack), batch_size=B, n_actions=env.action_space.n, device=device, seed=seed,
                          max_mem_size=mem_size, target_update_freq=max(100000, target_sync_vector_steps * num_envs),
                          eps_dec=eps_dec, eps_end=eps_end, fused=fused, replay=replay, replay_rows=num_envs if frames else None,
                          replay_slots=-(-int(mem_size) // num_envs) + int(stack) if frames else None)
    view = PixelObservation(env, robots=0, size=64, stack=int(stack), span=span)
    if resume:
        ck = torch.load(resume, map_location=device)
        agent.load_state_dict(ck["agent"])
        env.load_checkpoint_state(ck)
        pixels = view.restart()  # the frames are not checkpointed: every stack starts over from the restored state
    else:
        pixels = view.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    score_sum = torch.zeros(num_envs, device=device)
    real_rows = torch.zeros((), dtype=torch.int64, device=device)
    if frames and learn:
        agent.store_step(pixels)  # the observation every first transition starts from
    if not frames:
        before = torch.empty_like(pixels)
    for i in range(steps):
        action = agent.choose_action(pixels)
        if not frames:
            before.copy_(pixels)
        pixels, reward, done, info = view.step(action.view(-1, 1))
        real = (info.status & (STATUS_WAS_RESET | STATUS_NOT_READY)) == 0  # a call that only re-placed the arena is not a transition
        score_sum += reward
        real_rows += real.sum()
        if learn:
            if frames:
                agent.store_step(pixels, action, reward, done, real, first=(info.status & STATUS_WAS_RESET) != 0)
            else:
                agent.store_transition(before, action, reward, pixels, done, valid=real)
            for _ in range(updates_per_step):
                agent.learn()
        if log_every and (i + 1) % log_every == 0:
            _log_progress(i + 1, agent, env)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if checkpoint:
        _save_checkpoint(checkpoint, agent, **env.checkpoint_state())
    res = _train_result(agent, env, num_envs * steps, dt, steps, int(real_rows.item()), 0, updates_per_step if learn else 0, num_envs, False,
                        eps_dec, eps_end, False, float(score_sum.mean() / max(steps, 1)), "T", dtype, [])
    res.update(stack=int(stack), span=float(span), fused_act=bool(agent.fused),
               loss=float(agent.last_loss) if agent.last_loss is not None else None, replay=replay,
               replay_bytes_per_transition=agent.replay.bytes_per_transition if frames else 2 * agent.channels * 4096 + 13,
               replay_capacity=agent.mem_size)
    agent.close()
    env.close()
    if out:
        _write_result(out, res)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--preset", default=None, help="T (default), or any preset name; --train-hive / --play-hive: G")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--no-learn", action="store_true")
    ap.add_argument("--updates-per-step", type=int, default=4)
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--eps-dec", type=float, default=.999997)
    ap.add_argument("--eval-every", type=int, default=0)
    ap.add_argument("--eval-envs", type=int, default=16384)
    ap.add_argument("--log-every", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-overlap", action="store_true", help="gradient steps after the simulator's step instead of next to it")
    ap.add_argument("--no-fused", action="store_true", help="learn step through PyTorch autograd + torch.optim.Adam instead of rr_dqn_update")
    ap.add_argument("--budget", type=int, default=0, help="step_budget_clocks of the env (the budgeted step; 0 = synchronous)")
    ap.add_argument("--play-hive", default=None, metavar="CHECKPOINT",
                    help="no training: the checkpoint's policy plays preset G as the happy team's hive mind against OG_Twitchy (--num-envs, --steps)")
    ap.add_argument("--record", default=None, metavar="GIF",
                    help="--play-hive: an animated GIF of the first 16 arenas (a contact sheet of 96-pixel frames per step), rendered on the device")
    ap.add_argument("--record-view", default="field", choices=["field", "ego"],
                    help="--record: the whole field of each arena, or what its first hive robot sees (robot in the centre, front up)")
    ap.add_argument("--train-hive", action="store_true",
                    help="train the hive mind in the full game (preset G): one transition per hive robot and step; --resume takes the agent of "
                         "any checkpoint, e.g. one trained in preset T (--num-envs, --steps, --checkpoint, --updates-per-step, --batch-size)")
    ap.add_argument("--train-pixels", action="store_true",
                    help="train the convolutional agent on preset T's egocentric 64 x 64 frames (PixelObservation); acting is rr_cnn_act "
                         "(--num-envs, default 4096 here; --steps, --checkpoint, --resume, --updates-per-step, --batch-size, --pixel-stack)")
    ap.add_argument("--pixel-stack", type=int, default=4, help="--train-pixels: frames per observation (1..4; 3 channels each)")
    ap.add_argument("--pixel-replay", default="dense", choices=["dense", "frames"],
                    help="--train-pixels: the replay -- dense (both stacked observations of every transition) or frames (FrameReplay: every "
                         "frame once, rr_frames_push / rr_frames_sample)")
    a = ap.parse_args()
    if a.train_pixels:
        envs = a.num_envs if a.num_envs != ap.get_default("num_envs") else 4096  # (an observation is 48 KB at stack 4, not 44 bytes)
        res = train_pixels(envs, a.steps, a.pixel_stack, device=a.device, seed=a.seed, checkpoint=a.checkpoint, resume=a.resume,
                           log_every=a.log_every, learn=not a.no_learn, updates_per_step=a.updates_per_step, batch_size=a.batch_size or 256,
                           eps_dec=a.eps_dec, out=a.out, step_budget_clocks=a.budget, fused=False if a.no_fused else None,
                           replay=a.pixel_replay)
        print(json.dumps({k: v for k, v in res.items() if k != "curve"}))
        return
    if a.play_hive:
        print(json.dumps(play_hive(a.play_hive, a.num_envs, a.steps, a.device, a.seed, preset=a.preset or "G", step_budget_clocks=a.budget,
                                   record=a.record, record_view=a.record_view)))
        return
    if a.train_hive:
        print(json.dumps(train_hive(a.num_envs, a.steps, a.preset or "G", resume=a.resume, checkpoint=a.checkpoint,
                                    updates_per_step=a.updates_per_step, device=a.device, seed=a.seed, batch_size=a.batch_size,
                                    eps_dec=a.eps_dec, learn=not a.no_learn, log_every=a.log_every, out=a.out, step_budget_clocks=a.budget)))
        return
    res = train(a.num_envs, a.steps, a.preset or "T", a.device, a.seed, a.checkpoint, a.resume, learn=not a.no_learn,
                updates_per_step=a.updates_per_step, batch_size=a.batch_size, eps_dec=a.eps_dec, eval_every=a.eval_every,
                eval_envs=a.eval_envs, log_every=a.log_every, out=a.out, overlap_learn=not a.no_overlap,
                step_budget_clocks=a.budget, fused=False if a.no_fused else None)
    print(json.dumps({k: v for k, v in res.items() if k != "curve"}))


if __name__ == "__main__":
    main()
