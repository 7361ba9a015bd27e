"""Batched SAC trainer: the vectorised counterpart of the reference's Training_SAC_pytorch.py on the thrust entry
(BatchedRoboRugbyEnv(action_mode="thrust"): Box(-1, 1, (2 * nr_happy,)), rr_step_thrust).

Same agent as the reference: ActorNetwork (:157-240: Linear 11 -> 256 -> 256 -> (mu, sigma), sigma clamped to [1e-6, 1], tanh squash),
two CriticNetworks (:56-108, 11 + A inputs), a ValueNetwork and its soft-updated target (:111-154), Agent (:243-388: lr 1e-4, gamma .99,
tau .005, reward_scale 2, learn order value -> actor -> critics) -- but observations, replay and networks stay on the MI355X and one
call handles all N arenas.

Acting -- every row, every vector step -- is rr_sac_act where it applies (one HIP kernel: the hidden layers on the fp32 matrix cores, the
draw, the squash; csrc/rr_sac.hip); anything else, and fused=False, goes through the torch modules.  Learning is PyTorch autograd on the
same parameters (five small MLPs); with fused_targets=True its no-grad half -- the replay gathers, the policy sample, both critics on it and
the target value net: value_target and q_hat -- is rr_sac_targets, one HIP kernel, and autograd keeps the backward passes; with
fused_grads=True the value net's and both critics' gradients come from rr_sac_grads (one fused kernel and its reduce), and autograd keeps
the actor's backward alone.  No convergence claim is made for this trainer.

    python -m roborugby_amd.sac --num-envs 65536 --steps 300 --preset T --checkpoint runs/sac_T.pt [--fused-targets] [--fused-grads]
"""
import argparse
import copy
import json
import math
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .env import STATUS_NOT_READY, STATUS_WAS_RESET

HALF_LOG_TWO_PI = 0.5 * math.log(2.0 * math.pi)


def _mlp(n_in, fc1_dims, fc2_dims):
    return nn.Linear(n_in, fc1_dims), nn.Linear(fc1_dims, fc2_dims)


class CriticNetwork(nn.Module):
    """Q(s, a) (Training_SAC_pytorch.py:56-102)"""

    def __init__(self, input_dims, n_actions, fc1_dims=256, fc2_dims=256):
        super().__init__()
        self.fc1, self.fc2 = _mlp(input_dims + n_actions, fc1_dims, fc2_dims)
        self.q = nn.Linear(fc2_dims, 1)

    def forward(self, state, action):
        x = F.relu(self.fc1(torch.cat([state, action], dim=1)))
        return self.q(F.relu(self.fc2(x)))


class ValueNetwork(nn.Module):
    """V(s) (Training_SAC_pytorch.py:111-148)"""

    def __init__(self, input_dims, fc1_dims=256, fc2_dims=256):
        super().__init__()
        self.fc1, self.fc2 = _mlp(input_dims, fc1_dims, fc2_dims)
        self.v = nn.Linear(fc2_dims, 1)

    def forward(self, state):
        return self.v(F.relu(self.fc2(F.relu(self.fc1(state)))))


class ActorNetwork(nn.Module):
    """The policy (Training_SAC_pytorch.py:157-234).  parameters() come in rr_sac_act's order: fc1, fc2, mu, sigma (weight, bias each)."""
    reparam_noise = 1e-6

    def __init__(self, input_dims, max_action, n_actions=2, fc1_dims=256, fc2_dims=256):
        super().__init__()
        self.max_action, self.n_actions = float(max_action), int(n_actions)
        self.fc1, self.fc2 = _mlp(input_dims, fc1_dims, fc2_dims)
        self.mu = nn.Linear(fc2_dims, n_actions)
        self.sigma = nn.Linear(fc2_dims, n_actions)

    def head(self, state):
        """(mu, the raw sigma outputs before the clamp)"""
        x = F.relu(self.fc2(F.relu(self.fc1(state))))
        return self.mu(x), self.sigma(x)

    def forward(self, state):
        mu, raw = self.head(state)
        return mu, torch.clamp(raw, min=self.reparam_noise, max=1.0)

    def sample_normal(self, state, noise, reparameterize=True):
        """sample_normal (:207-234) with the standard normal draws given: x = mu + sigma * noise (detached unless reparameterize: Normal's
        sample() against rsample()), action = max_action * tanh(x), log_prob = sum_k Normal(mu, sigma).log_prob(x) - log(1 - action^2 + 1e-6)
        -> (action [n, A], log_prob [n])"""
        mu, sigma = self.forward(state)
        x = mu + sigma * noise
        zeta = noise  # (x - mu) / sigma: the draw itself, a constant under rsample()
        if not reparameterize:
            # a constant x: (x - mu) / sigma written around the draw, so that the value stays z where x - mu would cancel (sigma = 1e-6)
            x = x.detach()
            zeta = (mu.detach() - mu + sigma.detach() * noise) / sigma
        action = torch.tanh(x) * self.max_action
        log_probs = -0.5 * zeta ** 2 - torch.log(sigma) - HALF_LOG_TWO_PI
        log_probs = log_probs - torch.log(1 - action.pow(2) + self.reparam_noise)
        return action, log_probs.sum(1)


class BatchedSACAgent:
    """Agent (Training_SAC_pytorch.py:243-388) with [N]-batched choose_action / remember and a device replay.
    fused: None = rr_sac_act whenever it applies (a GPU, the 11-256-256 actor, n_actions 2 or 4); False = the torch path always.
    fused_targets: True = learn() takes value_target and q_hat from rr_sac_targets (one launch on the rings; the value target's noise is
    then the kernel's draw under (seed, learn call) instead of a torch.randn from the agent's generator); needs what fused=True needs and
    batch_size % 64 == 0.  Default False.
    fused_grads: True = the learn step takes the gradients of the value loss and the critic loss from rr_sac_grads (no autograd for the
    value net and the critics; the actor loss and its backward stay autograd); needs what fused_targets needs, works with fused_targets
    on or off.  Default False.
    The replay is a ring on the device with float actions [M, A], written with torch indexing for the rows whose `valid` is set."""

    def __init__(self, alpha=1e-4, beta=1e-4, input_dims=11, n_actions=2, max_action=1.0, gamma=.99, max_mem_size=1 << 20, tau=.005,
                 fc1_dims=256, fc2_dims=256, batch_size=4096, reward_scale=2.0, device="cpu", seed=0, fused=None, fused_targets=False,
                 fused_grads=False):
        self.gamma, self.tau, self.scale = gamma, tau, reward_scale
        self.n_actions, self.input_dims, self.max_action = int(n_actions), int(input_dims), float(max_action)
        self.mem_size, self.batch_size = int(max_mem_size), int(batch_size)
        self.device = torch.device(device)
        self.mem_cntr, self.updates, self.last_losses = 0, 0, None
        self._act_calls = 0  # fused choose_action calls so far: keys the kernel's draws (checkpointed)
        self._learn_calls = 0  # learn() calls through rr_sac_targets so far: keys that kernel's draws (checkpointed)
        self._seed = int(seed)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)
        torch.manual_seed(seed)
        d = self.device
        self.actor = ActorNetwork(input_dims, max_action, n_actions, fc1_dims, fc2_dims).to(d)
        self.critic_1 = CriticNetwork(input_dims, n_actions, fc1_dims, fc2_dims).to(d)
        self.critic_2 = CriticNetwork(input_dims, n_actions, fc1_dims, fc2_dims).to(d)
        self.value = ValueNetwork(input_dims, fc1_dims, fc2_dims).to(d)
        self.target_value = copy.deepcopy(self.value)  # update_network_parameters(tau=1), :279
        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr=alpha)
        self.value_optimizer = torch.optim.Adam(self.value.parameters(), lr=beta)
        self.critic_optimizer = torch.optim.Adam(list(self.critic_1.parameters()) + list(self.critic_2.parameters()), lr=beta)
        m = self.mem_size
        self.state_memory = torch.zeros(m, input_dims, device=d)
        self.new_state_memory = torch.zeros(m, input_dims, device=d)
        self.action_memory = torch.zeros(m, n_actions, device=d)
        self.reward_memory = torch.zeros(m, device=d)
        self.terminal_memory = torch.zeros(m, dtype=torch.bool, device=d)
        can_fuse = d.type == "cuda" and (input_dims, fc1_dims, fc2_dims) == (11, 256, 256) and self.n_actions in (2, 4)
        # default: on whenever it applies -- the kernel is faster than the torch path at 4,096 and at 65,536 rows (profiles/sac_act/)
        self.fused = can_fuse if fused is None else bool(fused)
        if self.fused and not can_fuse:
            raise ValueError("fused=True needs a GPU, the reference's 11-256-256 actor and 2 or 4 actions")
        self.fused_targets = bool(fused_targets)
        if self.fused_targets and not (can_fuse and self.batch_size > 0 and self.batch_size % 64 == 0):
            raise ValueError("fused_targets=True needs a GPU, the reference's 11-256-256 networks, 2 or 4 actions and a batch_size that is a "
                             "positive multiple of 64")
        self.fused_grads = bool(fused_grads)
        if self.fused_grads and not (can_fuse and self.batch_size > 0 and self.batch_size % 64 == 0):
            raise ValueError("fused_grads=True needs a GPU, the reference's 11-256-256 networks, 2 or 4 actions and a batch_size that is a "
                             "positive multiple of 64")
        self._dqn = _lib.DqnHandle(d) if self.fused or self.fused_targets or self.fused_grads else None
        self._grad_bufs = None  # rr_sac_grads' outputs: one tensor per parameter of value, critic_1, critic_2, and loss [3] (first use)

    # what dqn._train_result reads of an agent: SAC has no epsilon schedule, and its target follows every learn() (soft update)
    epsilon, target_update_freq = 0.0, 0
    target_syncs = property(lambda self: self.updates)

    def close(self):
        if getattr(self, "_dqn", None):
            self._dqn.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @torch.no_grad()
    def choose_action(self, observation, deterministic=False):
        """[n, 11] -> float32 [n, A]: a squashed sample of the policy per row (:281-285), or max_action * tanh(mu) with deterministic."""
        n = observation.shape[0]
        if (self.fused and n > 0 and n % 64 == 0 and observation.dtype == torch.float32 and observation.dim() == 2
                and observation.shape[1] == 11 and observation.is_contiguous() and observation.device == self.actor.mu.weight.device):
            return self._act_fused(observation, deterministic)
        return self._act_torch(observation, deterministic)

    @torch.no_grad()
    def _act_torch(self, observation, deterministic=False):
        """the torch path of choose_action: the modules' forward, torch.randn from the agent's generator, the squash"""
        mu, sigma = self.actor(observation.float())
        if deterministic:
            return torch.tanh(mu) * self.max_action
        noise = torch.randn(mu.shape, generator=self.gen, device=self.device)
        return torch.tanh(mu + sigma * noise) * self.max_action

    def _act_fused(self, obs, deterministic=False, log_prob=None, head=None, noise=None):
        n = obs.shape[0]
        out = torch.empty(n, self.n_actions, dtype=torch.float32, device=self.device)
        params = list(self.actor.parameters())
        assert all(p.is_contiguous() and p.dtype == torch.float32 for p in params)
        self._act_calls += 1
        self._dqn.sac_act(params, obs, n, self.n_actions, self.max_action, self._seed, self._act_calls, out, deterministic, log_prob, head, noise)
        return out

    @torch.no_grad()
    def remember(self, state, action, reward, state_, done, valid=None):
        """Appends the rows with valid=True (None: all) to the ring, in row order (ReplayBuffer.store_transition, :29-38)"""
        reward, done = reward.reshape(-1), done.reshape(-1)
        if valid is not None:
            idx = valid.reshape(-1).nonzero(as_tuple=True)[0]
            state, action, reward, state_, done = state[idx], action[idx], reward[idx], state_[idx], done[idx]
        n = state.shape[0]
        if n == 0:
            return
        if n > self.mem_size:
            raise ValueError(f"{n} transitions in one call do not fit a replay ring of {self.mem_size}")
        pos = (self.mem_cntr + torch.arange(n, device=self.device)) % self.mem_size
        self.state_memory[pos] = state.float()
        self.new_state_memory[pos] = state_.float()
        self.action_memory[pos] = action.float().view(n, self.n_actions)
        self.reward_memory[pos] = reward.float()
        self.terminal_memory[pos] = done.bool()
        self.mem_cntr += n

    def losses(self, batch, noise_value, noise_actor):
        """(value_loss, actor_loss, critic_loss) of Agent.learn (:344-383) on batch = (state, action, reward, new_state, done), a function
        of the batch and the two standard normal tensors [B, A]: noise_value of the non-reparameterised sample behind the value target,
        noise_actor of the reparameterised one behind the actor loss.  The composition of targets() and losses_given_targets()."""
        value_target, q_hat = self.targets(batch, noise_value)
        return self.losses_given_targets(batch[0], batch[1], value_target, q_hat, noise_actor)

    @torch.no_grad()
    def targets(self, batch, noise_value):
        """The no-grad half of losses(), the torch path: (value_target, q_hat) [B] each.  value_target = min(Q1, Q2)(s, a~) - log pi(a~ | s)
        with a~ the non-reparameterised sample under noise_value, q_hat = reward_scale r + gamma (done ? 0 : V_target(s'))."""
        state, _, reward, state_, done = batch
        value_ = self.target_value(state_).view(-1).masked_fill(done, 0.0)
        # (the reference leaves this target attached and zeroes what it sends into the actor and the critics before they are used)
        actions, log_probs = self.actor.sample_normal(state, noise_value, reparameterize=False)
        value_target = torch.min(self.critic_1(state, actions), self.critic_2(state, actions)).view(-1) - log_probs
        q_hat = self.scale * reward + self.gamma * value_
        return value_target, q_hat

    def targets_fused(self, batch_index, noise_value=None, mem_rows=None, **windows):
        """targets() of the ring rows batch_index (int64 [B], B a multiple of 64) through rr_sac_targets: (value_target, q_hat, state,
        action) with state / action the gathered rows.  noise_value None: the kernel draws under (seed, _learn_calls); windows: tensors
        for the kernel's optional outputs (policy_action, log_prob, head, noise_out, q1, q2, v_next)."""
        if self._dqn is None:
            raise ValueError("targets_fused needs an agent built with fused or fused_targets on a GPU")
        B, d = int(batch_index.shape[0]), self.device
        assert batch_index.dtype == torch.int64 and batch_index.is_contiguous() and batch_index.device == self.state_memory.device
        assert noise_value is None or (noise_value.dtype == torch.float32 and noise_value.is_contiguous() and tuple(noise_value.shape) == (B, self.n_actions))
        nets = [list(n.parameters()) for n in (self.actor, self.critic_1, self.critic_2, self.target_value)]
        assert all(p.is_contiguous() and p.dtype == torch.float32 for n in nets for p in n)
        value_target, q_hat = torch.empty(B, device=d), torch.empty(B, device=d)
        state, action = torch.empty(B, self.input_dims, device=d), torch.empty(B, self.n_actions, device=d)
        rings = (self.state_memory, self.new_state_memory, self.action_memory, self.reward_memory, self.terminal_memory)
        self._dqn.sac_targets(*nets, rings, min(self.mem_cntr, self.mem_size) if mem_rows is None else mem_rows, B, self.n_actions,
                              self.max_action, self.gamma, self.scale, value_target, q_hat, batch_index=batch_index, noise=noise_value,
                              seed=self._seed, calls=self._learn_calls, state=state, action=action, **windows)
        return value_target, q_hat, state, action

    def actor_loss(self, state, noise_actor):
        """mean(log pi(a | s) - min(Q1, Q2)(s, a)) with a the reparameterised sample under noise_actor (:357-366)"""
        actions, log_probs = self.actor.sample_normal(state, noise_actor, reparameterize=True)
        critic_value = torch.min(self.critic_1(state, actions), self.critic_2(state, actions)).view(-1)
        return torch.mean(log_probs - critic_value)

    def losses_given_targets(self, state, action, value_target, q_hat, noise_actor):
        """The autograd half of losses(): (value_loss, actor_loss, critic_loss) from the batch's states and actions, the two target
        vectors [B] (constants) and the standard normal tensor [B, A] of the reparameterised sample behind the actor loss."""
        value = self.value(state).view(-1)
        value_loss = 0.5 * F.mse_loss(value, value_target)
        actor_loss = self.actor_loss(state, noise_actor)
        critic_loss = 0.5 * F.mse_loss(self.critic_1(state, action).view(-1), q_hat) + 0.5 * F.mse_loss(self.critic_2(state, action).view(-1), q_hat)
        return value_loss, actor_loss, critic_loss

    @torch.no_grad()
    def grads_fused(self, state, action, value_target, q_hat):
        """The gradients of losses_given_targets()' value_loss and critic_loss through rr_sac_grads (no autograd): state [B, 11], action
        [B, A], value_target, q_hat [B], dense float32 on the agent's device, B a multiple of 64 -> ((value, critic_1, critic_2): per
        net one gradient tensor per parameter, in parameters() order), loss [3] = 0.5 * mse of value, critic_1, critic_2: value_loss =
        loss[0], critic_loss = loss[1] + loss[2]).  The tensors are the agent's own buffers: the next call overwrites them."""
        if self._dqn is None:
            raise ValueError("grads_fused needs an agent built with fused, fused_targets or fused_grads on a GPU")
        B, A = int(state.shape[0]), self.n_actions
        nets = [list(n.parameters()) for n in (self.value, self.critic_1, self.critic_2)]
        assert all(p.is_contiguous() and p.dtype == torch.float32 for n in nets for p in n)
        for t, shape in ((state, (B, self.input_dims)), (action, (B, A)), (value_target, (B,)), (q_hat, (B,))):
            assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape and t.device == nets[0][0].device
        if self._grad_bufs is None:
            self._grad_bufs = ([[torch.empty_like(p) for p in n] for n in nets], torch.empty(3, device=self.device))
        grads, loss = self._grad_bufs
        self._dqn.sac_grads(*nets, state, action, value_target, q_hat, B, A, *grads, loss)
        return tuple(grads), loss

    @torch.no_grad()
    def update_network_parameters(self, tau=None):
        """target_value <- tau * value + (1 - tau) * target_value (:290-304)"""
        tau = self.tau if tau is None else tau
        for pt, pv in zip(self.target_value.parameters(), self.value.parameters()):
            pt.mul_(1.0 - tau).add_(pv, alpha=tau)

    def learn(self):
        """One Agent.learn (:322-388): a batch drawn with replacement, the value, actor and critic steps in that order, the soft update.
        Each loss only steps its own network(s), and none depends on what an earlier step of the same call changed (the actor loss not on
        the value net, the critic loss on neither), so the three are computed on one forward and stepped in the reference's order.
        Returns the three losses (device scalars), None until the replay holds a batch.
        The draws are made here -- the batch rows, then the value target's noise, then the actor loss's -- and learn_on does the rest.
        With fused_targets: the batch rows as above, then ONE rr_sac_targets launch on the rings (gathers, the value target's noise drawn
        in the kernel under (seed, _learn_calls), value_target, q_hat), then the actor loss's noise from the generator, the autograd
        half on the kernel's gathered rows, the same three steps and soft update."""
        if self.mem_cntr < self.batch_size:
            return None
        max_mem = min(self.mem_cntr, self.mem_size)
        idx = torch.randint(0, max_mem, (self.batch_size,), generator=self.gen, device=self.device)
        if self.fused_targets:
            self._learn_calls += 1
            value_target, q_hat, state, action = self.targets_fused(idx, mem_rows=max_mem)
            noise_actor = torch.randn((self.batch_size, self.n_actions), generator=self.gen, device=self.device)
            return self._learn_given_targets(state, action, value_target, q_hat, noise_actor)
        batch = (self.state_memory[idx], self.action_memory[idx], self.reward_memory[idx], self.new_state_memory[idx], self.terminal_memory[idx])
        shape = (self.batch_size, self.n_actions)
        noise_value = torch.randn(shape, generator=self.gen, device=self.device)
        noise_actor = torch.randn(shape, generator=self.gen, device=self.device)
        return self.learn_on(batch, noise_value, noise_actor)

    def learn_on(self, batch, noise_value, noise_actor):
        """learn() after its draws, a function of the agent's state and its arguments alone: the losses of batch = (state, action, reward,
        new_state, done) under the two standard normal tensors [B, A], the value, actor and critic steps, the soft update, the counters."""
        value_target, q_hat = self.targets(batch, noise_value)
        return self._learn_given_targets(batch[0], batch[1], value_target, q_hat, noise_actor)

    def _learn_given_targets(self, state, action, value_target, q_hat, noise_actor):
        """learn() after its targets: autograd of the three losses, or (fused_grads) of the actor loss alone next to rr_sac_grads"""
        if self.fused_grads:
            return self._step_fused_grads(state.contiguous(), action.contiguous(), value_target, q_hat, noise_actor)
        return self._step(self.losses_given_targets(state, action, value_target, q_hat, noise_actor))

    def _step_fused_grads(self, state, action, value_target, q_hat, noise_actor):
        """_step() with fused_grads: the actor loss and its backward by autograd (inputs = the actor's parameters), the value net's and the
        critics' gradients from ONE rr_sac_grads call into the agent's per-parameter buffers, installed as .grad; then the same three
        steps in the reference's order, the soft update, the counters.  last_losses = (loss[0], actor_loss, loss[1] + loss[2])."""
        actor_loss = self.actor_loss(state, noise_actor)
        for opt in (self.value_optimizer, self.actor_optimizer, self.critic_optimizer):
            opt.zero_grad(set_to_none=True)
        actor_loss.backward(inputs=list(self.actor.parameters()))
        grads, loss = self.grads_fused(state, action, value_target, q_hat)
        for net, gs in zip((self.value, self.critic_1, self.critic_2), grads):
            for p, g in zip(net.parameters(), gs):
                p.grad = g
        for opt in (self.value_optimizer, self.actor_optimizer, self.critic_optimizer):
            opt.step()
        self.update_network_parameters()
        self.updates += 1
        self.last_losses = (loss[0].clone(), actor_loss.detach(), loss[1] + loss[2])
        return self.last_losses

    def _step(self, losses):
        """the value, actor and critic steps on their losses, the soft update, the counters"""
        value_loss, actor_loss, critic_loss = losses
        for loss, opt in ((value_loss, self.value_optimizer), (actor_loss, self.actor_optimizer), (critic_loss, self.critic_optimizer)):
            opt.zero_grad(set_to_none=True)
            loss.backward(inputs=[p for g in opt.param_groups for p in g["params"]])
        for opt in (self.value_optimizer, self.actor_optimizer, self.critic_optimizer):
            opt.step()
        self.update_network_parameters()
        self.updates += 1
        self.last_losses = (value_loss.detach(), actor_loss.detach(), critic_loss.detach())
        return self.last_losses

    # whole-agent checkpoint, without the replay (as the DQN agents')
    _NETS = ("actor", "critic_1", "critic_2", "value", "target_value")
    _OPTS = ("actor_optimizer", "value_optimizer", "critic_optimizer")

    def state_dict(self):
        sd = {k: getattr(self, k).state_dict() for k in self._NETS + self._OPTS}
        sd.update(kind="sac", n_actions=self.n_actions, mem_cntr=self.mem_cntr, updates=self.updates, act_calls=self._act_calls, fused=self.fused,
                  learn_calls=self._learn_calls)
        return sd

    def load_state_dict(self, sd):
        if sd.get("kind") != "sac" or int(sd["n_actions"]) != self.n_actions:
            raise ValueError(f"not a checkpoint of a SAC agent with {self.n_actions} actions")
        for k in self._NETS + self._OPTS:
            getattr(self, k).load_state_dict(sd[k])
        self._act_calls = int(sd.get("act_calls", 0))
        self._learn_calls = int(sd.get("learn_calls", 0))
        self.updates = int(sd.get("updates", 0))  # (the replay is not checkpointed: mem_cntr restarts at what this process has stored)


def train_sac(num_envs=65536, steps=300, preset="T", device="cuda:0", seed=0, checkpoint=None, resume=None, log_every=50, learn=True,
              mem_size=1 << 20, dtype="f64", updates_per_step=1, batch_size=4096, out=None, step_budget_clocks=0, fused=None,
              fused_targets=False, fused_grads=False):
    """The main loop of Training_SAC_pytorch.py over a batched env with action_mode="thrust": per vector step, serial on one stream,
    choose_action (rr_sac_act: one launch for every arena) -> env.step_thrust (the agent drives the happy team: A = 2 * nr_happy
    columns) -> remember the rows that were transitions (a row whose status has WAS_RESET was only re-placed and ends none) ->
    updates_per_step x learn() (fused_targets: its no-grad half through rr_sac_targets; fused_grads: the value net's and the critics'
    gradients through rr_sac_grads).  Returns dqn.train()'s result dict (+ n_actions, fused_act, fused_targets, fused_grads, mem_cntr, act_calls and the three losses).
    The budgeted step is not wired to this trainer: step_budget_clocks != 0 is refused."""
    import roborugby_amd as rr
    from .dqn import _save_checkpoint, _train_result, _write_result
    if step_budget_clocks:
        raise ValueError("train_sac: the budgeted step (step_budget_clocks) is not supported; use 0")
    env = rr.BatchedRoboRugbyEnv(num_envs, preset=preset, device=device, seed=seed, dtype=dtype, action_mode="thrust")
    A = env.action_space.shape[0]
    agent = BatchedSACAgent(input_dims=env.observation_space.shape[0], n_actions=A, max_action=float(env.action_space.high.max()),
                            max_mem_size=mem_size, batch_size=batch_size, device=device, seed=seed, fused=fused,
                            fused_targets=fused_targets, fused_grads=fused_grads)
    if resume:
        ck = torch.load(resume, map_location=device)
        agent.load_state_dict(ck["agent"])
        env.load_checkpoint_state(ck)
        observation = env.get_game_state()
    else:
        observation = env.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    score_sum = torch.zeros(num_envs, device=device)
    real_rows = torch.zeros((), dtype=torch.int64, device=device)
    for i in range(steps):
        action = agent.choose_action(observation)
        observation_, reward, done, info = env.step_thrust(action)
        real = (info.status & (STATUS_WAS_RESET | STATUS_NOT_READY)) == 0
        score_sum += reward
        real_rows += real.sum()
        if learn:
            agent.remember(observation, action, reward, observation_, done, valid=real)
            for _ in range(updates_per_step):
                agent.learn()
        observation = observation_
        if log_every and (i + 1) % log_every == 0:
            torch.cuda.synchronize()
            ls = [float(x) for x in agent.last_losses] if agent.last_losses else [float("nan")] * 3
            print(f"step {i + 1} stored {agent.mem_cntr} updates {agent.updates} mean-step-reward {float(score_sum.mean()) / (i + 1):.4f} "
                  f"value-loss {ls[0]:.4f} actor-loss {ls[1]:.4f} critic-loss {ls[2]:.4f}", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if checkpoint:
        _save_checkpoint(checkpoint, agent, **env.checkpoint_state())
    res = _train_result(agent, env, num_envs * steps, dt, steps, int(real_rows.item()), 0, updates_per_step if learn else 0, num_envs, False,
                        0.0, 0.0, False, float(score_sum.mean() / max(steps, 1)), preset, dtype, [])
    ls = [float(x) for x in agent.last_losses] if agent.last_losses else [None] * 3
    res.update(mode="train_sac", n_actions=A, fused_act=bool(agent.fused), fused_targets=bool(agent.fused_targets), fused_grads=bool(agent.fused_grads),
               mem_cntr=agent.mem_cntr,
               act_calls=agent._act_calls,
               tau=agent.tau, reward_scale=agent.scale, value_loss=ls[0], actor_loss=ls[1], critic_loss=ls[2], resumed_from=resume)
    agent.close()
    env.close()
    if out:
        _write_result(out, res)
    return res


def main():
    ap = argparse.ArgumentParser(description="batched SAC on the thrust entry (Training_SAC_pytorch.py's counterpart)")
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--preset", default="T", help="T, G, D or any preset name: the agent drives the happy team's 2 * nr_happy engines")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--no-learn", action="store_true")
    ap.add_argument("--updates-per-step", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=4096)
    ap.add_argument("--log-every", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-fused", action="store_true", help="choose_action through the torch modules instead of rr_sac_act")
    ap.add_argument("--fused-targets", action="store_true",
                    help="learn()'s no-grad half (replay gathers, policy sample, critics, target value net) through rr_sac_targets")
    ap.add_argument("--fused-grads", action="store_true",
                    help="the value net's and the critics' gradients through rr_sac_grads (the actor's backward stays autograd)")
    a = ap.parse_args()
    res = train_sac(a.num_envs, a.steps, a.preset, a.device, a.seed, a.checkpoint, a.resume, a.log_every, not a.no_learn,
                    updates_per_step=a.updates_per_step, batch_size=a.batch_size, out=a.out, fused=False if a.no_fused else None,
                    fused_targets=a.fused_targets, fused_grads=a.fused_grads)
    print(json.dumps({k: v for k, v in res.items() if k != "curve"}))


if __name__ == "__main__":
    main()
