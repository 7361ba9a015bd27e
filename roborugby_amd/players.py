"""Scripted opponents as on-device batched policies.

`Hive` is the reference's hive-mind player (DQN_pytorch_player.py: Stephen): one trained DQN policy drives every robot of the hive.
`og_twitchy` is the reference's OG_Twitchy (robo_rugby/gym_env/RR_Players.py:14-30): per robot, 5 % turn left (-1, 1),
45 % straight (1, 1), 45 % back (-1, -1), 5 % turn right (1, -1) -- as (L, R) thrust pairs for `step_thrust`."""
import torch

from . import _lib
from ._lib import ptr

_TABLE = ((-1.0, 1.0), (1.0, 1.0), (-1.0, -1.0), (1.0, -1.0))


def og_twitchy(num_envs, num_robots, generator=None, device="cuda"):
    """float32 [num_envs, 2*num_robots] thrust pairs drawn like OG_Twitchy.get_action() for every robot."""
    u = torch.rand(num_envs, num_robots, generator=generator, device=device)
    idx = (u > 0.05).long() + (u > 0.5).long() + (u >= 0.95).long()  # <=.05 left, <=.5 straight, <.95 back, else right
    table = torch.tensor(_TABLE, dtype=torch.float32, device=device)
    return table[idx].reshape(num_envs, 2 * num_robots)


def chase(env, obs, step=0, noise=0.1, seed=0, na=None, step_of=None, out=None):
    """The scripted policy of the contact-rich benchmark stream: robot 0 of every arena turns toward its
    ball (or drives forward within 8 degrees), `noise` of the arenas act at random, the other robots act at random.  ONE kernel
    launch on the current stream (rr_policy_chase); the draws are a function of (seed, global arena id, step index) -- `step`,
    or per arena `step_of` (int32 [N]).  Returns int32 [N, na]."""
    na = env.preset.nr if na is None else int(na)
    if out is None:
        out = torch.empty(env.num_envs, na, dtype=torch.int32, device=env.device)
    obs = obs.contiguous()
    assert obs.dtype == torch.float32 and obs.shape == (env.num_envs, 11)
    env._handle.launch("rr_policy_chase", ptr(obs), ptr(step_of), int(step) & 0xFFFFFFFF, float(noise), int(seed), ptr(out), na)
    return out


# GameEnv_Simple._dct_thrust_from_direction (RR_EnvBase.py:593-602): Direction 0..7 -> (L, R)
_THRUST_FROM_DIRECTION = ((1.0, 1.0), (-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0), (0.0, 1.0), (1.0, 0.0), (-1.0, 0.0), (0.0, -1.0))


class Hive:
    """The reference's hive mind (DQN_pytorch_player.py:10-85, `Stephen`) for every arena at once: each step every hive robot is given
    a ball (greedy, nearest pair first, balls lying in a goal ignored), the ONE trained agent is asked for an action on
    get_game_state(obj_robot=robot, obj_ball=its ball) with epsilon 0.2, and the (L, R) thrust pairs go to `env.step_thrust`; a
    robot without a ball stands still (0, 0).

    act() is rr_hive_observe -> ONE rr_dqn_act over the N * NR rows (padded to a multiple of 64) -> table lookup, all on the current
    stream: no host synchronisation, and with `out` given no allocation.  On an env that has, or has had, a step budget
    (env.has_had_budget) act() holds the rows of arenas parked mid-step instead: rr_hive_observe_held -> rr_dqn_act into a scratch
    buffer -> rr_hive_commit, so `assign`, `obs` and `actions` of a parked arena stay those of the step it is in the middle of and
    transition() / store() hand out the transition of the step the arena ACCEPTED; `held` says which arenas those were.  `agent`: a roborugby_amd.dqn.BatchedDQNAgent (its Q_eval
    acts) or the six parameter tensors (fc1.weight, fc1.bias, fc2.weight, fc2.bias, fc3.weight, fc3.bias; float32, on the env's
    device).  `robots`: indices of the hive's robots, happy robots first (None: the happy team).  `observer`: what the agent was
    trained on -- None = the env's own when it is SingleBall_6wayLidar(_v2), else SingleBall_6wayLidar_v2 (what `dqn.train` uses;
    the reference's Stephen insists on 'SingleBall_6wayLidar').  The epsilon draws are a function of (seed, row, number of act()
    calls so far); a captured graph replays the draws of the call it captured."""

    def __init__(self, env, agent, robots=None, epsilon=0.2, seed=0, observer=None):
        self.env, self.epsilon, self.seed = env, float(epsilon), int(seed)
        nr, N = env.preset.nr, env.num_envs
        self.robots = tuple(range(env.preset.nr_happy)) if robots is None else tuple(sorted({int(r) for r in robots}))
        if not self.robots or self.robots[0] < 0 or self.robots[-1] >= nr:
            raise ValueError(f"robots: a non-empty subset of 0..{nr - 1}")
        self.mask, self.kind, _ = env._hive_args(sum(1 << r for r in self.robots), observer)
        if self.kind not in (0, 1):
            raise ValueError("observer: 'SingleBall_6wayLidar_v2' or 'SingleBall_6wayLidar'")
        params = list(agent.Q_eval.parameters()) if hasattr(agent, "Q_eval") else list(agent)
        shapes = [(256, 11), (256,), (256, 256), (256,), (8, 256), (8,)]
        if [tuple(p.shape) for p in params] != shapes or any(p.dtype != torch.float32 or p.device != env.device or not p.is_contiguous()
                                                              for p in params):
            raise ValueError("agent: the reference's 11-256-256-8 network (six contiguous float32 tensors on the env's device)")
        self._params = params  # (kept alive; the pointers are read at every act(): in-place updates of a learning agent are seen)
        self._dqn = getattr(agent, "_dqn", None)  # the rr_dqn handle (_lib.DqnHandle): a fused agent's is borrowed, never closed here
        self._owns = not (self._dqn and self._dqn.h)
        if self._owns:
            self._dqn = _lib.DqnHandle(env.device)
        self._agent = agent  # (kept alive: a borrowed rr_dqn handle is the agent's)
        self.rows = (N * nr + 63) // 64 * 64
        dev = env.device
        self._assign = torch.full((N, nr), -1, dtype=torch.int32, device=dev)  # (-1: an arena held from the very first act() has no row)
        self._obs = torch.zeros(self.rows, 11, dtype=torch.float32, device=dev)  # (the padding rows stay 0)
        self._actions = torch.zeros(self.rows, dtype=torch.int32, device=dev)
        self._thrust = torch.empty(N * nr, 2, dtype=torch.float32, device=dev)
        self._has = torch.empty(N, nr, dtype=torch.bool, device=dev)
        self._table = torch.tensor(_THRUST_FROM_DIRECTION, dtype=torch.float32, device=dev)
        self._held = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._fresh = None  # the agent's answers before rr_hive_commit accepts them (budgeted step only)
        self.calls = 0

    def close(self):
        if getattr(self, "_owns", False):
            self._dqn.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def _dqn_h(self):
        """the rr_dqn handle act() runs on (None: its owner has closed it)"""
        return self._dqn.h

    @property
    def assign(self):
        """int32 [N, NR]: the ball every robot was given in the last act() (-1: none / outside the hive)"""
        return self._assign

    @property
    def obs(self):
        """float32 [N, NR, 11]: the observations the agent was asked on in the last act()"""
        return self._obs[:self.env.num_envs * self.env.preset.nr].view(self.env.num_envs, self.env.preset.nr, 11)

    @property
    def actions(self):
        """int32 [N, NR]: the agent's answers of the last act() (meaningful where assign >= 0)"""
        return self._actions[:self.env.num_envs * self.env.preset.nr].view(self.env.num_envs, self.env.preset.nr)

    @property
    def held(self):
        """bool [N]: arenas that were parked mid-step at the last act() on a budgeted env -- their assign / obs / actions rows were held"""
        return self._held.view(torch.bool)

    def _dqn_act(self, actions, stream):
        self.calls += 1
        self._dqn.act(self._params, self._obs, self.rows, self.epsilon, self.seed, self.calls, actions, stream=stream)

    def _act_held(self, out, stream):
        """act() under the budgeted step: observe (held rows kept) -> the agent's fresh answers -> commit, on the current stream"""
        env = self.env
        if self._fresh is None:
            self._fresh = torch.zeros(self.rows, dtype=torch.int32, device=env.device)
        env.hive_observe(self.mask, _OBSERVER_OF_KIND[self.kind], out=(self._assign, self._obs, self._held), held=True)
        self._dqn_act(self._fresh, stream)  # (held arenas waste their draws)
        env.hive_commit(self._fresh, self._assign, self._held, self._actions, out, self.mask)
        return out

    @torch.no_grad()
    def act(self, out=None, status=None):
        """float32 [N, 2*NR] thrust pairs for env.step_thrust.  Columns of robots outside the hive are left as the caller filled them
        in `out` (0 in a fresh tensor), so another player -- `og_twitchy` -- can drive them.  status (optional, the last step's
        info.status): rows of arenas that are NOT_READY (budgeted step, parked mid-step) are left alone; the step ignores them.
        Without `status`, on an env that has (had) a step budget: the held pipeline (see the class)."""
        env = self.env
        N, nr = env.num_envs, env.preset.nr
        if out is None:
            out = torch.zeros(N, 2 * nr, dtype=torch.float32, device=env.device)
        assert out.dtype == torch.float32 and out.shape == (N, 2 * nr) and out.is_contiguous()
        stream = self._dqn.stream()
        if status is None and env.has_had_budget:
            return self._act_held(out, stream)
        # (the entry itself, not env.hive_observe: on the stream rr_dqn_act goes to, into buffers that are this object's own)
        env._handle.call("rr_hive_observe", self.mask, self.kind, ptr(self._assign), ptr(self._obs), stream)
        self._dqn_act(self._actions, stream)
        torch.index_select(self._table, 0, self._actions[:N * nr], out=self._thrust)
        torch.ge(self._assign, 0, out=self._has)
        thr = self._thrust.view(N, nr, 2)
        thr.mul_(self._has.unsqueeze(-1))  # a robot without a ball stands still
        out3 = out.view(N, nr, 2)
        if status is not None:
            from .env import STATUS_NOT_READY
            keep = ((status & STATUS_NOT_READY) != 0).view(N, 1)
            for r in self.robots:
                out3[:, r] = torch.where(keep, out3[:, r], thr[:, r])
        elif len(self.robots) == nr:
            out.copy_(self._thrust.view(N, 2 * nr))
        else:
            for r in self.robots:
                out3[:, r].copy_(thr[:, r])
        return out

    # ---- training the hive in the full game (dqn.train_hive): act() -> env.step_thrust -> store()
    @torch.no_grad()
    def transition(self, done, status):
        """The transition of every hive robot over the step taken since the last act(): ONE rr_hive_transition launch on the current
        stream with the assignment act() made, into persistent buffers, no host synchronisation.  done, status: the step's.
        -> (next_obs float32 [N,NR,11], reward float32 [N,NR], terminal bool [N,NR], valid bool [N,NR]); a row is valid when its robot
        had a ball, the arena really stepped and the ball is still in play -- next_obs is the robot's view of THAT ball after the step.
        The env must track the prior step (env.track_prior_step() before the step).  On an env that has (had) a step budget this is
        rr_hive_transition_held: a row of an arena whose step is still in progress is invalid, and the row of the call that completes
        it pairs with the obs / actions act() held for it."""
        env = self.env
        N, nr = env.num_envs, env.preset.nr
        if getattr(self, "_next_obs", None) is None:
            dev = env.device
            self._next_obs = torch.zeros(N * nr, 11, dtype=torch.float32, device=dev)
            self._reward = torch.zeros(N * nr, dtype=torch.float32, device=dev)
            self._terminal = torch.zeros(N * nr, dtype=torch.bool, device=dev)
            self._valid = torch.zeros(N * nr, dtype=torch.bool, device=dev)
        fn = env.hive_transition_held if env.has_had_budget else env.hive_transition
        fn(self._assign, status, done, robot_mask=self.mask, observer=_OBSERVER_OF_KIND[self.kind],
           out=(self._next_obs, self._reward, self._terminal, self._valid))
        return self._next_obs.view(N, nr, 11), self._reward.view(N, nr), self._terminal.view(N, nr), self._valid.view(N, nr)

    @torch.no_grad()
    def store(self, agent, done, status):
        """transition() + ONE agent.store_transition over the N * NR rows: what the agent was asked on (obs), what it answered
        (actions), reward, next_obs, terminal, valid= -- the store compacts the valid rows in (arena, robot) order.  Call it after
        env.step_thrust and before the next act()."""
        n = self.env.num_envs * self.env.preset.nr
        self.transition(done, status)
        agent.store_transition(self._obs[:n], self._actions[:n], self._reward, self._next_obs, self._terminal, valid=self._valid)


_OBSERVER_OF_KIND = {0: "SingleBall_6wayLidar_v2", 1: "SingleBall_6wayLidar"}
