"""Host-side mirror of the reference's gym.Env surface for the batched MI355X simulator.

Reference boundary (harman097/RoboRugby): `gym.make('RoboRugbySimpleDuel-v3')` -> `SimpleDuel3`
(robo_rugby/gym_env/RR_Environments.py:27-32) whose `reset/step/get_game_state/observation_space/action_space/
spec/metadata/unwrapped/render/seed/close` are what Training_DQN_pytorch.py:239-360 touches.  Here the same
names drive N arenas at once; obs/reward/done are PyTorch-ROCm tensors that never leave the device, and the step
itself is one HIP kernel launch through the C-ABI (include/roborugby_amd.h).  PyTorch is plumbing only (device
memory + streams).  No CPU fallback exists: without the HIP library / a GPU this module raises.
"""
import ctypes as C
import math
import numbers
import types

import numpy as np
import torch

from . import _lib
from ._lib import ptr
from .config import PRESETS, ENV_IDS, Preset
from .spaces import Box, Discrete

STATUS_BITS = {
    1: "UNABLE TO RESOLVE BOT/BOT COLLISIONS",            # RR_EnvBase.py:313
    2: "ROBOTS STUCK FROM PRIOR FRAME.",                  # RR_EnvBase.py:328
    4: "UNABLE TO UNDO MOVE FOR ROBOT",                   # RR_EnvBase.py:325
    8: "UNABLE TO RESOLVE ALL COLLISIONS FOR FRAME",      # RR_EnvBase.py:421
    16: "Really tho?? The balls are in the EXACT same spot????",  # RR_TrashyPhysics.py:250
    32: "Numerator AND Denominator are both 0.",          # MyUtils.py:25
    64: "Game is over. Go home.",                         # RR_EnvBase.py:262
    128: "action outside Direction 0..7",                 # KeyError at RR_EnvBase.py:606
}
STATUS_WARN, STATUS_RESET_GAVE_UP, STATUS_WAS_RESET = 256, 512, 1024
STATUS_GOAL_H_DESTROYED, STATUS_GOAL_G_DESTROYED, STATUS_NO_BALLS = 2048, 4096, 8192  # opt-in goal scoring only
STATUS_NOT_READY = 16384  # budgeted step only (step_budget_clocks > 0): the arena's step is still in progress
STATUS_FLAG_MASK, STATUS_NAUGHTY_SHIFT = 0xFFFF, 16  # info.status: flags in bits 0-15, NaughtyBots' robots in bits 16+

# reward mixins of RR_ScoreKeepers.py (ids of the C-ABI's keeper program) and observer mixins of RR_Observers.py
KEEPERS = {"NaughtyBots": 1, "ChasePosBall": 2, "PushPosBallsToGoal": 3, "DontDriveInGoals": 4, "KeepMovingGuys": 5,
           "BaseDestruction": 6, "PushNegBallsFromGoal": 7}
OBSERVERS = {"SingleBall_6wayLidar_v2": 0, "SingleBall_6wayLidar": 1, "PosBall_BasicLidar": 2, "AllCoords": 3,
             "AllCoords_WithPrior": 4}


def observer_dim(kind, nr, nb):
    return {0: 11, 1: 11, 2: 5, 3: 3 * nr + 2 * nb, 4: 6 * nr + 4 * nb}[kind]
SIMPLE_DUEL3_REWARDS = ("PushPosBallsToGoal", "ChasePosBall", "NaughtyBots")  # RR_Environments.py:27-32


def keeper_exec_order(mro_names):
    """on_step_end execution order of a keeper stack given in class (MRO) order: every keeper calls super() first --
    so the LAST one listed runs first -- except NaughtyBots, whose on_step_end never calls super()
    (RR_ScoreKeepers.py:130-135): keepers listed after it do not run at all."""
    names = list(mro_names)
    for n in names:
        if n not in KEEPERS:
            raise KeyError(f"unknown score keeper {n!r}; available: {sorted(KEEPERS)}")
    if "NaughtyBots" in names:
        names = names[:names.index("NaughtyBots") + 1]
    return [KEEPERS[n] for n in reversed(names)]


class Direction:  # GameEnv_Simple.Direction (RR_EnvBase.py:583-591)
    FORWARD, BACKWARD, LEFT, RIGHT, F_L, F_R, B_L, B_R = range(8)


class DebugInfo(dict):
    """RR_EnvBase.py:562-566: a dict (so wrappers can add keys) with the grumpy team's view as attributes."""

    def __init__(self, adblGrumpyState, dblGrumpyScore, status=None):
        super().__init__()
        self.adblGrumpyState = adblGrumpyState
        self.dblGrumpyScore = dblGrumpyScore
        self.status = status


def _expect(what, t, dtypes, numel, at_least=False, device=None):
    """The contract of a tensor handed to a launch -- contiguous, one of `dtypes`, exactly (at_least: at least) `numel` elements, on
    `device` when one is named -- as an AssertionError"""
    assert t.dtype in dtypes and t.is_contiguous() and (t.numel() >= numel if at_least else t.numel() == numel) \
        and (device is None or t.device == device), f"{what}: a contiguous {' / '.join(str(d) for d in dtypes)} tensor of " \
        f"{'at least ' if at_least else ''}{numel} elements{'' if device is None else f' on {device}'}"


_I32, _U8 = (torch.int32,), (torch.uint8, torch.bool)


# rr_config.dtype (include/roborugby_amd.h): "f64" = the reference's arithmetic, state and arithmetic in fp64 (parity mode, default);
# "f32_state" = BASELINE config 2's "fp32 state": the arenas' records in HBM are fp32, a step computes in fp64 between loading a record
# and writing it back (single steps within 1e-5 of the fp64 reference, contact steps included: tests/test_gpu_fp32.py); "f32" = state
# and arithmetic in fp32, the fast mode (quiet steps within 1e-5, contact steps statistically).
DTYPES = {"f64": 0, "f32": 1, "f32_state": 2}


class BatchedRoboRugbyEnv:
    """N lockstep arenas of SimpleDuel3 on one MI355X.

    reset() -> obs float32[N,11];  step(actions) -> (obs float32[N,11], reward float32[N], done bool[N], info)
    with info.adblGrumpyState float32[N,11] | None, info.dblGrumpyScore float32[N], info.status int32[N] (fault / reset flags
    in bits 0-15, the robots NaughtyBots flagged this step in bits 16+).

    time_limit=True reports done when step_count == max_episode_steps like gym's TimeLimit wrapper does for the
    DQN script; False is the raw env rule (step_count > T, RR_EnvBase.py:555-559).  With auto_reset=True a step
    on a finished arena re-places it (status bit 1024, reward 0, done False, obs = first obs of the new episode)
    instead of raising "Game is over" -- the policy's action for that arena is ignored on that call.  With
    reset_on_fault (default = auto_reset) a step in which the reference would have raised or hung
    (info.status bits 1|2|4|8|16|32) also reports done=True, so faulted arenas are re-placed instead of lingering.

    step_budget_clocks > 0 selects the BUDGETED step (opt-in extension, include/roborugby_amd.h): a call no longer waits for its
    slowest arena -- an arena whose wavefront is over the budget (shader clocks) at the end of an expensive physics sub-step
    parks there, the call reports STATUS_NOT_READY for it (reward 0, done False, its observation row keeps the previous
    values: step() then hands out persistent buffers) and the next call resumes it, ignoring the action it is given.  Each
    arena's trajectory as a function of the actions it accepted is bit-identical to the synchronous mode.
    """
    metadata = {"render.modes": ["human", "rgb_array"], "video.frames_per_second": 30}
    reward_range = (-float("inf"), float("inf"))

    def __init__(self, num_envs, preset="T", device=None, seed=0, time_limit=True, auto_reset=True, dtype="f64",
                 arena_offset=0, env_id="RoboRugbySimpleDuel-v3", reset_on_fault=None, action_mode="discrete",
                 rewards=SIMPLE_DUEL3_REWARDS, observer="SingleBall_6wayLidar_v2", lst_starting_config=None,
                 goal_scoring=False, step_budget_clocks=0, exact_trig=False):
        self.preset = PRESETS[preset] if isinstance(preset, str) else preset
        assert isinstance(self.preset, Preset)
        if not torch.cuda.is_available():
            raise RuntimeError("roborugby_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.type != "cuda":
            raise ValueError("device must be a ROCm/HIP device ('cuda:N')")
        self.num_envs = int(num_envs)
        if dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {sorted(DTYPES)}")
        if dtype == "f32_state" and step_budget_clocks:
            raise ValueError("dtype 'f32_state' has no budgeted step (a parked arena's record would be rounded in the middle of its step)")
        self.dtype = dtype
        self.time_limit, self.auto_reset = bool(time_limit), bool(auto_reset)
        # where the reference would raise / hang inside step() the episode ends (done=True + status bit) so that
        # auto-reset re-places the arena; default: on exactly when auto_reset is
        self.reset_on_fault = bool(auto_reset if reset_on_fault is None else reset_on_fault)
        p = self.preset
        # exact_trig=True: the parity build (libroborugby_amd_exact.so, same ABI): sin / cos of the robot kinematics ~correctly rounded and
        # the reference's scratch-rect carry (set_scratch_rect), so free-running episodes follow the reference bit for bit -- most of them
        # to their last step; ~80 % of the default library's speed, fp64 only
        self.exact_trig = bool(exact_trig)
        if self.exact_trig and dtype != "f64":
            raise ValueError("exact_trig is a property of the fp64 parity mode")
        counts = (p.nr_happy, p.nr_grumpy, p.nb_pos, p.nb_neg)
        from . import build as _build
        if counts in _build.BUILT_SHAPES:
            lib = _lib.load(exact=self.exact_trig)
        else:  # the reference's entity counts are free integers (RR_Constants.py:30-34): a library for this one shape, compiled on demand
            if dtype == "f32":
                raise ValueError("entity counts outside the built shapes: dtype 'f64' or 'f32_state'")
            lib = _lib.load_shape(counts, exact=self.exact_trig)
        cfg = _lib.RRConfig(
            struct_size=C.sizeof(_lib.RRConfig), num_envs=self.num_envs, nr_happy=p.nr_happy, nr_grumpy=p.nr_grumpy,
            nb_pos=p.nb_pos, nb_neg=p.nb_neg, arena_w=p.arena_w, arena_h=p.arena_h, game_len_steps=p.game_len_steps,
            game_mode=int(p.game_mode), time_limit=int(self.time_limit), auto_reset=int(self.auto_reset),
            reset_on_fault=int(self.reset_on_fault),
            dtype=DTYPES[dtype], device=self.device.index or 0, seed=int(seed),
            arena_offset=int(arena_offset), step_budget_clocks=int(step_budget_clocks), reserved_=0)
        self.step_budget_clocks = int(step_budget_clocks)
        self._bout = None  # persistent step outputs of the budgeted mode (NOT_READY rows keep their previous observation)
        self._handle = _lib.EnvHandle.create(lib, cfg, self.device)
        # other mixin stacks of the reference: `rewards` in class order like the reference's env classes
        # (RR_Environments.py), `observer` one of OBSERVERS.  SimpleDuel3's own stack is the default and stays fused in
        # the step kernel; anything else runs in light side kernels around it.
        if observer not in OBSERVERS:
            raise KeyError(f"unknown observer {observer!r}; available: {sorted(OBSERVERS)}")
        self.observer, self.obs_kind = observer, OBSERVERS[observer]
        self.obs_dim = observer_dim(self.obs_kind, p.nr, p.nb)
        if self.obs_kind == 4:  # the prior-step copies have to be snapshotted at every on_step_begin from now on
            self.track_prior_step()
        self.rewards = tuple(rewards)
        prog = np.asarray(keeper_exec_order(self.rewards), np.int32)
        self._handle.call("rr_set_reward_program", prog.ctypes.data_as(C.c_void_p), len(prog))
        # Opt-in goal scoring -- an EXTENSION: the reference's goals never score on its live path
        # (RR_Goal.py:58-91 is only reached from the never-called __old_step and is broken), so this has no reference behaviour
        # to match.  A ball inside a goal triangle for 150 consecutive steps is consumed (out of play), +-500 points, three
        # negative balls destroy a goal, a destroyed goal / an empty field ends the episode (include/roborugby_amd.h).
        self.goal_scoring = bool(goal_scoring)
        if self.goal_scoring:
            self._handle.launch("rr_set_goal_scoring", 1)
        m = max(p.arena_w, p.arena_h, 360)  # RR_Observers.py:30-37
        self.observation_space = Box(-m, m, (self.obs_dim,), np.float32)
        # GameEnv_Simple: Discrete(8) (RR_EnvBase.py:610); bare GameEnv: Box(-1, 1, (2*happy robots,)) (RR_EnvBase.py:118-123),
        # the surface Training_SAC_pytorch.py:270,423 reads (`action_space.high`, `.shape[0]`)
        if action_mode not in ("discrete", "thrust"):
            raise ValueError("action_mode must be 'discrete' or 'thrust'")
        self.action_mode = action_mode
        self.action_space = Discrete(8) if action_mode == "discrete" else Box(-1.0, 1.0, (2 * p.nr_happy,), np.float32)
        self.spec = types.SimpleNamespace(id=env_id, max_episode_steps=p.game_len_steps, nondeterministic=True,
                                          reward_threshold=1.0)  # robo_rugby/__init__.py:28-34
        self.has_grumpy = p.nr_grumpy > 0
        # GameEnv.__init__ (RR_EnvBase.py:111-116): CONFIG_RANDOM keeps what _set_random_positions returned at
        # construction, a given lst_starting_config ([[(x, y, rot) x NR], [(x, y) x NB]], one layout for every arena or a
        # pair of [N, ...] arrays) is applied at once; either way reset(bln_randomize_pos=False) goes back to it.
        if lst_starting_config is None:
            st = self.get_state()
            self._start_robots = st["robots"][:, :, [0, 1, 6]].contiguous()
            self._start_balls = torch.cat([st["balls"][:, :, :2], torch.zeros_like(st["balls"][:, :, :2])], dim=2).contiguous()
        else:
            if len(lst_starting_config) != 2:  # RR_EnvBase.py:135-136
                raise Exception(f"Expected list of 2 lists. Not whatever this is: {lst_starting_config}")
            r = torch.as_tensor(np.asarray(lst_starting_config[0], dtype=np.float64), device=self.device)
            b = torch.as_tensor(np.asarray(lst_starting_config[1], dtype=np.float64), device=self.device)
            if r.shape[-2:] != (p.nr, 3):  # RR_EnvBase.py:138-139
                raise Exception(f"Robot count mismatch. {p.nr} != {r.shape[-2] if r.dim() >= 2 else r.shape}.")
            if b.shape[-2:] != (p.nb, 2):  # RR_EnvBase.py:141-142
                raise Exception(f"Ball count mismatch. {p.nb} != {b.shape[-2] if b.dim() >= 2 else b.shape}.")
            self._start_robots = r.expand(self.num_envs, p.nr, 3).contiguous()
            b = b.expand(self.num_envs, p.nb, 2)
            self._start_balls = torch.cat([b, torch.zeros_like(b)], dim=2).contiguous()
            self._reset_to_start(None, None)
        if self.step_budget_clocks:
            self._seed_bout()

    # ---------------------------------------------------------------- helpers
    @property
    def unwrapped(self):
        return self

    # the C-ABI's handle, its library and the current stream, as tests and tools hand them to raw calls
    _h = property(lambda self: self._handle.h)
    _lib = property(lambda self: self._handle.lib)

    def _stream(self):
        return self._handle.stream()

    def _new(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _step_outputs(self, lead, fd=torch.float32, alloc=torch.empty):
        """(obs, reward, done_u8, obs_g, reward_g, status) of a step: leading shape `lead` -- (N,), a rollout's (S, N) --, float dtype fd"""
        def new(*tail, dtype=fd):
            return alloc(lead + tail, dtype=dtype, device=self.device)
        return new(11), new(), new(dtype=torch.uint8), new(11) if self.has_grumpy else None, new(), new(dtype=torch.int32)

    def _step_result(self, obs, rew, done, obs_g, rew_g, status, observe=True):
        """what a step returns from its six outputs; observe: under another observer than the fused one, that observer's view"""
        if observe and self.obs_kind != 0:
            obs, obs_g = self.get_game_state(1), (self.get_game_state(-1) if self.has_grumpy else None)
        return obs, rew, done.view(torch.bool), DebugInfo(obs_g, rew_g, status)

    def _set(self, name, *tensors, reseed=True):
        """The tail of a setter: the launch, a wait for it (the inputs may be temporaries) and -- reseed: set_state and set_poses, which
        rewrite the poses the observations are made of -- on a handle that has had a budget the persistent step outputs seeded again"""
        self._handle.launch(name, *map(ptr, tensors))
        torch.cuda.current_stream(self.device).synchronize()
        if reseed and self._bout is not None:
            self._seed_bout()

    def _seed_bout(self, mask=None, obs=None):
        """Budgeted mode: the persistent step outputs, with both teams' observation rows of the arenas in `mask` (None: all) set to
        the CURRENT observation -- a row that is NOT_READY in the next step() is not written by the kernel and must read as the
        arena's previous observation.  Called when the first budget is set and for the rows of arenas rewritten from outside (all of
        them after set_state / set_poses / reset(), the masked ones after reset(mask), which passes the happy rows it returns as
        `obs`); the other rows keep what step() handed out: a parked arena's record holds the middle of its step, not an observation."""
        N = self.num_envs
        if self._bout is None:
            self._bout = self._step_outputs((N,), alloc=torch.zeros)  # (reward, done and status read 0 until a step writes them)
            mask = None
        for team, rows in ((1, self._bout[0]), (-1, self._bout[3])):
            if rows is None:
                continue
            if team == 1 and obs is not None:
                cur = obs
            else:
                cur = rows if mask is None else self._new((N, 11), torch.float32)
                self._handle.launch("rr_observe", team, -1, -1, ptr(cur))
            if mask is not None:
                rows.copy_(torch.where(mask.view(N, 1).bool(), cur, rows))
            elif cur is not rows:
                rows.copy_(cur)

    # ---------------------------------------------------------------- gym surface
    def _reset_to_start(self, mask, obs):
        self._handle.launch("rr_reset_to_poses", ptr(mask), ptr(self._start_robots), ptr(self._start_balls), ptr(obs), None)

    def _mask(self, mask):
        """uint8 [N] device mask; scalars / wrong sizes are rejected (the kernels index mask[arena] for every arena)."""
        if mask is None:
            return None
        if isinstance(mask, (bool, int, float)) or (hasattr(mask, "ndim") and mask.ndim == 0):
            raise TypeError("reset(mask=...): a per-arena mask of num_envs booleans is required, not a scalar "
                            "(the reference's reset(False) is reset(bln_randomize_pos=False) here)")
        m = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).contiguous().view(-1)
        if m.numel() != self.num_envs:
            raise ValueError(f"reset(mask=...): {m.numel()} entries for {self.num_envs} arenas")
        return m

    def reset(self, mask=None, *, bln_randomize_pos=True):
        """env.reset(bln_randomize_pos) (RR_EnvBase.py:202-216) for all arenas, or those where mask is True: a fresh random
        placement (_set_random_positions), or with bln_randomize_pos=False the start configuration kept since construction
        (_set_starting_positions, RR_EnvBase.py:131-153; main.py:107 replays its layout that way).
        Budgeted mode: an arena in the mask that is parked loses the rest of its step (like set_state); the rows outside the mask
        are each arena's previous observation -- for a parked arena the one the last step() without `out` handed out -- and the
        NOT_READY rows of the next step() keep them."""
        N = self.num_envs
        obs = self._new((N, 11), torch.float32)
        mask = self._mask(mask)
        if mask is not None:
            # rows that are not reset keep their current observation; a parked arena has none (its record is mid-step)
            self._handle.launch("rr_observe", 1, -1, -1, ptr(obs))
            if self._bout is not None:
                parked = (self._bout[5] & STATUS_NOT_READY) != 0
                obs = torch.where(parked.view(N, 1), self._bout[0], obs).contiguous()
        if bln_randomize_pos:
            self._handle.launch("rr_reset", ptr(mask), ptr(obs), None)
        else:
            self._reset_to_start(mask, obs)
        if self._bout is not None:  # budgeted mode: a NOT_READY row of the next step keeps these observations
            self._seed_bout(mask, obs)
        return obs if self.obs_kind == 0 else self.get_game_state(1)

    def starting_positions(self):
        """The retained start configuration in the reference's format per arena (GameEnv._lst_starting_positions):
        (robots [N,NR,3] x, y, rot ; balls [N,NB,2] x, y)."""
        return self._start_robots.clone(), self._start_balls[:, :, :2].clone()

    def step(self, actions, out=None):
        """GameEnv_Simple.step for every arena.  actions: int tensor [N] or [N,NA] (NA <= robots; action i drives
        robot i, happy robots first -- Training_DQN_pytorch.py:341 passes NA=1).  `out` may carry preallocated
        (obs, reward, done_u8, obs_g, reward_g, status) tensors to reuse."""
        N = self.num_envs
        a = torch.as_tensor(actions, device=self.device)
        if self.action_mode == "thrust" or a.is_floating_point():
            return self.step_thrust(a)
        if a.dim() == 1:
            a = a.view(N, 1)
        if a.shape[0] != N or a.dim() != 2:
            raise ValueError(f"actions must be [N] or [N,NA]; got {tuple(a.shape)}")
        if a.shape[1] > self.preset.nr:  # RR_EnvBase.py:621-622
            raise Exception(f"{a.shape[1]} commands but only {self.preset.nr} robots.")
        own = out is None and (bool(self.step_budget_clocks) or self._bout is not None)  # (budget 0 after a budget: parks may remain)
        if own:
            if self._bout is None:  # rows of parked arenas are not written: they must find their previous observation here
                self._seed_bout()
            out = self._bout
        out = self._step_discrete("rr_step", a, out)
        if own:  # hand out copies: the persistent buffers are overwritten by the next call
            out = [t.clone() if t is not None else None for t in out]
        return self._step_result(*out)

    def _step_discrete(self, name, a, out=None, fd=torch.float32):
        """What step and step_f64 share: rr_step / rr_step_f64 on the actions a [N, NA] into `out`, or into fresh outputs of float
        dtype fd -> the six outputs"""
        a = a.to(torch.int32).contiguous()
        if out is None:
            out = self._step_outputs((self.num_envs,), fd)
        self._handle.launch(name, ptr(a), a.shape[1], *map(ptr, out))
        return out

    def set_step_budget(self, clocks):
        """rr_set_step_budget: switch the budgeted step on (clocks > 0) or off (0: parked arenas finish in the next calls), or change
        the budget.  Arenas parked at the time go on with their step; the NOT_READY rows of step() keep their previous observation
        (once a handle has had a budget, step() without `out` hands out the persistent buffers whatever the budget)."""
        self._handle.call("rr_set_step_budget", int(clocks))
        self.step_budget_clocks = int(clocks)
        if self.step_budget_clocks and self._bout is None:
            self._seed_bout()

    def rollout(self, actions, repeat=None, out=None):
        """Open-loop rollout in ONE launch: `actions` int [S, N] / [S, N, NA] steps the batch S times (or, with
        `repeat=S`, int [N] / [N, NA] is applied S times: action repeat / frame skip).  Returns (obs [S,N,11],
        reward [S,N], done [S,N], DebugInfo with [S,...] members): bit-identical to S step() calls, but no arena waits
        for the slowest arena of the batch between steps.  Build-side extension (rr_rollout); the reference's gym API steps
        one call at a time."""
        N = self.num_envs
        a = torch.as_tensor(actions, device=self.device).to(torch.int32)
        if repeat is not None:
            S = int(repeat)
            a = (a.view(N, 1) if a.dim() == 1 else a).contiguous()
            na, rep = a.shape[1], 1
        else:
            if a.dim() == 2:
                a = a.unsqueeze(-1)
            a = a.contiguous()
            S, na, rep = a.shape[0], a.shape[2], 0
        if a.shape[-2] != N or self.action_mode != "discrete" or self.obs_kind != 0:
            raise ValueError("rollout: discrete actions [S,N(,NA)] and the default observer only")
        if out is None:
            out = self._step_outputs((S, N))
        self._handle.launch("rr_rollout", ptr(a), na, S, rep, *map(ptr, out))
        return self._step_result(*out)

    def step_thrust(self, thrust, f64=False):
        """GameEnv.step with continuous (L,R) thrust pairs (RR_EnvBase.py:260-273): float tensor [N, 2*k].  f64=True returns the
        observation / reward in fp64 (rr_step_thrust_f64: the entry's parity checks)."""
        N = self.num_envs
        t = torch.as_tensor(thrust, device=self.device, dtype=torch.float32).contiguous().view(N, -1)
        if t.shape[1] % 2 or t.shape[1] > 2 * self.preset.nr:  # RR_EnvBase.py:270-271
            raise Exception(f"{t.shape[1]} commands but only {self.preset.nr * 2} robot engines.")
        out = self._step_outputs((N,), torch.float64 if f64 else torch.float32)
        self._handle.launch("rr_step_thrust_f64" if f64 else "rr_step_thrust", ptr(t), t.shape[1] // 2, *map(ptr, out))
        return self._step_result(*out)

    def step_f64(self, actions):
        """Same step with fp64 outputs (parity checks against the fp64 reference arithmetic)."""
        N = self.num_envs
        a = torch.as_tensor(actions, device=self.device)
        out = self._step_discrete("rr_step_f64", a.view(N, 1) if a.dim() == 1 else a, fd=torch.float64)
        return self._step_result(*out, observe=False)  # (the fused observer's, whatever the env's own)

    def get_game_state(self, int_team=None, robot_idx=-1, ball_idx=-1, f64=False, observer=None):
        """get_game_state of the configured (or named) observer mixin (RR_Observers.py); None when the reference
        returns None (the team has no robot)."""
        team = 1 if int_team is None else int(int_team)
        kind = self.obs_kind if observer is None else OBSERVERS[observer]
        if kind not in (3, 4) and robot_idx < 0 and ((team == 1 and self.preset.nr_happy == 0) or (team == -1 and self.preset.nr_grumpy == 0)):
            return None
        dim = observer_dim(kind, self.preset.nr, self.preset.nb)
        obs = self._new((self.num_envs, dim), torch.float64 if f64 else torch.float32)
        self._handle.launch("rr_observe_kind_f64" if f64 else "rr_observe_kind", kind, team, int(robot_idx), int(ball_idx), ptr(obs), dim)
        return obs

    @property
    def has_had_budget(self):
        """the handle has, or has had, a step budget: arenas may be parked mid-step (the hive then holds their rows)"""
        return bool(self.step_budget_clocks) or self._bout is not None

    def hive_observe(self, robot_mask=None, observer=None, f64=False, out=None, held=False):
        """The hive-mind player's view (DQN_pytorch_player.py: Stephen.__ponder + the observation __consult asks for) of every arena in
        one launch (rr_hive_observe): -> (assign int32 [N,NR], obs [N,NR,11]).  assign[a, r] is the ball robot r of arena a goes for --
        greedy, nearest (robot, ball) pair first, balls lying in a goal ignored -- or -1 (no ball left, or r is outside the hive);
        obs[a, r] = get_game_state(robot_idx=r, ball_idx=assign[a, r]) seen from r's own team, 0 where assign is -1.
        robot_mask: bit r = robot r belongs to the hive (None: every happy robot); observer: 'SingleBall_6wayLidar_v2' or
        'SingleBall_6wayLidar' (None: the env's own when it is one of the two, else the former); out: (assign, obs) to reuse.
        held=True (rr_hive_observe_held, the budgeted step): -> (assign, obs, held uint8 [N]); the rows of an arena parked mid-step are
        NOT written -- they stay what `out` holds, the rows of the step it is in the middle of -- and held is 1 there; out: (assign, obs,
        held) to reuse (without `out` the rows of held arenas are 0 / -1)."""
        N, nr = self.num_envs, self.preset.nr
        mask, kind, od = self._hive_args(robot_mask, observer, f64)
        if out is None and held:
            out = (torch.full((N, nr), -1, dtype=torch.int32, device=self.device), torch.zeros((N, nr, 11), dtype=od, device=self.device),
                   self._new((N,), torch.uint8))
        elif out is None:
            out = (self._new((N, nr), torch.int32), self._new((N, nr, 11), od))
        out = tuple(out[:3 if held else 2])
        _expect("assign", out[0], _I32, N * nr)
        _expect("obs", out[1], (od,), N * nr * 11, at_least=True)
        if held:
            _expect("held", out[2], _U8, N, device=self.device)
        self._handle.launch("rr_hive_observe" + ("_held" if held else "") + ("_f64" if f64 else ""), mask, kind, *map(ptr, out))
        return out

    def _hive_args(self, robot_mask, observer, f64=False):
        """What every hive entry starts with -> (mask, kind, float dtype).  robot_mask: one bit per robot, None = the happy team;
        observer: None = the env's own when it is SingleBall_6wayLidar(_v2), else SingleBall_6wayLidar_v2; f64: the outputs' dtype"""
        mask = (1 << self.preset.nr_happy) - 1 if robot_mask is None else int(robot_mask)
        if mask < 0 or mask > 0xFFFFFFFF:
            raise ValueError("robot_mask: one bit per robot")
        kind = (self.obs_kind if self.obs_kind in (0, 1) else 0) if observer is None else OBSERVERS[observer]
        return mask, kind, torch.float64 if f64 else torch.float32

    def hive_commit(self, fresh, assign, held, accepted, thrust, robot_mask=None):
        """The tail of the hive's turn under the budgeted step, in one launch (rr_hive_commit): for every arena that is not held and every
        robot of the mask, accepted[a, r] = fresh[a, r] and thrust[a, 2r:2r+2] = the (L, R) pair of that direction -- (0, 0) without a ball
        (assign < 0) or for a value outside 0..7.  Held arenas and robots outside the mask keep what `accepted` and `thrust` hold.
        fresh, assign, accepted: int32 [N,NR]; held: uint8 [N] (hive_observe(held=True)); thrust: float32 [N,2*NR].  -> (accepted, thrust)"""
        N, nr, dev = self.num_envs, self.preset.nr, self.device
        mask = self._hive_args(robot_mask, None)[0]
        for what, t in (("fresh", fresh), ("assign", assign), ("accepted", accepted)):
            _expect(what, t, _I32, N * nr, at_least=True, device=dev)
        _expect("held", held, _U8, N, device=dev)
        _expect("thrust", thrust, (torch.float32,), N * 2 * nr, device=dev)
        self._handle.launch("rr_hive_commit", mask, ptr(fresh), ptr(assign), ptr(held), ptr(accepted), ptr(thrust))
        return accepted, thrust

    def track_prior_step(self, on=True):
        """rr_track_prior_step: every step from now on first snapshots what the sprites' on_step_begin copies (robot and ball centres at
        the step's begin).  observer='AllCoords_WithPrior' switches it on by itself; hive_transition needs it on BEFORE the step it
        looks back on."""
        self._handle.launch("rr_track_prior_step", int(bool(on)))

    def hive_transition(self, assign, status, done, robot_mask=None, observer=None, f64=False, out=None):
        """Training the hive in the full game: the transition of every hive robot over the step that was just taken, in one launch
        (rr_hive_transition) -> (next_obs [N,NR,11], reward [N,NR], terminal uint8 [N,NR], valid uint8 [N,NR]).
        assign: what hive_observe returned BEFORE the step; status, done: the step's (info.status, done).  A row is valid when its robot
        is in the mask, was given a ball, the arena really stepped (not re-placed, not STEP_AFTER_DONE) and the ball is still in play;
        then next_obs is the robot's observation of THE SAME ball after the step, reward the per-robot reward defined in
        include/roborugby_amd.h and terminal = done.  Invalid rows are 0.  Needs track_prior_step() before the step; refuses a handle with
        a step budget (hive_transition_held is the entry for one).  robot_mask / observer / f64 as in hive_observe; out: the four
        tensors to reuse."""
        return self._hive_transition("rr_hive_transition", assign, status, done, robot_mask, observer, f64, out)

    def hive_transition_held(self, assign, status, done, robot_mask=None, observer=None, f64=False, out=None):
        """hive_transition on a handle with a step budget (rr_hive_transition_held): the same rows, bit for bit -- for a caller that held
        the rows of parked arenas (hive_observe(held=True) -> hive_commit, the same buffers every call): a valid row is then the
        transition of the step the arena accepted, however many calls that step took.  Arguments as hive_transition's."""
        return self._hive_transition("rr_hive_transition_held", assign, status, done, robot_mask, observer, f64, out)

    def _hive_transition(self, name, assign, status, done, robot_mask, observer, f64, out):
        N, nr, dev = self.num_envs, self.preset.nr, self.device
        mask, kind, od = self._hive_args(robot_mask, observer, f64)
        if out is None:
            out = (self._new((N, nr, 11), od), self._new((N, nr), od), self._new((N, nr), torch.uint8), self._new((N, nr), torch.uint8))
        next_obs, reward, terminal, valid = out
        done = done.view(torch.uint8) if done.dtype == torch.bool else done
        _expect("assign", assign, _I32, N * nr, device=dev)
        _expect("status", status, _I32, N, device=dev)
        _expect("done", done, (torch.uint8,), N, device=dev)
        _expect("next_obs", next_obs, (od,), N * nr * 11, at_least=True)
        _expect("reward", reward, (od,), N * nr, at_least=True)
        _expect("terminal", terminal, _U8, N * nr, at_least=True)
        _expect("valid", valid, _U8, N * nr, at_least=True)
        self._handle.launch(name + ("_f64" if f64 else ""), mask, kind, ptr(assign), ptr(status), ptr(done), *map(ptr, out))
        return next_obs, reward, terminal, valid

    def render(self, mode="human", arena=0):
        """The pygame window (RR_EnvBase.py:218-258) is UI and out of scope: 'human' is a no-op so callers' render()
        stays harmless; 'rgb_array' returns a CPU debug picture of ONE arena (arena width + 300-px dashboard strip like
        the reference's surface) drawn with PIL from the device state."""
        if mode == "human":
            return None
        if mode != "rgb_array":
            raise NotImplementedError("Other mode types not supported.")
        from .render import draw_arena
        st = self.get_state()
        return draw_arena(self.preset, st["robots"][arena].cpu().numpy(), st["balls"][arena].cpu().numpy())

    RENDER_BATCH_MAX_BYTES = 1 << 30

    def render_batch(self, arenas=None, width=None, height=None, samples=1, out=None):
        """RGB frames of many arenas in one launch, straight from the records on the device (rr_render; the picture is specified in
        include/roborugby_amd.h): -> uint8 [M, height, width, 3] on the env's device, enqueued on the current stream.  The field only --
        no dashboard strip --, scaled independently in x and y; `samples` (1, 2 or 4) per axis and pixel, box-filtered.
        arenas: an int tensor or a sequence of arena indices (any order, duplicates allowed; an index outside 0 .. N-1 gives an
        all-zero frame), None: every arena.  width / height: None = the native int(arena_w) x int(arena_h); width a multiple of 4.
        out: a contiguous uint8 tensor of M * height * width * 3 elements on the device to write into.  Raises ValueError before any
        launch when the result would exceed 1 GiB."""
        p = self.preset
        w = int(p.arena_w) if width is None else int(width)
        h = int(p.arena_h) if height is None else int(height)
        idx = None if arenas is None else self._index_list(arenas, "render_batch(arenas=...)")
        m = self.num_envs if idx is None else int(idx.numel())
        out = self._frames("render_batch", m, w, h, (m, h, w, 3), out)
        self._handle.launch("rr_render", ptr(idx), m, w, h, int(samples), ptr(out))
        return out

    def _index_list(self, x, where):
        """int32 device tensor of a 1-D sequence of integer indices (render_batch / render_ego: arenas, robots)"""
        x = torch.as_tensor(x)
        if x.is_floating_point() or x.dtype == torch.bool or x.dim() != 1:
            raise ValueError(f"{where}: a 1-D sequence of integer indices")
        return x.to(device=self.device, dtype=torch.int32).contiguous()

    def _frames(self, method, m, w, h, shape, out):
        """The m frames of w x h RGB pixels `method` (render_batch / render_ego) writes, as `shape`: `out` when it is given and fits,
        else a new tensor; ValueError for no frame at all, for more than RENDER_BATCH_MAX_BYTES and for an `out` that does not fit"""
        if m < 1 or w < 1 or h < 1:
            raise ValueError(f"{method}: at least one frame of at least one pixel")
        if m * h * w * 3 > self.RENDER_BATCH_MAX_BYTES:
            raise ValueError(f"{method}: {m} frames of {w}x{h} are {m * h * w * 3 / 2 ** 30:.2f} GiB, above the 1 GiB a call may write; "
                             "render fewer frames per call or smaller ones")
        if out is None:
            return self._new(shape, torch.uint8)
        if not (out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == m * h * w * 3 and out.device == self.device):
            raise ValueError(f"{method}(out=...): a contiguous uint8 tensor of {m}x{h}x{w}x3 elements on {self.device}")
        return out.view(shape)

    def render_ego(self, arenas=None, robots=None, width=64, height=None, span=400.0, ahead=0.0, samples=1, relative=True, planar=False,
                   out=None):
        """Egocentric RGB frames, one per (arena, robot), in one launch, straight from the records on the device (rr_render_ego; the
        picture is specified in include/roborugby_amd.h): -> uint8 [M, height, width, 3], or [M, 3, height, width] when `planar`, on the
        env's device, enqueued on the current stream.  A frame is centred on its robot -- `ahead` arena units in front of it, when given --
        with the robot's front up; it covers `span` arena units across, at the same scale downwards; beyond the walls it is grey.
        relative: a grumpy viewer sees the team, ball and goal colours swapped, so that "mine" looks the same for either team.
        arenas: as in render_batch (None: every arena).  robots: the viewing robot, happy robots first -- an int for every frame, or a
        1-D int sequence / tensor of length M (None: robot 0); an index outside 0 .. NR-1 gives an all-zero frame, as does a viewer with a
        non-finite pose.  height: None = width; width a multiple of 4.  out: a contiguous uint8 tensor of M * height * width * 3
        elements on the device to write into.  Raises ValueError before any launch when the result would exceed 1 GiB."""
        w = int(width)
        h = w if height is None else int(height)
        idx = None if arenas is None else self._index_list(arenas, "render_ego(arenas=...)")
        m = self.num_envs if idx is None else int(idx.numel())
        rob = None
        if robots is not None:
            if isinstance(robots, numbers.Integral) and not isinstance(robots, bool):
                rob = torch.full((max(m, 1),), int(robots), dtype=torch.int32, device=self.device) if int(robots) != 0 else None
            else:
                rob = self._index_list(robots, "render_ego(robots=...)")
                if int(rob.numel()) != m:
                    raise ValueError(f"render_ego(robots=...): {int(rob.numel())} robots for {m} frames")
        out = self._frames("render_ego", m, w, h, (m, 3, h, w) if planar else (m, h, w, 3), out)
        flags = (1 if relative else 0) | (2 if planar else 0)  # RR_EGO_RELATIVE, RR_EGO_PLANAR
        self._handle.launch("rr_render_ego", ptr(idx), ptr(rob), m, w, h, int(samples), float(span), float(ahead), flags, ptr(out))
        return out

    def seed(self, seed=None):
        """Like the reference (RR_EnvBase.py:568-570) this does not re-seed placement; the reset RNG is keyed at
        construction (`seed=`)."""
        return [seed]

    def close(self):
        if getattr(self, "_handle", None):  # (its own __del__ destroys a handle nobody closed)
            self._handle.close()

    # ---------------------------------------------------------------- state exchange / logging
    def get_state(self):
        """Canonical fp64 state (layout in include/roborugby_amd.h): dict of device tensors."""
        p, N = self.preset, self.num_envs
        robots = self._new((N, p.nr, 10), torch.float64)
        robots_i = self._new((N, p.nr, 3), torch.int32)
        balls = self._new((N, p.nb, 8), torch.float64)
        step = self._new((N,), torch.int32)
        self._handle.launch("rr_get_state", ptr(robots), ptr(robots_i), ptr(balls), ptr(step))
        return dict(robots=robots, robots_i=robots_i, balls=balls, step=step)

    def set_scratch_rect(self, xy):
        """Parity build only (exact_trig=True): centre of the reference's module-global scratch rect, [N,2] fp64 -- e.g. the
        `state_inner[..., :2]` a golden trajectory dumped (include/roborugby_amd.h: rr_set_scratch_rect)."""
        xy = torch.as_tensor(xy, dtype=torch.float64, device=self.device).contiguous().view(self.num_envs, 2)
        self._set("rr_set_scratch_rect", xy, reseed=False)

    def get_scratch_rect(self):
        xy = self._new((self.num_envs, 2), torch.float64)
        self._handle.launch("rr_get_scratch_rect", ptr(xy))
        return xy

    def get_episode_state(self):
        """Build-side bookkeeping that a checkpoint has to carry next to get_state(): `ints` [N,5] = episode index (keys the
        reset RNG: without it a resumed run would replay the placements of episodes 1, 2, ...), steps in the running
        episode, finished episodes, last episode's length, fault flag; `acc` [N,4] = running / last finished returns."""
        ints, acc = self._new((self.num_envs, 5), torch.int32), self._new((self.num_envs, 4), torch.float64)
        self._handle.launch("rr_get_episode_state", ptr(ints), ptr(acc))
        return dict(ints=ints, acc=acc)

    def set_episode_state(self, ints, acc):
        ints = torch.as_tensor(ints, dtype=torch.int32, device=self.device).contiguous().view(self.num_envs, 5)
        acc = torch.as_tensor(acc, dtype=torch.float64, device=self.device).contiguous().view(self.num_envs, 4)
        self._set("rr_set_episode_state", ints, acc, reseed=False)

    def checkpoint_state(self):
        """Everything a resumed run needs besides the agent: `env_state` (get_state), `episode` (get_episode_state: the episode index
        keys the reset RNG) and, for the parity build, `scratch_rect` (the reference's module-global rect, part of its state).
        Budgeted mode: take it only after a call in which no row was NOT_READY (set_step_budget(0) + one step() guarantees that):
        rr_set_state on resume clears a parked step, i.e. would drop the rest of that step and the action the arena accepted."""
        ck = dict(env_state=self.get_state(), episode=self.get_episode_state())
        if self.exact_trig:
            ck["scratch_rect"] = self.get_scratch_rect()
        return ck

    def load_checkpoint_state(self, ck):
        st = ck["env_state"]
        self.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
        if "episode" in ck:
            self.set_episode_state(ck["episode"]["ints"], ck["episode"]["acc"])
        if self.exact_trig and "scratch_rect" in ck:
            self.set_scratch_rect(ck["scratch_rect"])

    def set_state(self, robots, robots_i, balls, step):
        p, N = self.preset, self.num_envs
        robots = torch.as_tensor(robots, dtype=torch.float64, device=self.device).contiguous().view(N, p.nr, 10)
        robots_i = torch.as_tensor(robots_i, dtype=torch.int32, device=self.device).contiguous().view(N, p.nr, 3)
        balls = torch.as_tensor(balls, dtype=torch.float64, device=self.device).contiguous().view(N, p.nb, 8)
        step = torch.as_tensor(step, dtype=torch.int32, device=self.device).contiguous().view(N)
        self._set("rr_set_state", robots, robots_i, balls, step)

    def set_poses(self, robots_xyr, balls_xyv):
        """The reference's lst_starting_config (RR_EnvBase.py:35-52) per arena, plus ball velocities."""
        p, N = self.preset, self.num_envs
        r = torch.as_tensor(robots_xyr, dtype=torch.float64, device=self.device).contiguous().view(N, p.nr, 3)
        b = torch.as_tensor(balls_xyv, dtype=torch.float64, device=self.device).contiguous().view(N, p.nb, 4)
        self._set("rr_set_poses", r, b)

    def goal_scores(self):
        """Goal.get_score() of (happy, grumpy) goal (RR_Goal.py:87-88): identically 0 on the live path -- the reference
        never feeds its goal bookkeeping, so `done` is purely the step counter -- unless the env was
        built with goal_scoring=True (the opt-in extension): then 500 x (positive - negative balls the goal has consumed)."""
        s = self._new((self.num_envs, 2), torch.int32)
        self._handle.launch("rr_goal_scores", ptr(s))
        return s

    def episode_stats(self):
        """(last finished episode return happy, grumpy, its length, number of finished episodes) per arena."""
        N = self.num_envs
        lr, lrg = self._new((N,), torch.float32), self._new((N,), torch.float32)
        ll, cnt = self._new((N,), torch.int32), self._new((N,), torch.int32)
        self._handle.launch("rr_episode_stats", ptr(lr), ptr(lrg), ptr(ll), ptr(cnt))
        return lr, lrg, ll, cnt

    def lanes_per_env(self):
        v = C.c_int32()
        self._handle.call("rr_lanes_per_env", C.byref(v))
        return v.value

    def state_bytes_per_env(self):
        b = C.c_int64()
        self._handle.call("rr_state_bytes_per_env", C.byref(b))
        return b.value


class RoboRugbyEnv:
    """Single-arena, reference-shaped view: numpy in/out, Python exceptions where the reference raises.

    `env.step([action]) -> (ndarray[11], float, bool, DebugInfo)` exactly as Training_DQN_pytorch.py:341-343
    consumes it.  Backed by a BatchedRoboRugbyEnv with num_envs=1 on the GPU (no CPU path)."""
    metadata = BatchedRoboRugbyEnv.metadata
    reward_range = BatchedRoboRugbyEnv.reward_range

    def __init__(self, preset="T", device=None, seed=0, time_limit=True, dtype="f64", action_mode="discrete",
                 lst_starting_config=None, **kw):
        self._b = BatchedRoboRugbyEnv(1, preset=preset, device=device, seed=seed, time_limit=time_limit,
                                      auto_reset=False, dtype=dtype, action_mode=action_mode,
                                      lst_starting_config=lst_starting_config, **kw)
        self.observation_space = self._b.observation_space
        self.action_space = self._b.action_space
        self.spec = self._b.spec
        self.preset = self._b.preset
        self._f64 = dtype == "f64" and self._b.obs_kind == 0  # the reference hands out float64 ndarrays

    @property
    def unwrapped(self):
        return self

    def reset(self, bln_randomize_pos=True):
        """RR_EnvBase.py:202-216; reset(False) replays the layout kept since construction (main.py:107)."""
        obs = self._b.reset(bln_randomize_pos=bln_randomize_pos)
        if self._f64:
            obs = self._b.get_game_state(1, f64=True)
        return obs[0].double().cpu().numpy()

    def step(self, lstArgs):
        arr = np.concatenate([np.asarray(a).reshape(-1) for a in lstArgs], axis=None) if len(lstArgs) else np.zeros(0)
        if self._b.action_mode == "thrust":  # GameEnv.step: flat (L, R) thrust pairs (RR_EnvBase.py:269-273)
            if len(arr) > self.preset.nr * 2:
                raise Exception(f"{len(arr)} commands but only {self.preset.nr * 2} robot engines.")
            obs, rew, done, info = self._b.step_thrust(torch.as_tensor(arr.astype(np.float32)).view(1, -1))
        else:
            if len(arr) > self.preset.nr:
                raise Exception(f"{len(arr)} commands but only {self.preset.nr} robots.")
            a = torch.as_tensor(arr.astype(np.int64)).view(1, -1)
            obs, rew, done, info = self._b.step_f64(a) if self._f64 else self._b.step(a)
        st = int(info.status[0]) & STATUS_FLAG_MASK
        for bit, msg in STATUS_BITS.items():
            if st & bit:
                raise ZeroDivisionError(msg) if bit == 32 else Exception(msg)
        g = info.adblGrumpyState[0].double().cpu().numpy() if info.adblGrumpyState is not None else None
        return (obs[0].double().cpu().numpy(), float(rew[0]), bool(done[0]),
                DebugInfo(g, float(info.dblGrumpyScore[0]), st))

    def get_game_state(self, int_team=None, obj_robot=None, obj_ball=None):
        o = self._b.get_game_state(int_team, -1 if obj_robot is None else int(obj_robot),
                                   -1 if obj_ball is None else int(obj_ball), f64=self._f64)
        return None if o is None else o[0].double().cpu().numpy()

    def render(self, mode="human"):
        return self._b.render(mode)

    def seed(self, seed=None):
        return [seed]

    def close(self):
        self._b.close()


def make(env_id="RoboRugbySimpleDuel-v3", num_envs=None, preset="T", **kw):
    """gym.make look-alike (robo_rugby/__init__.py:4-34).  num_envs=None -> reference-shaped single env."""
    if env_id not in ENV_IDS:
        raise KeyError(f"unknown env id {env_id!r}; registered and constructible in the reference: {list(ENV_IDS)}")
    if num_envs is None:
        return RoboRugbyEnv(preset=preset, **kw)
    return BatchedRoboRugbyEnv(num_envs, preset=preset, env_id=env_id, **kw)
