"""ctypes binding of the C-ABI in include/roborugby_amd.h.

There is NO CPU fallback: if the HIP library is missing or cannot be loaded this module raises."""
import ctypes as C
import os

# PyTorch-ROCm bundles its own libamdhip64; it must be the HIP runtime this process loads FIRST so that the
# library below (linked against the same soname) shares it -- device pointers and streams handed across the
# C-ABI are only meaningful inside one runtime instance.
import torch  # noqa: F401  (import order matters)

HERE = os.path.dirname(os.path.abspath(__file__))
# RR_LIB_PATH lets tools/ A/B-test alternative builds of the same ABI (kernel tuning); default = the in-tree build
LIB_PATH = os.environ.get("RR_LIB_PATH", os.path.join(HERE, "libroborugby_amd.so"))
LIB_PATH_EXACT = os.path.join(HERE, "libroborugby_amd_exact.so")  # the exact-trig parity build (build.py: -DRR_EXACT_TRIG=1)


class RRConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("num_envs", C.c_int32),
        ("nr_happy", C.c_int32), ("nr_grumpy", C.c_int32), ("nb_pos", C.c_int32), ("nb_neg", C.c_int32),
        ("arena_w", C.c_double), ("arena_h", C.c_double),
        ("game_len_steps", C.c_int32), ("game_mode", C.c_int32), ("time_limit", C.c_int32), ("auto_reset", C.c_int32),
        ("reset_on_fault", C.c_int32),
        ("dtype", C.c_int32), ("device", C.c_int32),
        ("seed", C.c_uint64), ("arena_offset", C.c_uint64),
        ("step_budget_clocks", C.c_uint32), ("reserved_", C.c_uint32),
    ]


class RRDqnArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("batch", C.c_int32),
        ("eval_params", C.c_void_p * 6), ("target_params", C.c_void_p * 6),
        ("state_memory", C.c_void_p), ("new_state_memory", C.c_void_p), ("action_memory", C.c_void_p),
        ("reward_memory", C.c_void_p), ("terminal_memory", C.c_void_p), ("batch_index", C.c_void_p),
        ("gamma", C.c_float), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("loss_out", C.c_void_p),
    ]


class RRSacTargetsArgs(C.Structure):
    """rr_sac_targets_args (include/roborugby_amd.h)"""
    _fields_ = [
        ("struct_size", C.c_int32), ("batch", C.c_int32), ("n_actions", C.c_int32), ("flags", C.c_int32),
        ("actor", C.c_void_p * 8), ("critic_1", C.c_void_p * 6), ("critic_2", C.c_void_p * 6), ("target_value", C.c_void_p * 6),
        ("state_memory", C.c_void_p), ("new_state_memory", C.c_void_p), ("action_memory", C.c_void_p), ("reward_memory", C.c_void_p),
        ("terminal_memory", C.c_void_p), ("mem_rows", C.c_int64), ("batch_index", C.c_void_p), ("noise", C.c_void_p),
        ("max_action", C.c_float), ("gamma", C.c_float), ("reward_scale", C.c_float),
        ("seed", C.c_uint64), ("call", C.c_uint32),
        ("value_target", C.c_void_p), ("q_hat", C.c_void_p), ("state", C.c_void_p), ("action", C.c_void_p),
        ("policy_action", C.c_void_p), ("log_prob", C.c_void_p), ("head", C.c_void_p), ("noise_out", C.c_void_p),
        ("q1", C.c_void_p), ("q2", C.c_void_p), ("v_next", C.c_void_p),
    ]


class RRSacGradsArgs(C.Structure):
    """rr_sac_grads_args (include/roborugby_amd.h)"""
    _fields_ = [
        ("struct_size", C.c_int32), ("batch", C.c_int32), ("n_actions", C.c_int32), ("flags", C.c_int32),
        ("value", C.c_void_p * 6), ("critic_1", C.c_void_p * 6), ("critic_2", C.c_void_p * 6),
        ("state", C.c_void_p), ("action", C.c_void_p), ("value_target", C.c_void_p), ("q_hat", C.c_void_p),
        ("grad_value", C.c_void_p * 6), ("grad_critic_1", C.c_void_p * 6), ("grad_critic_2", C.c_void_p * 6),
        ("loss", C.c_void_p),
    ]


# name -> (restype, argtypes); every symbol include/roborugby_amd.h declares
_vp = C.c_void_p
SYMBOLS = {
    "rr_abi_version": (C.c_int, []),
    "rr_last_error": (C.c_char_p, []),
    "rr_exact_trig": (C.c_int, []),
    "rr_create": (C.c_int, [C.POINTER(RRConfig), C.POINTER(_vp)]),
    "rr_destroy": (C.c_int, [_vp]),
    "rr_reset": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "rr_step": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_step_f64": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_set_step_budget": (C.c_int, [_vp, C.c_uint32]),
    "rr_step_thrust": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_step_thrust_f64": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_rollout": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_observe": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    "rr_observe_f64": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    "rr_set_reward_program": (C.c_int, [_vp, _vp, C.c_int32]),
    "rr_observe_kind": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp]),
    "rr_observe_kind_f64": (C.c_int, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp]),
    "rr_hive_observe": (C.c_int, [_vp, C.c_uint32, C.c_int32, _vp, _vp, _vp]),
    "rr_hive_observe_f64": (C.c_int, [_vp, C.c_uint32, C.c_int32, _vp, _vp, _vp]),
    "rr_hive_transition": (C.c_int, [_vp, C.c_uint32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_hive_transition_f64": (C.c_int, [_vp, C.c_uint32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_hive_observe_held": (C.c_int, [_vp, C.c_uint32, C.c_int32, _vp, _vp, _vp, _vp]),
    "rr_hive_observe_held_f64": (C.c_int, [_vp, C.c_uint32, C.c_int32, _vp, _vp, _vp, _vp]),
    "rr_hive_commit": (C.c_int, [_vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_hive_transition_held": (C.c_int, [_vp, C.c_uint32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_hive_transition_held_f64": (C.c_int, [_vp, C.c_uint32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_render": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]),
    "rr_render_ego": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, _vp, _vp]),
    "rr_track_prior_step": (C.c_int, [_vp, C.c_int32, _vp]),
    "rr_set_goal_scoring": (C.c_int, [_vp, C.c_int32, _vp]),
    "rr_goal_scores": (C.c_int, [_vp, _vp, _vp]),
    "rr_set_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_get_state": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_set_poses": (C.c_int, [_vp, _vp, _vp, _vp]),
    "rr_reset_to_poses": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_get_scratch_rect": (C.c_int, [_vp, _vp, _vp]),
    "rr_set_scratch_rect": (C.c_int, [_vp, _vp, _vp]),
    "rr_get_episode_state": (C.c_int, [_vp, _vp, _vp, _vp]),
    "rr_set_episode_state": (C.c_int, [_vp, _vp, _vp, _vp]),
    "rr_episode_stats": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_policy_chase": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_float, C.c_uint64, _vp, C.c_int32, _vp]),
    "rr_dqn_create": (C.c_int, [C.c_int32, C.POINTER(_vp)]),
    "rr_dqn_destroy": (C.c_int, [_vp]),
    "rr_dqn_last_error": (C.c_char_p, []),
    "rr_dqn_update": (C.c_int, [_vp, C.POINTER(RRDqnArgs), _vp]),
    "rr_dqn_grads": (C.c_int, [_vp, C.POINTER(RRDqnArgs), _vp, _vp]),
    "rr_dqn_param_count": (C.c_int32, []),
    "rr_dqn_store": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_dqn_act": (C.c_int, [_vp, C.POINTER(_vp * 6), _vp, C.c_int32, C.c_float, C.c_uint64, C.c_uint32, _vp, _vp, _vp]),
    "rr_cnn_act": (C.c_int, [_vp, C.POINTER(_vp * 8), _vp, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_uint32, _vp, _vp, _vp]),
    "rr_sac_act": (C.c_int, [_vp, C.POINTER(_vp * 8), _vp, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "rr_sac_targets": (C.c_int, [_vp, C.POINTER(RRSacTargetsArgs), _vp]),
    "rr_sac_grads": (C.c_int, [_vp, C.POINTER(RRSacGradsArgs), _vp]),
    "rr_frames_push": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_frames_sample": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _vp, C.c_uint64,
                                   C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rr_dqn_adam_state":(C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_int64), C.c_int32, _vp]),
    "rr_probe_hbm_copy": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "rr_state_bytes_per_env": (C.c_int, [_vp, C.POINTER(C.c_int64)]),
    "rr_lanes_per_env": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
}

RR_SAC_DETERMINISTIC = 1  # rr_sac_act's flag (include/roborugby_amd.h)

_lib = None
_lib_exact = None


def load(exact=False):
    """Loads libroborugby_amd.so (built by roborugby_amd.build / __graft_entry__.build); exact=True: the exact-trig parity build
    libroborugby_amd_exact.so (same ABI, same sources, -DRR_EXACT_TRIG=1)."""
    global _lib, _lib_exact
    if exact:
        if _lib_exact is None:
            _lib_exact = _load_path(LIB_PATH_EXACT, True)
        return _lib_exact
    if _lib is None:
        _lib = _load_path(LIB_PATH, False)
    return _lib


_shape_libs = {}


def load_shape(counts, exact=False):
    """The one-shape library of entity counts outside the built list (build.build_shape_library), compiled on demand when it is missing
    or older than its sources -- hipcc has to be there for that; the same ABI, no fallback of any kind."""
    from . import build as _build
    key = (tuple(int(c) for c in counts), bool(exact))
    _build.shape_lanes(*key[0], exact=key[1])  # ValueError for counts this build of the kernel refuses: nothing to compile
    if key not in _shape_libs:
        path = _build.shape_lib_path(*key[0], exact=exact)
        if _build.shape_is_stale(*key[0], exact=exact) and (_build.sources_present() or not os.path.exists(path)):
            try:
                _build.build_shape_library(*key[0], verbose=True, exact=exact)
            except Exception as exc:
                raise ImportError(f"{path}: no library for {key[0][0]}+{key[0][1]} robots / {key[0][2]}+{key[0][3]} balls and it could not be "
                                  f"built ({exc}): `python -m roborugby_amd.build --shape={','.join(map(str, key[0]))}` needs hipcc") from exc
        _shape_libs[key] = _bind(C.CDLL(path), exact, False, path)
    return _shape_libs[key]


def _bind(lib, exact, overridden, path):
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    assert lib.rr_exact_trig() == (1 if exact else 0) or overridden, path
    return lib


def _load_path(path, exact):
    from . import build as _build
    overridden = not exact and "RR_LIB_PATH" in os.environ
    stale = not overridden and os.path.exists(path) and _build.sources_present() and _build.is_stale(exact)
    if not os.path.exists(path) or stale:
        # not a fallback: the only thing ever loaded is the HIP library, (re)built here if the in-tree .so is absent or
        # older than its sources (an edited rr_sim.hpp must never be tested against yesterday's kernels)
        try:
            if overridden:
                raise RuntimeError("RR_LIB_PATH points to a missing file")
            _build.build_hip_library(verbose=True, exact=exact)
        except Exception as exc:
            if stale:
                raise ImportError(f"{path} is older than its sources and could not be rebuilt ({exc})") from exc
            raise ImportError(
                f"{path} is missing and could not be built ({exc}): run `python -m roborugby_amd.build`. "
                "roborugby_amd has no CPU fallback.") from exc
    return _bind(C.CDLL(path), exact, overridden, path)


class RRError(RuntimeError):
    pass


def check(rc, what, lib=None, err_fn="rr_last_error"):
    """Raises RRError with the message of the library that returned `rc` (`lib`; the env passes its own -- the default and the
    parity library keep separate thread-local strings).  `err_fn`: the entry point that holds the message."""
    if rc != 0:
        libs = [lib] if lib is not None else [x for x in (_lib, _lib_exact) if x is not None] or [load()]
        msg = b"; ".join(m for m in (getattr(x, err_fn)() for x in libs) if m)
        raise RRError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")


def ptr(t, offset=0):
    """a tensor's (or None's) device pointer as the C-ABI takes it, `offset` bytes in: c_void_p, or None"""
    return C.c_void_p(t.data_ptr() + offset) if t is not None else None


def current_stream(device):
    """the device's current torch stream, as the C-ABI takes it"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _Handle:
    """Owner of one C-ABI handle: `lib` the library it lives in, `h` the handle (None once closed), `device` the torch device its launches
    go to.  A subclass names the entry that destroys the handle and the one that holds its library's error message."""
    DESTROY = ERR = None

    def __init__(self, lib, h, device):
        self.lib, self.h, self.device = lib, h, device

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            getattr(self.lib, self.DESTROY)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self):
        """the device's current torch stream, as the C-ABI takes it"""
        return current_stream(self.device)

    def call(self, name, *args):
        """lib.<name>(handle, *args); an RRError that names <name> and carries the library's message unless it returns 0"""
        rc = getattr(self.lib, name)(self.h, *args)
        if rc:
            check(rc, name, self.lib, self.ERR)

    def launch(self, name, *args):
        """call() with the device's current stream appended: the entries that enqueue work take it last"""
        rc = getattr(self.lib, name)(self.h, *args, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc:
            check(rc, name, self.lib, self.ERR)


class EnvHandle(_Handle):
    """Owner of one env handle (rr_create .. rr_destroy): the arenas' records on the device.  EnvHandle(lib, h, device) adopts a handle
    that exists; create() makes one."""
    DESTROY, ERR = "rr_destroy", "rr_last_error"

    @classmethod
    def create(cls, lib, cfg, device):
        h = C.c_void_p()
        check(lib.rr_create(C.byref(cfg), C.byref(h)), "rr_create", lib)
        return cls(lib, h, device)


class DqnHandle(_Handle):
    """Owner of one rr_dqn handle (rr_dqn_create .. rr_dqn_destroy): the per-workgroup partial gradients and the Adam moments of the fused
    learn step, ~73 MB of device memory.  The rr_dqn_* calls write their messages to rr_dqn_last_error."""
    DESTROY, ERR = "rr_dqn_destroy", "rr_dqn_last_error"

    def __init__(self, device):
        lib, h = load(), C.c_void_p()
        check(lib.rr_dqn_create(device.index or 0, C.byref(h)), "rr_dqn_create", lib, self.ERR)
        super().__init__(lib, h, device)

    def act(self, params, obs, n, epsilon, seed, calls, actions, q=None, stream=None):
        """rr_dqn_act on the 11-256-256-8 network `params` (its six tensors): epsilon-greedy int32 actions for the n rows of `obs`, the
        draws keyed by (seed, row, the low 32 bits of `calls`); q: optionally the float32 [n, 8] Q-values it acted on."""
        ptrs = (C.c_void_p * 6)(*[p.data_ptr() for p in params])
        self.call("rr_dqn_act", C.byref(ptrs), ptr(obs), n, float(min(max(epsilon, 0.0), 1.0)), int(seed), calls & 0xFFFFFFFF, ptr(actions),
                  ptr(q), self.stream() if stream is None else stream)

    def sac_act(self, params, obs, n, n_actions, max_action, seed, calls, actions, deterministic=False, log_prob=None, head=None, noise=None):
        """rr_sac_act on the actor `params` (its eight tensors): float32 [n, n_actions] squashed samples for the n rows of `obs`, the draws
        keyed by (seed, row, the low 32 bits of `calls`); log_prob [n], head [n, 2 n_actions], noise [n, n_actions]: optionally written."""
        ptrs = (C.c_void_p * 8)(*[p.data_ptr() for p in params])
        self.launch("rr_sac_act", C.byref(ptrs), ptr(obs), n, n_actions, float(max_action), RR_SAC_DETERMINISTIC if deterministic else 0,
                    int(seed) & 0xFFFFFFFFFFFFFFFF, calls & 0xFFFFFFFF, ptr(actions), ptr(log_prob), ptr(head), ptr(noise))

    def sac_targets(self, actor, critic_1, critic_2, target_value, rings, mem_rows, batch, n_actions, max_action, gamma, reward_scale,
                    value_target, q_hat, batch_index=None, noise=None, seed=0, calls=0, state=None, action=None, **windows):
        """rr_sac_targets: the no-grad half of the SAC learn step in one launch.  actor (eight tensors, rr_sac_act's order), critic_1,
        critic_2, target_value (six each); rings = (state_memory, new_state_memory, action_memory, reward_memory, terminal_memory) of
        which rows 0 .. mem_rows-1 may be addressed; batch_index int64 [batch] (None: rows 0 .. batch-1); noise [batch, n_actions] (None:
        the kernel draws under (seed, the low 32 bits of `calls`)).  Written: value_target, q_hat [batch]; optionally the gathered state
        [batch, 11] / action [batch, n_actions] and the windows policy_action, log_prob, head, noise_out, q1, q2, v_next (keywords)."""
        a = RRSacTargetsArgs()
        a.struct_size, a.batch, a.n_actions, a.flags = C.sizeof(RRSacTargetsArgs), int(batch), int(n_actions), 0
        for field, params in (("actor", actor), ("critic_1", critic_1), ("critic_2", critic_2), ("target_value", target_value)):
            arr = getattr(a, field)
            if len(params) != len(arr):
                raise ValueError(f"sac_targets: {field} takes {len(arr)} tensors, got {len(params)}")
            for k, p in enumerate(params):
                arr[k] = p.data_ptr()
        (a.state_memory, a.new_state_memory, a.action_memory, a.reward_memory, a.terminal_memory) = (t.data_ptr() for t in rings)
        a.mem_rows = int(mem_rows)
        a.batch_index, a.noise = ptr(batch_index), ptr(noise)
        a.max_action, a.gamma, a.reward_scale = float(max_action), float(gamma), float(reward_scale)
        a.seed, a.call = int(seed) & 0xFFFFFFFFFFFFFFFF, int(calls) & 0xFFFFFFFF
        a.value_target, a.q_hat, a.state, a.action = ptr(value_target), ptr(q_hat), ptr(state), ptr(action)
        for k in ("policy_action", "log_prob", "head", "noise_out", "q1", "q2", "v_next"):
            setattr(a, k, ptr(windows.pop(k, None)))
        if windows:
            raise TypeError(f"sac_targets: unknown windows {sorted(windows)}")
        self.launch("rr_sac_targets", C.byref(a))

    def sac_grads(self, value, critic_1, critic_2, state, action, value_target, q_hat, batch, n_actions, grad_value, grad_critic_1,
                  grad_critic_2, loss):
        """rr_sac_grads: the gradients of the SAC value loss and critic loss in one fused launch (plus its reduce).  value, critic_1,
        critic_2: six tensors each (rr_sac_targets' order); state [batch, 11], action [batch, n_actions], value_target, q_hat [batch]:
        dense float32.  Written: grad_value, grad_critic_1, grad_critic_2 (six tensors each, the parameters' shapes) and loss [3] =
        0.5 * mse of the value net, critic_1 and critic_2."""
        a = RRSacGradsArgs()
        a.struct_size, a.batch, a.n_actions, a.flags = C.sizeof(RRSacGradsArgs), int(batch), int(n_actions), 0
        for field, tensors in (("value", value), ("critic_1", critic_1), ("critic_2", critic_2), ("grad_value", grad_value),
                               ("grad_critic_1", grad_critic_1), ("grad_critic_2", grad_critic_2)):
            arr = getattr(a, field)
            if len(tensors) != len(arr):
                raise ValueError(f"sac_grads: {field} takes {len(arr)} tensors, got {len(tensors)}")
            for k, p in enumerate(tensors):
                arr[k] = p.data_ptr()
        a.state, a.action, a.value_target, a.q_hat, a.loss = ptr(state), ptr(action), ptr(value_target), ptr(q_hat), ptr(loss)
        self.launch("rr_sac_grads", C.byref(a))
