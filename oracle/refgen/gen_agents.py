#!/usr/bin/env python3
"""Agent fixtures from the reference trainers' own programs -- TEST INFRASTRUCTURE ONLY (needs the reference tree).

Imports Training_SAC_pytorch.py and Training_DQN_pytorch.py *unmodified*, by path, under gen_golden.py's stand-ins (robo_rugby, gym and
pygame through load_reference("G"); `gym.wrappers`, `matplotlib` and `imageio`, which only the trainers' import lines and `__main__`
blocks name, as empty modules) and writes three fixtures into tests/golden/ (or RR_GOLDEN_OUT):

  sac_learn.npz   Agent.learn (Training_SAC_pytorch.py:322-388) once per case, its five networks replaced by the reference's own
                  ActorNetwork / CriticNetwork / ValueNetwork at fc1_dims = fc2_dims = 32: the gradients left in .grad, the losses,
                  the parameters after the call
  sac_act.npz     ActorNetwork.sample_normal(state, reparameterize=False) (:207-234) at the real width 256
  dqn_learn.npz   DQNAgent.learn (Training_DQN_pytorch.py:151-191) once, 11-256-256-8: the gradient of Q_eval

What is substituted in the reference, and nothing else:
  * the normal draws are FED IN.  The SAC module's name `Normal` is bound to FedNormal below: log_prob is torch.distributions.Normal's,
    sample() is loc + scale * z under no_grad and rsample() is loc + scale * z, with z taken from the fixture instead of torch's
    generator;
  * the batch rows: np.random.choice answers "rows 0 .. batch-1" while learn() runs;
  * torch.cuda.is_available answers False (the CPU only, one thread).
Weights, batches, observations and draws come from seeded numpy generators and are stored in the fixtures; torch's initialisation
enters nothing.

Every case runs twice from identical copies: the reference as it stands (float32), and in float64 -- every network through .double(),
and torch.float (SAC: dtype=T.float) and torch.Tensor.float (DQN: state.float()) rebound to their float64 counterparts for the
duration of that one call, restored in a finally.  The float64 run is the truth that is recorded; E is the largest absolute difference
per tensor between the two runs: the reference's own float32 error, the yardstick of the tests' bars.  (Where sigma is clamped to 1e-6
the float32 run's gradient of mu.weight / mu.bias is about 1 % of its scale off: +-(x - mu) / sigma^2 terms of size 1e6 cancel inside
Normal.log_prob's backward.  Hence the float64 run.)

The learn fixtures' batch rows are chosen from a larger seeded pool so that none sits on a knife edge in the float64 run: no hidden
pre-activation, no raw sigma output at a clamp bound and no q1 - q2 of a policy action within MARGIN of the point where a derivative
jumps (there a gradient entry depends on the last bits of a float32 sum, whoever computes it).

usage:  python oracle/refgen/gen_agents.py [sac_learn] [sac_act] [dqn_learn]      (default: all three, in this one fresh process)
"""
import contextlib
import importlib.util
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
GOLD = os.environ.get("RR_GOLDEN_OUT") or os.path.join(REPO, "tests", "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
import sac_ref  # noqa: E402  repository code: the float32 restatement of rr_sac_act's draw is an INPUT of sac_act.npz

MARGIN = 1e-4           # knife-edge distance kept by the learn fixtures' rows (float64 run)
WELL = 1e-3             # an entry is well-conditioned for Adam's first step when |g| >= WELL * max |g| of its tensor
SAC_NETS = ("actor", "critic_1", "critic_2", "value", "target_value")
META = {
    "generator": "oracle/refgen/gen_agents.py",
    "reference": "harman097/RoboRugby: Training_SAC_pytorch.py, Training_DQN_pytorch.py (unmodified, imported by path under stand-ins)",
    "substitutions": [
        "Normal in the SAC module -> FedNormal: log_prob delegates to torch.distributions.Normal; the standard normal draw z is fed in: "
        "sample() = (loc + scale * z) under no_grad, rsample() = loc + scale * z",
        "np.random.choice -> rows 0 .. batch-1 while learn() runs",
        "torch.cuda.is_available -> False; torch.set_num_threads(1)",
        "float64 run only: networks .double(); torch.float -> torch.float64, torch.Tensor.float -> torch.Tensor.double during the call",
        "gym.wrappers, matplotlib(.pyplot), imageio: empty modules (only import lines and __main__ blocks name them)",
    ],
    "E": "largest |float32 run - float64 run| per tensor: the reference's own float32 error",
    "margin": MARGIN, "well_conditioned": f"|g64| >= {WELL} * max |g64| of the tensor",
}


# ------------------------------------------------------------------ the reference, and the three substitutions
def load_trainers():
    torch.set_num_threads(1)
    torch.cuda.is_available = lambda: False
    from load_reference import REF_ROOT, load_reference
    load_reference("G")
    gym = sys.modules["gym"]
    if not hasattr(gym, "wrappers"):
        gym.wrappers = sys.modules["gym.wrappers"] = types.ModuleType("gym.wrappers")
    for name in ("matplotlib", "matplotlib.pyplot", "imageio"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    if not hasattr(np, "bool"):  # (numpy 1.24 .. 1.26 dropped the alias the trainers' replay constructors name)
        np.bool = np.bool_
    mods = []
    for name in ("Training_SAC_pytorch", "Training_DQN_pytorch"):
        spec = importlib.util.spec_from_file_location("rr_reference_" + name, os.path.join(REF_ROOT, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    mods[0].Normal = FedNormal
    return mods


class FedNormal:
    """torch.distributions.Normal with the standard normal draw fed in (FedNormal.feed: consumed front to back, one tensor per draw)"""
    feed = []

    def __init__(self, loc, scale):
        self.loc, self.scale = loc, scale
        self._normal = torch.distributions.Normal(loc, scale)

    def _z(self):
        return FedNormal.feed.pop(0).to(self.loc.dtype)

    def sample(self):
        with torch.no_grad():
            return self.loc + self.scale * self._z()

    def rsample(self):
        return self.loc + self.scale * self._z()

    def log_prob(self, value):
        return self._normal.log_prob(value)


@contextlib.contextmanager
def as_float64():
    old = torch.float, torch.Tensor.float
    torch.float, torch.Tensor.float = torch.float64, torch.Tensor.double
    try:
        yield
    finally:
        torch.float, torch.Tensor.float = old


@contextlib.contextmanager
def first_rows():
    old = np.random.choice
    np.random.choice = lambda a, size=None, replace=True, p=None: np.arange(size)
    try:
        yield
    finally:
        np.random.choice = old


@contextlib.contextmanager
def locals_at_return(code, names, out):
    """out[name] = the value of that local when the function whose code object is `code` returns"""
    def prof(frame, event, arg):
        if event == "return" and frame.f_code is code:
            out.update({k: frame.f_locals[k] for k in names if k in frame.f_locals})
    sys.setprofile(prof)
    try:
        yield
    finally:
        sys.setprofile(None)


class Watch:
    """forward hooks on the nets' Linear layers: per call, each row's distance from a knife edge (fc1 / fc2: |pre-activation|; sigma: the
    distance of the raw output from both clamp bounds), and the outputs of the layers named in `keep`"""

    def __init__(self, nets, keep=()):
        self.rows, self.kept, self.handles = [], {}, []
        for net_name, net in nets.items():
            for name, layer in net.named_children():
                if name in ("fc1", "fc2", "sigma") or (net_name, name) in keep:
                    self.handles.append(layer.register_forward_hook(self._hook(net_name, name, (net_name, name) in keep)))

    def _hook(self, net_name, name, keep):
        def hook(module, args, out):
            o = out.detach().double()
            if name == "sigma":
                self.rows.append(torch.minimum((o - sac_ref.SIGMA_MIN).abs(), (o - sac_ref.SIGMA_MAX).abs()).min(1)[0])
            elif name in ("fc1", "fc2"):
                self.rows.append(o.abs().min(1)[0])
            if keep:
                self.kept.setdefault((net_name, name), []).append(o.clone())
        return hook

    def add(self, per_row):
        self.rows.append(per_row.detach().double().view(-1))

    def margin(self):
        return torch.stack(self.rows).min(0)[0]

    def close(self):
        for h in self.handles:
            h.remove()


def linear(rng, n_out, n_in, scale=1.0, grid=None):
    """torch.nn.Linear's initial ranges from the numpy generator; grid: round to multiples of it (compressible, exact in float32)"""
    b = 1.0 / math.sqrt(n_in)
    w, bias = rng.uniform(-b, b, (n_out, n_in)) * scale, rng.uniform(-b, b, n_out) * scale
    if grid:
        w, bias = np.round(w / grid) * grid, np.round(bias / grid) * grid
    return w.astype(np.float32), bias.astype(np.float32)


def mlp(rng, n_in, width, heads, grid=None):
    sd = {}
    for name, (n_out, k) in (("fc1", (width, n_in)), ("fc2", (width, width))) + tuple((h, (n, width)) for h, n in heads):
        sd[name + ".weight"], sd[name + ".bias"] = linear(rng, n_out, k, grid=grid)
    return sd


def aim_sigma(actor_sd, obs, mean, std):
    """scales and shifts the sigma head so that every raw sigma output has this mean and standard deviation over the rows of obs"""
    params = [actor_sd[k] for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "mu.weight", "mu.bias", "sigma.weight", "sigma.bias")]
    A = params[4].shape[0]
    params[7] = np.zeros(A, np.float32)
    raw = sac_ref.actor_head64(params, obs)[:, A:]
    gain = std / raw.std(0)
    actor_sd["sigma.weight"] = (actor_sd["sigma.weight"] * gain[:, None]).astype(np.float32)
    actor_sd["sigma.bias"] = (mean - raw.mean(0) * gain).astype(np.float32)


def load(net, sd, double):
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return net.double() if double else net


def grads(net):
    return {k: p.grad.detach().double().numpy().copy() for k, p in net.named_parameters()}


def params(net):
    return {k: p.detach().double().numpy().copy() for k, p in net.named_parameters()}


def save(name, out, meta):
    os.makedirs(GOLD, exist_ok=True)
    out["meta"] = np.array(json.dumps(dict(META, python=sys.version.split()[0], torch=torch.__version__.split("+")[0], **meta)))
    path = os.path.join(GOLD, name)
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes", flush=True)


# ------------------------------------------------------------------ sac_learn.npz
SAC_LEARN_CASES = (  # (name, A, mean and std aimed at for the raw sigma outputs, seed)
    ("A2_inside", 2, 0.5, 0.08, 101), ("A4_inside", 4, 0.5, 0.08, 102), ("A2_above", 2, 0.8, 0.13, 103), ("A4_both", 4, 0.5, 1.0, 104))
SAC_HP = dict(alpha=3e-4, beta=1e-4, gamma=0.99, tau=0.005, reward_scale=2.0, batch=64, width=32, pool=256)
# (alpha differs from beta, unlike the reference's defaults, so that the step shows which optimizer owns which network)


def sac_agent(S, A, nets_sd, double):
    hp = SAC_HP
    env = types.SimpleNamespace(action_space=types.SimpleNamespace(high=np.ones(A, np.float32)))
    agent = S.Agent(alpha=hp["alpha"], beta=hp["beta"], input_dims=[11], env=env, gamma=hp["gamma"], n_actions=A, max_size=hp["batch"],
                    tau=hp["tau"], batch_size=hp["batch"], reward_scale=hp["reward_scale"])
    w = hp["width"]
    agent.actor = S.ActorNetwork(hp["alpha"], [11], max_action=env.action_space.high, fc1_dims=w, fc2_dims=w, n_actions=A)
    agent.critic_1 = S.CriticNetwork(hp["beta"], [11], n_actions=A, fc1_dims=w, fc2_dims=w, name="critic_1")
    agent.critic_2 = S.CriticNetwork(hp["beta"], [11], n_actions=A, fc1_dims=w, fc2_dims=w, name="critic_2")
    agent.value = S.ValueNetwork(hp["beta"], [11], fc1_dims=w, fc2_dims=w, name="value")
    agent.target_value = S.ValueNetwork(hp["beta"], [11], fc1_dims=w, fc2_dims=w, name="target_value")
    for k in SAC_NETS:
        load(getattr(agent, k), nets_sd[k], double)
    return agent


def sac_pool_margin(S, A, nets_sd, pool):
    """each pool row's distance from a knife edge in a float64 forward of everything learn() evaluates on it"""
    agent = sac_agent(S, A, nets_sd, True)
    watch = Watch({k: getattr(agent, k) for k in SAC_NETS})
    t = lambda a: torch.from_numpy(a).double()
    state, action, state_ = t(pool["state"]), t(pool["action"]), t(pool["new_state"])
    with torch.no_grad():
        agent.value(state), agent.target_value(state_)
        agent.critic_1(state, action), agent.critic_2(state, action)
        FedNormal.feed = [t(pool["noise_value"]), t(pool["noise_actor"])]
        for reparameterize in (False, True):
            a, _ = agent.actor.sample_normal(state, reparameterize=reparameterize)
            watch.add((agent.critic_1(state, a) - agent.critic_2(state, a)).abs())
    watch.close()
    return watch.margin().numpy()


def sac_learn_run(S, A, nets_sd, batch, double):
    agent = sac_agent(S, A, nets_sd, double)
    for i in range(SAC_HP["batch"]):
        agent.remember(batch["state"][i], batch["action"][i], batch["reward"][i], batch["new_state"][i], bool(batch["done"][i]))
    nets = {k: getattr(agent, k) for k in SAC_NETS}
    watch = Watch(nets, keep=(("actor", "sigma"),))
    FedNormal.feed = [torch.from_numpy(batch["noise_value"]), torch.from_numpy(batch["noise_actor"])]
    got = {}
    with first_rows(), locals_at_return(S.Agent.learn.__code__, ("value_loss", "actor_loss", "critic_loss", "q1_new_policy", "q2_new_policy"), got):
        if double:
            with as_float64():
                agent.learn()
        else:
            agent.learn()
    watch.close()
    assert not FedNormal.feed and torch.float is torch.float32
    want = torch.float64 if double else torch.float32
    assert all(p.dtype == want and p.grad.dtype == want for net in nets.values() for p in net.parameters())
    assert got["value_loss"].dtype == want
    watch.add((got["q1_new_policy"] - got["q2_new_policy"]).abs())
    return dict(grads={k: grads(nets[k]) for k in SAC_NETS[:4]}, after={k: params(nets[k]) for k in SAC_NETS},
                losses=np.array([float(got[k].detach()) for k in ("value_loss", "actor_loss", "critic_loss")]),
                raw_sigma=watch.kept[("actor", "sigma")][0].numpy(), margin=float(watch.margin().min()))


def gen_sac_learn(S):
    out, meta_cases, hp = {}, {}, SAC_HP
    for name, A, mean, std, seed in SAC_LEARN_CASES:
        rng = np.random.default_rng(seed)
        f, w, P = np.float32, hp["width"], hp["pool"]
        nets_sd = dict(actor=mlp(rng, 11, w, (("mu", A), ("sigma", A))), critic_1=mlp(rng, 11 + A, w, (("q", 1),)),
                       critic_2=mlp(rng, 11 + A, w, (("q", 1),)), value=mlp(rng, 11, w, (("v", 1),)))
        nets_sd["target_value"] = {k: (v + 0.02 * rng.standard_normal(v.shape)).astype(f) for k, v in nets_sd["value"].items()}
        state = rng.uniform(-1.0, 1.0, (P, 11)).astype(f)
        pool = dict(state=state, new_state=(state + 0.1 * rng.standard_normal((P, 11))).astype(f), action=rng.uniform(-1.0, 1.0, (P, A)).astype(f),
                    reward=(2.0 * rng.standard_normal(P)).astype(f), noise_value=rng.standard_normal((P, A)).astype(f),
                    noise_actor=rng.standard_normal((P, A)).astype(f))
        aim_sigma(nets_sd["actor"], state, mean, std)
        rows = np.nonzero(sac_pool_margin(S, A, nets_sd, pool) > MARGIN)[0][:hp["batch"]]
        assert len(rows) == hp["batch"], (name, len(rows))
        batch = {k: v[rows] for k, v in pool.items()}
        batch["done"] = np.arange(hp["batch"]) % 5 == 4  # every fifth row is terminal
        r32, r64 = sac_learn_run(S, A, nets_sd, batch, False), sac_learn_run(S, A, nets_sd, batch, True)
        raw = r64["raw_sigma"]
        lo, hi = raw < sac_ref.SIGMA_MIN, raw > sac_ref.SIGMA_MAX
        if name.endswith("inside"):
            assert not lo.any() and not hi.any() and raw.min() > sac_ref.SIGMA_MIN and raw.max() < sac_ref.SIGMA_MAX, name
        elif name.endswith("above"):
            assert hi.any() and not lo.any() and not hi.all(), name
        else:
            assert hi.sum() >= 8 and lo.sum() >= 8 and (~lo & ~hi).sum() >= 8, name
        assert r64["margin"] > MARGIN, (name, r64["margin"])
        shares = {}
        for net in SAC_NETS[:4]:
            for k, g in r64["grads"][net].items():
                out[f"{name}.g64.{net}.{k}"] = g
                out[f"{name}.E.{net}.{k}"] = np.float64(np.abs(r32["grads"][net][k] - g).max())
                shares[f"{net}.{k}"] = round(float((np.abs(g) >= WELL * np.abs(g).max()).mean()), 4)
                assert np.abs(g).max() > 0 and shares[f"{net}.{k}"] >= 0.70, (name, net, k, shares[f"{net}.{k}"])
        for net in SAC_NETS:
            for k, v in nets_sd[net].items():
                out[f"{name}.w.{net}.{k}"] = v
                out[f"{name}.after.{net}.{k}"] = r64["after"][net][k]
        for k, v in batch.items():
            out[f"{name}.{k}"] = v
        out[f"{name}.losses64"], out[f"{name}.E_losses"] = r64["losses"], np.abs(r32["losses"] - r64["losses"])
        out[f"{name}.raw_sigma64"] = raw
        meta_cases[name] = dict(n_actions=A, seed=seed, sigma_below=int(lo.sum()), sigma_above=int(hi.sum()), margin=r64["margin"],
                                well_conditioned_share=shares, smallest_share=min(shares.values()))
        print(name, "losses", r64["losses"], "sigma below / above", int(lo.sum()), int(hi.sum()), "smallest share", min(shares.values()), flush=True)
    save("sac_learn.npz", out, dict(hyper=hp, cases=meta_cases, max_action=1.0, nets=list(SAC_NETS),
                                    keys="<case>.{w,after}.<net>.<param>, <case>.{g64,E}.<net>.<param>, <case>.{state,action,reward,new_state,"
                                         "done,noise_value,noise_actor,losses64,E_losses,raw_sigma64}; losses: value, actor, critic"))


# ------------------------------------------------------------------ sac_act.npz
SAC_ACT_CASES = (  # (name, A, mean and std aimed at for the raw sigma outputs, max_action, seed of the heads, (seed, call) of the draws)
    ("A2_inside", 2, 0.5, 0.08, 1.0, 201, (2, 7)), ("A4_inside", 4, 0.5, 0.08, 1.0, 202, (0x1234ABCD00000002, 1)),
    ("A4_both", 4, 0.5, 1.0, 1.0, 203, (2, 0xFFFFFFFF)), ("A2_half", 2, 0.5, 0.08, 0.5, 204, (7, 3)))
ACT_ROWS = 128


def gen_sac_act(S):
    rng = np.random.default_rng(200)
    hidden = mlp(rng, 11, 256, ())  # one pair of hidden layers for the four cases (the file stays small); the heads differ
    out = {f"hidden.{k}": v for k, v in hidden.items()}
    meta_cases = {}
    for name, A, mean, std, max_action, seed, (draw_seed, call) in SAC_ACT_CASES:
        rng = np.random.default_rng(seed)
        sd = dict(hidden)
        for h in ("mu", "sigma"):
            sd[h + ".weight"], sd[h + ".bias"] = linear(rng, A, 256)
        obs = rng.uniform(-1.0, 1.0, (ACT_ROWS, 11)).astype(np.float32)
        aim_sigma(sd, obs, mean, std)
        z = sac_ref.draw32(draw_seed, ACT_ROWS, call)[:, :A].copy()
        res = []
        for double in (False, True):
            actor = load(S.ActorNetwork(1e-4, [11], max_action=max_action, fc1_dims=256, fc2_dims=256, n_actions=A), sd, double)
            watch = Watch({"actor": actor}, keep=(("actor", "mu"), ("actor", "sigma")))
            FedNormal.feed = [torch.from_numpy(z)]
            with torch.no_grad():
                state = torch.from_numpy(obs)
                action, log_prob = actor.sample_normal(state.double() if double else state, reparameterize=False)
            watch.close()
            assert action.dtype == (torch.float64 if double else torch.float32) and log_prob.shape == (ACT_ROWS, 1)
            head = torch.cat([watch.kept[("actor", "mu")][0], watch.kept[("actor", "sigma")][0]], 1).numpy()
            res.append((action.double().numpy(), log_prob.double().numpy().reshape(-1), head))
        (a32, lp32, h32), (a64, lp64, h64) = res
        rows = sac_ref.well_conditioned_rows(a64, max_action)
        assert rows.mean() >= 0.90, (name, rows.mean())
        raw = h64[:, A:]
        lo, hi = raw < sac_ref.SIGMA_MIN, raw > sac_ref.SIGMA_MAX
        assert (lo.sum() >= 16 and hi.sum() >= 16) if name.endswith("both") else not (lo.any() or hi.any()), name
        for k in ("mu.weight", "mu.bias", "sigma.weight", "sigma.bias"):
            out[f"{name}.{k}"] = sd[k]
        out[f"{name}.obs"], out[f"{name}.z"] = obs, z
        out[f"{name}.action64"], out[f"{name}.log_prob64"], out[f"{name}.head64"] = a64, lp64, h64
        out[f"{name}.E_a"], out[f"{name}.E_lp"] = np.float64(np.abs(a32 - a64).max()), np.float64(np.abs(lp32 - lp64)[rows].max())
        out[f"{name}.E_head"] = np.float64(np.abs(h32 - h64).max())
        out[f"{name}.seed_call_A"] = np.array([draw_seed, call, A], dtype=np.uint64)
        out[f"{name}.max_action"] = np.float64(max_action)
        meta_cases[name] = dict(n_actions=A, max_action=max_action, seed=draw_seed, call=call, well_conditioned_rows=int(rows.sum()),
                                sigma_below=int(lo.sum()), sigma_above=int(hi.sum()))
        print(name, "E_a", float(out[f"{name}.E_a"]), "E_lp", float(out[f"{name}.E_lp"]), "well-conditioned rows", int(rows.sum()), flush=True)
    save("sac_act.npz", out, dict(cases=meta_cases, rows=ACT_ROWS, z="sac_ref.draw32(seed, rows, call)[:, :A] (repository code, an input)",
                                  head64="mu [0..A), then the raw sigma outputs before the clamp",
                                  E_lp="on sac_ref.well_conditioned_rows of action64 only"))


# ------------------------------------------------------------------ dqn_learn.npz
DQN_HP = dict(gamma=0.99, lr=0.0005, batch=64, pool=192, grid=2.0 ** -12, margin=1e-3)


def dqn_agent(D, sd_eval, sd_target, double):
    agent = D.DQNAgent(gamma=DQN_HP["gamma"], epsilon=1.0, lr=DQN_HP["lr"], input_dims=[11], batch_size=DQN_HP["batch"], n_actions=8,
                       max_mem_size=DQN_HP["batch"])
    load(agent.Q_eval, sd_eval, double), load(agent.Q_target, sd_target, double)
    return agent


def gen_dqn_learn(D):
    hp, f = DQN_HP, np.float32
    rng = np.random.default_rng(301)
    sd_eval = mlp(rng, 11, 256, (("fc3", 8),), grid=hp["grid"])  # on a grid of 2^-12: exact in float32, and the file compresses
    sd_target = {k: (v + np.round(0.01 * rng.standard_normal(v.shape) / hp["grid"]) * hp["grid"]).astype(f) for k, v in sd_eval.items()}
    P = hp["pool"]
    # observations shaped like the env's (angles / distances of a few hundred), rewards of a few units
    state = (rng.uniform(0.0, 1.0, (P, 11)) * 360.0 - 50.0).astype(f)
    new_state = (state + 3.0 * rng.standard_normal((P, 11))).astype(f)
    agent = dqn_agent(D, sd_eval, sd_target, True)
    watch = Watch(dict(Q_eval=agent.Q_eval, Q_target=agent.Q_target))
    with torch.no_grad(), as_float64():
        agent.Q_eval(torch.from_numpy(state)), agent.Q_target(torch.from_numpy(new_state))
    watch.close()
    rows = np.nonzero(watch.margin().numpy() > hp["margin"])[0][:hp["batch"]]
    assert len(rows) == hp["batch"], len(rows)
    B = hp["batch"]
    batch = dict(state=state[rows], new_state=new_state[rows], action=rng.permutation(B).astype(np.int32) % 8,
                 reward=(2.0 * rng.standard_normal(B)).astype(f), done=np.arange(B) % 5 == 4)
    assert set(batch["action"]) == set(range(8)) and batch["done"].any() and not batch["done"].all()
    res = []
    for double in (False, True):
        agent = dqn_agent(D, sd_eval, sd_target, double)
        for i in range(B):
            agent.store_transition(batch["state"][i], batch["action"][i], batch["reward"][i], batch["new_state"][i], bool(batch["done"][i]))
        got = {}
        with first_rows(), locals_at_return(D.DQNAgent.learn.__code__, ("loss",), got):
            if double:
                with as_float64():
                    agent.learn()
            else:
                agent.learn()
        want = torch.float64 if double else torch.float32
        assert got["loss"].dtype == want and all(p.grad.dtype == want for p in agent.Q_eval.parameters())
        assert torch.float is torch.float32 and torch.zeros(1).double().float().dtype == torch.float32
        res.append((grads(agent.Q_eval), float(got["loss"].detach())))
    (g32, loss32), (g64, loss64) = res
    out = {}
    for k, g in g64.items():
        assert np.abs(g).max() > 0, k
        out[f"g64.{k}"], out[f"E.{k}"] = g, np.float64(np.abs(g32[k] - g).max())
        out[f"eval.{k}"], out[f"target.{k}"] = sd_eval[k], sd_target[k]
    out.update(batch)
    out["loss64"], out["E_loss"] = np.float64(loss64), np.float64(abs(loss32 - loss64))
    print("dqn_learn loss", loss64, {k: float(out[f"E.{k}"]) / np.abs(g).max() for k, g in g64.items()}, flush=True)
    save("dqn_learn.npz", out, dict(hyper=hp, net="11-256-256-8", terminal_rows=int(batch["done"].sum()),
                                    keys="{eval,target}.<param>, {g64,E}.<param>, state, new_state, action, reward, done, loss64, E_loss"))


def main():
    parts = sys.argv[1:] or ["sac_learn", "sac_act", "dqn_learn"]
    S, D = load_trainers()
    if "sac_learn" in parts:
        gen_sac_learn(S)
    if "sac_act" in parts:
        gen_sac_act(S)
    if "dqn_learn" in parts:
        gen_dqn_learn(D)


if __name__ == "__main__":
    main()
