"""rr_render_ego on the MI355X through BatchedRoboRugbyEnv.render_ego, PixelObservation and play_hive's ego recorder: egocentric frames of
many (arena, robot) pairs in one launch, held to tests/render_ego_ref.py -- the independent fp64 restatement of the picture
include/roborugby_amd.h specifies -- under that module's rule (exact outside a 1e-3 band around the layer boundaries, at most 0.2 % of a
frame's pixels inside it).  The states are the recorded ones the CPU twin (tests/test_render_ego_emulated.py) uses, tiled over 64 arenas
through set_state."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
N = 64

import oracle_lib as ol  # noqa: E402
import render_ego_ref as ego  # noqa: E402
import render_ref as ref  # noqa: E402


@functools.lru_cache(maxsize=None)
def _states(preset):
    st = ref.golden_states(GOLDEN, preset)
    pick = np.arange(N) % len(st["step"])
    return {k: v[pick] for k, v in st.items()}, len(st["step"])


@functools.lru_cache(maxsize=None)
def _want(preset, k, viewer, config, relative=True):
    """the reference's frame of tiled state k seen from `viewer`: computed once, shared by every test that needs it, never written to"""
    cfg, (st, _) = ol.PRESETS[preset], _states(preset)
    w, h, S, span, ahead = config
    return ego.frame(cfg["W"], cfg["H"], cfg["nr_h"], cfg["nb_p"], st["robots"][k], st["balls"][k], viewer, w, h, S, span, ahead, relative)


def _env(preset, **kw):
    import roborugby_amd as rr
    env = rr.BatchedRoboRugbyEnv(N, preset=ol.product_preset(preset), seed=3, **kw)
    st, _ = _states(preset)
    env.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    return env


def _render(env, config, **kw):
    w, h, S, span, ahead = config
    return env.render_ego(width=w, height=h, samples=S, span=span, ahead=ahead, **kw)


def _check_every_viewer(env, preset, configs, what=""):
    """every unique state seen from every robot, one launch per configuration"""
    cfg, unique = ol.PRESETS[preset], _states(preset)[1]
    nr = cfg["nr_h"] + cfg["nr_g"]
    arenas, robots = np.repeat(np.arange(unique), nr), np.tile(np.arange(nr), unique)
    for config in configs:
        frames = _render(env, config, arenas=arenas, robots=robots)
        assert frames.shape == (unique * nr, config[1], config[0], 3) and frames.dtype == torch.uint8 and frames.device == env.device
        worst = 0.0
        for f, k, v in zip(frames.cpu().numpy(), arenas, robots):
            want, dist = _want(preset, int(k), int(v), config)
            worst = max(worst, ego.check(f, want, dist, config[2], (what, preset, config, int(k), int(v))))
        print(f"{what} {preset} {config}: {len(arenas)} frames, worst exempt share {100 * worst:.3f} %")


@pytest.mark.parametrize("dtype", ["f64", "f32_state", "f32"])
def test_G_frames_match_the_reference_in_every_dtype_from_every_robot(dtype):
    env = _env("G", dtype=dtype)
    _check_every_viewer(env, "G", ego.CONFIGS, dtype)
    unique = _states("G")[1]
    full = env.render_ego(robots=3)  # the defaults: every arena, 64 x 64, span 400, relative colours, interleaved
    assert full.shape == (N, 64, 64, 3)
    assert torch.equal(full[unique:], full[:N - unique])  # the tiled arenas hold the same states: the same frames
    want, dist = _want("G", 1, 3, ego.CONFIGS[0])
    ego.check(full[1].cpu().numpy(), want, dist, 1, (dtype, "defaults"))
    env.close()


@pytest.mark.parametrize("preset", ["T", "Dwide"])
def test_other_shapes_and_a_non_square_arena(preset):
    env = _env(preset)
    _check_every_viewer(env, preset, ego.CONFIGS[1:3])
    env.close()


def test_the_parity_library_draws_the_same_picture():
    env = _env("G", exact_trig=True)
    _check_every_viewer(env, "G", ego.CONFIGS[3:], "parity library")
    env.close()


def test_relative_planar_and_supersampled_frames_are_what_they_must_be_bit_for_bit():
    env = _env("G")
    robots = torch.arange(N, dtype=torch.int32) % 4
    kw = dict(robots=robots, span=400.0, ahead=100.0)
    absolute = env.render_ego(width=64, height=48, relative=False, **kw)
    relative = env.render_ego(width=64, height=48, relative=True, **kw)
    happy = (robots < 2).to(env.device)
    assert torch.equal(relative[happy], absolute[happy])  # a happy viewer: the flag changes nothing
    swapped = torch.as_tensor(ego.swap_palette(absolute.cpu().numpy()), device=env.device)
    assert torch.equal(relative[~happy], swapped[~happy]) and not torch.equal(relative[~happy], absolute[~happy])
    for S in (1, 2):
        inter = env.render_ego(width=64, height=48, samples=S, **kw)
        planar = env.render_ego(width=64, height=48, samples=S, planar=True, **kw)
        assert planar.shape == (N, 3, 48, 64) and torch.equal(planar, inter.permute(0, 3, 1, 2))
    for S, size in ((2, 32), (4, 24)):
        fine = env.render_ego(width=size * S, samples=1, **kw).to(torch.int64)
        got = env.render_ego(width=size, samples=S, **kw)
        box = (fine.view(N, size, S, size, S, 3).sum(dim=(2, 4)) + (S * S) // 2) // (S * S)
        assert torch.equal(got.to(torch.int64), box)
    env.close()


def test_index_lists_of_every_kind_duplicates_and_indices_out_of_range():
    env = _env("G")
    base = [env.render_ego(robots=v, width=64, height=48) for v in range(4)]
    arenas = [63, 0, 0, 17, -1, 64, 5, 5, 2 ** 31 - 1, 9]
    robots = [3, 1, 1, 0, 0, 0, -1, 4, 0, -2 ** 31]
    kinds = (list, np.array, torch.tensor, lambda x: torch.tensor(x, dtype=torch.int32, device=env.device))
    for kind in kinds:
        got = env.render_ego(arenas=kind(arenas), robots=kind(robots), width=64, height=48)
        assert got.shape == (10, 48, 64, 3)
        assert torch.equal(got[1], got[2])
        assert int(got[4:].max()) == 0
        assert all(torch.equal(got[k], base[robots[k]][arenas[k]]) for k in range(4))
    assert all(int(b.amax(dim=(1, 2, 3)).min()) == 255 for b in base)  # no in-range frame is black
    only = env.render_ego(robots=np.arange(N) % 4, width=64, height=48)  # robots alone: arena k
    assert all(torch.equal(only[k], base[k % 4][k]) for k in range(N))
    env.close()


@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("S", [1, 4])
def test_every_byte_of_the_frames_is_rewritten_and_nothing_behind_them(S, planar):
    env = _env("G")
    m, w, h = 5, 64, 48
    kw = dict(arenas=[3, 1, 64, 2, 0], robots=[0, 3, 1, 4, 2], width=w, height=h, samples=S, planar=planar)
    fresh = env.render_ego(**kw)
    for fill in (0xAB, 0x54):  # two fills: a byte left alone shows in one of the two
        buf = torch.full((m + 2, h * w * 3), fill, dtype=torch.uint8, device=env.device)
        got = env.render_ego(out=buf[:m], **kw)
        assert got.data_ptr() == buf.data_ptr() and got.shape == fresh.shape
        assert bool((buf[m:] == fill).all())
        assert torch.equal(got, fresh)
    env.close()


def _bits(state):
    return {k: v.clone().view(torch.int64 if v.dtype == torch.float64 else torch.int32) for k, v in state.items()}


def test_rendering_reads_the_records_and_nothing_else():
    env, twin = _env("G"), _env("G")
    before = _bits(env.get_state())
    env.render_ego(robots=2, width=96, samples=2)
    env.render_ego(arenas=[5, 5, -3, 99], robots=[1, 7, 0, 0], width=64, height=48, planar=True)
    after = _bits(env.get_state())
    assert all(torch.equal(before[k], after[k]) for k in before)
    g = torch.Generator(device="cuda").manual_seed(4)
    for k in range(10):
        a = torch.randint(0, 8, (N, 4), generator=g, device="cuda", dtype=torch.int32)
        o1, r1, d1, i1 = env.step(a)
        env.render_ego(robots=k % 4, width=32)
        o2, r2, d2, i2 = twin.step(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(i1.status, i2.status)
    s1, s2 = _bits(env.get_state()), _bits(twin.get_state())
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    env.close(); twin.close()


def _budgeted_env():
    """budget 1 on the stuck chase arenas (every one of them parks in its first call), next to recorded quiet states (a quiet arena never
    reads the clock)"""
    import roborugby_amd as rr
    d = np.load(os.path.join(HERE, "data", "stuck_chase_G.npz"))
    quiet, _ = _states("G")
    k = 24
    st = {key: np.concatenate([d[key], quiet[key][:k]]) for key in ("robots", "robots_i", "balls", "step")}
    n = len(st["step"])
    env = rr.BatchedRoboRugbyEnv(n, preset="G", seed=3, time_limit=True, auto_reset=True, step_budget_clocks=1)
    env.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    acts = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    acts[:n - k] = torch.as_tensor(d["actions"], device="cuda").to(torch.int32)
    return env, acts, n


def test_a_budgeted_handle_renders_and_its_ready_arenas_match_the_reference():
    from roborugby_amd.env import STATUS_NOT_READY
    env, acts, n = _budgeted_env()
    _, _, _, info = env.step(acts)
    config = ego.CONFIGS[3]
    frames = _render(env, config, robots=1)          # returns 0 with arenas parked mid-step
    assert frames.shape == (n, 96, 96, 3) and int(frames.amax(dim=(1, 2, 3)).min()) == 255
    ready = torch.nonzero((info.status & STATUS_NOT_READY) == 0).view(-1).cpu().numpy()
    assert 0 < len(ready) < n, len(ready)
    now = {key: v.cpu().numpy() for key, v in env.get_state().items()}
    cfg = ol.PRESETS["G"]
    for a in ready[-8:]:
        want, dist = ego.frame(cfg["W"], cfg["H"], cfg["nr_h"], cfg["nb_p"], now["robots"][a], now["balls"][a], 1, 96, 96, 1, 500.0, 60.0, True)
        ego.check(frames[a].cpu().numpy(), want, dist, 1, ("budget", int(a)))
    print(f"budget 1: {n - len(ready)} of {n} arenas parked; {min(len(ready), 8)} ready frames checked")
    env.close()


def test_every_guard_refuses_with_a_message_and_leaves_the_buffer_alone():
    env = _env("G")
    lib, h, s = env._lib, env._h, env._stream()
    buf = torch.full((4 * 48 * 64 * 3 + 8,), 0xAB, dtype=torch.uint8, device=env.device)
    p = C.c_void_p(buf.data_ptr())
    assert buf.data_ptr() % 4 == 0
    nan, inf = float("nan"), float("inf")
    ok = (h, None, None, 4, 64, 48, 1, 400.0, 0.0, 3, p)

    def case(**kw):
        names = ("h", "arenas", "robots", "m", "width", "height", "samples", "span", "ahead", "flags", "rgb")
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    cases = {
        "null handle": case(h=None), "null rgb": case(rgb=None), "m = 0": case(m=0), "m above 1 << 20": case(m=(1 << 20) + 1),
        "width 0": case(width=0), "width not a multiple of 4": case(width=62), "width above 1024": case(m=1, width=1028, height=1),
        "height 0": case(height=0), "height above 1024": case(m=1, width=4, height=1025),
        "samples 3": case(samples=3), "samples 0": case(samples=0), "samples 8": case(samples=8),
        "span NaN": case(span=nan), "span inf": case(span=inf), "span below 16": case(span=15.5), "span above 16384": case(span=16385.0),
        "span negative": case(span=-400.0), "ahead NaN": case(ahead=nan), "ahead inf": case(ahead=-inf), "ahead above 8192": case(ahead=8193.0),
        "ahead below -8192": case(ahead=-8193.0), "flag bit 2": case(flags=4), "flag bits high": case(flags=-1),
        "misaligned rgb": case(rgb=C.c_void_p(buf.data_ptr() + 2)),
    }
    for what, args in cases.items():
        assert lib.rr_render_ego(*args, s) == -1, what
        msg = lib.rr_last_error()
        assert msg and msg.startswith(b"rr_render_ego:"), (what, msg)
    torch.cuda.synchronize()
    assert bool((buf == 0xAB).all())
    assert lib.rr_render_ego(*ok, s) == 0  # ... and the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert bool((buf[:4 * 48 * 64 * 3] != 0xAB).any()) and bool((buf[4 * 48 * 64 * 3:] == 0xAB).all())
    # the Python surface refuses before any launch as well
    with pytest.raises(ValueError, match="1 GiB"):
        env.render_ego(arenas=list(range(64)) * 6, width=1024)
    with pytest.raises(ValueError):
        env.render_ego(arenas=[0.5])
    with pytest.raises(ValueError):
        env.render_ego(robots=[0.5] * N)
    with pytest.raises(ValueError):
        env.render_ego(robots=[0, 1])  # two robots for 64 frames
    with pytest.raises(ValueError):
        env.render_ego(width=64, height=48, out=buf[:100])
    from roborugby_amd import _lib
    with pytest.raises(_lib.RRError, match="multiple of 4"):
        env.render_ego(width=30)
    assert env.render_ego(arenas=[1], width=4, height=1).shape == (1, 1, 4, 3)  # the smallest frame there is
    assert env.render_ego(arenas=[1], width=4, height=1, planar=True).shape == (1, 3, 1, 4)
    env.close()


def _slots(pix, stack):
    return pix.view(pix.shape[:-3] + (stack, 3) + pix.shape[-2:])


def test_pixel_observation_stacks_frames_and_restarts_a_re_placed_row():
    import roborugby_amd as rr
    from roborugby_amd.env import STATUS_WAS_RESET
    env, twin = (rr.BatchedRoboRugbyEnv(N, preset="T", seed=3) for _ in range(2))
    px = rr.PixelObservation(env, robots=0, size=32, stack=3)
    assert px.observation_space.shape == (9, 32, 32) and px.observation_space.dtype == np.uint8
    assert int(px.observation_space.low.max()) == 0 and int(px.observation_space.high.min()) == 255
    pix = px.reset()
    lidar = twin.reset()
    assert pix.shape == (N, 9, 32, 32) and pix.dtype == torch.uint8 and pix.device == env.device and torch.equal(px.lidar, lidar)
    cur = env.render_ego(robots=0, width=32, planar=True)
    assert all(torch.equal(_slots(pix, 3)[:, k], cur) for k in range(3))
    st = {k: v.clone() for k, v in env.get_state().items()}
    st["step"][::4] = env.spec.max_episode_steps - 2   # these end their episode, and are re-placed, within four steps
    env.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    twin.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    g = torch.Generator(device="cuda").manual_seed(5)
    restarted = torch.zeros(N, dtype=torch.bool, device="cuda")
    ptr = pix.data_ptr()
    for k in range(5):
        prev = _slots(pix, 3).clone()
        a = torch.randint(0, 8, (N,), generator=g, device="cuda", dtype=torch.int32)
        if k % 2:
            pix, reward, done, info = px.step(a)
            o2, r2, d2, i2 = twin.step(a)
        else:  # ... and the thrust entry
            thrust = (a.view(N, 1) % 3 - 1).to(torch.float32).repeat(1, 2)
            pix, reward, done, info = px.step_thrust(thrust)
            o2, r2, d2, i2 = twin.step_thrust(thrust)
        assert pix.data_ptr() == ptr and pix.shape == (N, 9, 32, 32)  # the persistent buffer
        assert torch.equal(info.lidar, o2) and torch.equal(reward, r2) and torch.equal(done, d2) and torch.equal(info.status, i2.status)
        now, cur = _slots(pix, 3), env.render_ego(robots=0, width=32, planar=True)
        assert torch.equal(now[:, 2], cur)  # the newest slot is the picture of the current state
        was = (info.status & STATUS_WAS_RESET) != 0
        assert torch.equal(now[was, 0], cur[was]) and torch.equal(now[was, 1], cur[was])
        assert torch.equal(now[~was, :2], prev[~was, 1:])  # the others dropped their oldest frame
        restarted |= was
    assert bool(restarted[::4].all()) and not bool(restarted.all())
    # a masked reset restarts the rows in the mask and leaves the others alone
    prev = _slots(pix, 3).clone()
    mask = torch.arange(N, device="cuda") % 3 == 0
    now = _slots(px.reset(mask), 3)
    cur = env.render_ego(robots=0, width=32, planar=True)
    assert all(torch.equal(now[mask, k], cur[mask]) for k in range(3)) and torch.equal(now[~mask], prev[~mask])
    assert not torch.equal(now[mask], prev[mask])
    env.close(); twin.close()


def test_pixel_observation_of_several_robots_and_under_the_budgeted_step():
    import roborugby_amd as rr
    from roborugby_amd.env import STATUS_NOT_READY, STATUS_WAS_RESET
    env = _env("G")
    px = rr.PixelObservation(env, robots=(0, 2), size=32, span=300.0, ahead=40.0, stack=3, relative=True)
    pix = px.reset()
    assert pix.shape == (N, 2, 9, 32, 32)
    a = torch.randint(0, 8, (N, 4), device="cuda", dtype=torch.int32)
    first = _slots(pix, 3).clone()
    pix, _, _, info = px.step(a)
    assert pix.shape == (N, 2, 9, 32, 32)
    now = _slots(pix, 3)
    for r, robot in enumerate((0, 2)):
        cur = env.render_ego(robots=robot, width=32, span=300.0, ahead=40.0, planar=True)
        assert torch.equal(now[:, r, 2], cur) and torch.equal(now[:, r, :2], first[:, r, 1:])
    assert not torch.equal(now[:, 0, 2], now[:, 1, 2])
    env.close()
    # budget 1: a NOT_READY row keeps its stack, a row that stepped shifts
    env, acts, n = _budgeted_env()
    px = rr.PixelObservation(env, robots=1, size=32, stack=2)   # (no reset: the stack starts as the picture of the state it finds)
    before = _slots(px._pixels(), 2).clone()
    assert torch.equal(before[:, 0], before[:, 1]) and int(before.amax(dim=(1, 2, 3, 4)).min()) == 255
    pix, _, _, info = px.step(acts)
    now = _slots(pix, 2)
    parked = (info.status & STATUS_NOT_READY) != 0
    stepped = ~parked & ((info.status & STATUS_WAS_RESET) == 0)
    assert 0 < int(parked.sum()) < n and int(stepped.sum()) > 0
    assert torch.equal(now[parked], before[parked])
    cur = env.render_ego(robots=1, width=32, planar=True)
    assert torch.equal(now[stepped, 0], before[stepped, 1]) and torch.equal(now[stepped, 1], cur[stepped])
    env.close()


def test_play_hive_records_the_ego_view_and_plays_the_same_game(tmp_path):
    from PIL import Image
    from roborugby_amd import dqn
    ck, gif = str(tmp_path / "ck.pt"), str(tmp_path / "hive_ego.gif")
    dqn.train(num_envs=256, steps=2, preset="T", checkpoint=ck, log_every=0, batch_size=256)
    plain = dqn.play_hive(ck, num_envs=N, steps=5, seed=2)
    taped = dqn.play_hive(ck, num_envs=N, steps=5, seed=2, record=gif, record_view="ego")
    assert set(plain) == set(taped)
    assert all(plain[k] == taped[k] for k in plain if k != "env_steps_per_s"), (plain, taped)
    with Image.open(gif) as im:
        assert im.n_frames == 5 and im.size == (2 + 4 * 98, 2 + 4 * 98)  # 16 views of 96x96, two pixels between and around them
        im.seek(4)
        last = np.asarray(im.convert("RGB"))
    tile = last[2:98, 2:98]
    assert len(np.unique(last.reshape(-1, 3), axis=0)) > 4   # something is on it ...
    assert (np.abs(tile[47:49, 47:49].astype(int) - np.array(ref.TEAM_HAPPY)).sum(axis=-1) < 60).all()  # ... the viewer, in the centre
    with pytest.raises(ValueError):
        dqn.play_hive(ck, num_envs=N, steps=1, seed=2, record_view="sky")
