"""rr_render on the MI355X through BatchedRoboRugbyEnv.render_batch: frames of many arenas in one launch, held to tests/render_ref.py --
the independent fp64 restatement of the picture include/roborugby_amd.h specifies -- under that module's rule (exact outside a 1e-3 band
around the layer boundaries, at most 0.2 % of a frame's pixels inside it).  The states are the recorded ones the CPU twin
(tests/test_render_emulated.py) uses, tiled over 64 arenas through set_state."""
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
import render_ref as ref  # noqa: E402


@functools.lru_cache(maxsize=None)
def _states(preset):
    st = ref.golden_states(GOLDEN, preset)
    pick = np.arange(N) % len(st["step"])
    return {k: v[pick] for k, v in st.items()}, len(st["step"])


@functools.lru_cache(maxsize=None)
def _want(preset, k, width, height, S=1):
    """the reference's frame of tiled state k: computed once, shared by every test that needs it, never written to"""
    cfg, (st, _) = ol.PRESETS[preset], _states(preset)
    return ref.frame(cfg["W"], cfg["H"], cfg["nr_h"], cfg["nb_p"], st["robots"][k], st["balls"][k], width, height, S)


def _env(preset, **kw):
    import roborugby_amd as rr
    env = rr.BatchedRoboRugbyEnv(N, preset=ol.product_preset(preset), seed=3, **kw)
    st, _ = _states(preset)
    env.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    return env


def _check_frames(preset, frames, arenas, width, height, S=1, what=""):
    frames = frames.cpu().numpy()
    worst = 0.0
    for f, k in zip(frames, arenas):
        want, dist = _want(preset, int(k), width, height, S)
        worst = max(worst, ref.check(f, want, dist, S, (what, preset, width, height, int(k))))
    print(f"{what} {preset} {width}x{height} S={S}: {len(frames)} frames, worst exempt share {100 * worst:.3f} %")


@pytest.mark.parametrize("dtype", ["f64", "f32_state", "f32"])
def test_G_frames_match_the_reference_in_every_dtype(dtype):
    env = _env("G", dtype=dtype)
    unique = _states("G")[1]
    for w, h in ((96, 96), (64, 48)):
        frames = env.render_batch(width=w, height=h)
        assert frames.shape == (N, h, w, 3) and frames.dtype == torch.uint8 and frames.device == env.device
        _check_frames("G", frames[:unique], range(unique), w, h, what=dtype)
        assert torch.equal(frames[unique:], frames[:N - unique])  # the tiled arenas hold the same states: the same frames
    native = env.render_batch(arenas=[0, 7])
    assert native.shape == (2, 800, 800, 3)
    _check_frames("G", native, (0, 7), 800, 800, what=dtype + " native")
    env.close()


@pytest.mark.parametrize("preset,size", [("T", (96, 96)), ("Dwide", (96, 64))])
def test_other_shapes_and_a_non_square_arena(preset, size):
    env = _env(preset)
    unique = _states(preset)[1]
    _check_frames(preset, env.render_batch(width=size[0], height=size[1])[:unique], range(unique), *size)
    env.close()


def test_the_parity_library_draws_the_same_picture():
    env = _env("G", exact_trig=True)
    unique = _states("G")[1]
    _check_frames("G", env.render_batch(width=96, height=96)[:unique], range(unique), 96, 96, what="parity library")
    env.close()


def test_arena_lists_duplicates_and_indices_out_of_range():
    env = _env("G")
    base = env.render_batch(width=64, height=48)
    idx = [63, 0, 0, 17, -1, 64]
    for arenas in (idx, torch.tensor(idx), torch.tensor(idx, dtype=torch.int32, device=env.device), np.array(idx)):
        got = env.render_batch(arenas=arenas, width=64, height=48)
        assert got.shape == (6, 48, 64, 3)
        assert torch.equal(got[1], got[2])
        assert int(got[4:].max()) == 0
        assert all(torch.equal(got[k], base[idx[k]]) for k in range(4))
    assert int(base.amax(dim=(1, 2, 3)).min()) == 255  # no in-range frame is black
    env.close()


@pytest.mark.parametrize("S", [1, 4])
def test_every_byte_of_the_frames_is_rewritten_and_nothing_behind_them(S):
    env = _env("G")
    m, w, h = 5, 64, 48
    buf = torch.full((m + 2, h, w, 3), 0xAB, dtype=torch.uint8, device=env.device)
    got = env.render_batch(arenas=[3, 1, 64, 2, 0], width=w, height=h, samples=S, out=buf[:m])
    assert got.data_ptr() == buf.data_ptr()
    assert bool((buf[m:] == 0xAB).all())
    fresh = env.render_batch(arenas=[3, 1, 64, 2, 0], width=w, height=h, samples=S)
    assert torch.equal(buf[:m], fresh)
    other = torch.full((m + 2, h, w, 3), 0x54, dtype=torch.uint8, device=env.device)  # another fill: a byte left alone shows in one of the two
    env.render_batch(arenas=[3, 1, 64, 2, 0], width=w, height=h, samples=S, out=other[:m])
    assert torch.equal(other[:m], fresh) and bool((other[m:] == 0x54).all())
    env.close()


@pytest.mark.parametrize("S,size", [(2, 48), (4, 24)])
def test_supersampling_is_the_box_filter_of_the_larger_frame_bit_for_bit(S, size):
    env = _env("G")
    fine = env.render_batch(width=96, height=96).to(torch.int64)
    got = env.render_batch(width=size, height=size, samples=S)
    box = (fine.view(N, size, S, size, S, 3).sum(dim=(2, 4)) + (S * S) // 2) // (S * S)
    assert torch.equal(got.to(torch.int64), box)
    _check_frames("G", got[:3], range(3), size, size, S)
    env.close()


def _bits(state):
    return {k: v.clone().view(torch.int64 if v.dtype == torch.float64 else torch.int32) for k, v in state.items()}


def test_rendering_reads_the_records_and_nothing_else():
    env, twin = _env("G"), _env("G")
    before = _bits(env.get_state())
    env.render_batch(width=96, height=96, samples=2)
    env.render_batch(arenas=[5, 5, -3, 99], width=64, height=48)
    after = _bits(env.get_state())
    assert all(torch.equal(before[k], after[k]) for k in before)
    g = torch.Generator(device="cuda").manual_seed(4)
    for _ in range(10):
        a = torch.randint(0, 8, (N, 4), generator=g, device="cuda", dtype=torch.int32)
        o1, r1, d1, i1 = env.step(a)
        env.render_batch(width=32, height=32)
        o2, r2, d2, i2 = twin.step(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(i1.status, i2.status)
    s1, s2 = _bits(env.get_state()), _bits(twin.get_state())
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    env.close(); twin.close()


def test_a_budgeted_handle_renders_and_its_ready_arenas_match_the_reference():
    """budget 1 on the stuck chase arenas (every one of them parks in its first call), next to recorded quiet states (a quiet arena
    never reads the clock): the entry accepts the handle, parked arenas show their mid-step record, the others the picture of their state"""
    import roborugby_amd as rr
    from roborugby_amd.env import STATUS_NOT_READY
    d = np.load(os.path.join(HERE, "data", "stuck_chase_G.npz"))
    quiet, _ = _states("G")
    k = 24
    st = {key: np.concatenate([d[key], quiet[key][:k]]) for key in ("robots", "robots_i", "balls", "step")}
    n = len(st["step"])
    env = rr.BatchedRoboRugbyEnv(n, preset="G", seed=3, time_limit=True, auto_reset=True, step_budget_clocks=1)
    env.set_state(st["robots"], st["robots_i"], st["balls"], st["step"])
    acts = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    acts[:n - k] = torch.as_tensor(d["actions"], device="cuda").to(torch.int32)
    _, _, _, info = env.step(acts)
    frames = env.render_batch(width=96, height=96)          # returns 0 with arenas parked mid-step
    assert frames.shape == (n, 96, 96, 3) and int(frames.amax(dim=(1, 2, 3)).min()) == 255
    ready = torch.nonzero((info.status & STATUS_NOT_READY) == 0).view(-1).cpu().numpy()
    assert 0 < len(ready) < n, len(ready)
    now = {key: v.cpu().numpy() for key, v in env.get_state().items()}
    cfg = ol.PRESETS["G"]
    for a in ready[-8:]:
        want, dist = ref.frame(cfg["W"], cfg["H"], cfg["nr_h"], cfg["nb_p"], now["robots"][a], now["balls"][a], 96, 96)
        ref.check(frames[a].cpu().numpy(), want, dist, 1, ("budget", int(a)))
    print(f"budget 1: {n - len(ready)} of {n} arenas parked; {min(len(ready), 8)} ready frames checked")
    env.close()


def test_every_guard_refuses_with_a_message_and_leaves_the_buffer_alone():
    env = _env("G")
    lib, h, s = env._lib, env._h, env._stream()
    buf = torch.full((4 * 48 * 64 * 3 + 8,), 0xAB, dtype=torch.uint8, device=env.device)
    p = C.c_void_p(buf.data_ptr())
    assert buf.data_ptr() % 4 == 0
    cases = {
        "null handle": (None, None, 4, 64, 48, 1, p),
        "null rgb": (h, None, 4, 64, 48, 1, None),
        "m = 0": (h, None, 0, 64, 48, 1, p),
        "m above 1 << 20": (h, None, (1 << 20) + 1, 64, 48, 1, p),
        "width 0": (h, None, 4, 0, 48, 1, p),
        "width not a multiple of 4": (h, None, 4, 62, 48, 1, p),
        "width above 4096": (h, None, 1, 4100, 1, 1, p),
        "height 0": (h, None, 4, 64, 0, 1, p),
        "height above 4096": (h, None, 1, 4, 4097, 1, p),
        "samples 3": (h, None, 4, 64, 48, 3, p),
        "samples 0": (h, None, 4, 64, 48, 0, p),
        "samples 8": (h, None, 4, 64, 48, 8, p),
        "misaligned rgb": (h, None, 4, 64, 48, 1, C.c_void_p(buf.data_ptr() + 2)),
    }
    for what, (hh, arenas, m, w, hgt, S, rgb) in cases.items():
        assert lib.rr_render(hh, arenas, m, w, hgt, S, rgb, s) == -1, what
        msg = lib.rr_last_error()
        assert msg and msg.startswith(b"rr_render:"), (what, msg)
    torch.cuda.synchronize()
    assert bool((buf == 0xAB).all())
    # the Python surface refuses before any launch as well
    with pytest.raises(ValueError, match="1 GiB"):
        env.render_batch(arenas=list(range(64)) * 10, width=800, height=800)
    with pytest.raises(ValueError):
        env.render_batch(arenas=[0.5])
    with pytest.raises(ValueError):
        env.render_batch(width=64, height=48, out=buf[:100])
    from roborugby_amd import _lib
    with pytest.raises(_lib.RRError, match="multiple of 4"):
        env.render_batch(width=30, height=30)
    assert env.render_batch(arenas=[1], width=4, height=1).shape == (1, 1, 4, 3)  # the smallest frame there is
    env.close()


def test_render_keeps_drawing_the_host_picture():
    env = _env("G")
    img = env.render("rgb_array", arena=2)
    assert img.shape == (800, 1100, 3) and env.render("human") is None
    env.close()


def test_play_hive_records_a_gif_and_plays_the_same_game(tmp_path):
    from PIL import Image
    from roborugby_amd import dqn
    ck, gif = str(tmp_path / "ck.pt"), str(tmp_path / "hive.gif")
    dqn.train(num_envs=256, steps=2, preset="T", checkpoint=ck, log_every=0, batch_size=256)
    plain = dqn.play_hive(ck, num_envs=N, steps=5, seed=2)
    taped = dqn.play_hive(ck, num_envs=N, steps=5, seed=2, record=gif)
    assert set(plain) == set(taped)
    assert all(plain[k] == taped[k] for k in plain if k != "env_steps_per_s"), (plain, taped)
    with Image.open(gif) as im:
        assert im.n_frames == 5 and im.size == (2 + 4 * 98, 2 + 4 * 98)  # 16 arenas of 96x96, two pixels between and around them
        im.seek(4)
        last = np.asarray(im.convert("RGB"))
    assert (last[2:98, 2:98] == 255).all(axis=-1).mean() > 0.5  # a white field ...
    assert len(np.unique(last.reshape(-1, 3), axis=0)) > 4      # ... with something on it
