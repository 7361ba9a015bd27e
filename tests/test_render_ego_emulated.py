"""The egocentric frame kernel's source (csrc/rr_render.hpp: draw-list builder with the viewer's palette, camera, shading core, both
byte packings) compiled with g++ and walked over k_render_ego's grid on the host (tests/emu/rr_render_ego_emu.cpp), against
tests/render_ego_ref.py -- the independent fp64 restatement of the picture include/roborugby_amd.h specifies -- under that module's rule:
exact outside a 1e-3 band around the layer boundaries, at most 0.2 % of a frame's pixels inside it.  tests/test_gpu_render_ego.py holds
the device to the same reference on the same states."""
import functools
import math

import numpy as np
import pytest

import oracle_lib as ol
import render_ego_emu_lib as emu
import render_ego_ref as ego
import render_ref as ref


@functools.lru_cache(maxsize=None)
def _states(golden_dir, preset):
    return ref.golden_states(golden_dir, preset)


@functools.lru_cache(maxsize=None)
def _reference(golden_dir, preset, config, relative=True):
    """the reference's frames of a fixture's states for every viewer [viewer][state], computed once and shared by the fp64 and the fp32 case"""
    cfg, st = ol.PRESETS[preset], _states(golden_dir, preset)
    w, h, S, span, ahead = config
    return [[ego.frame(cfg["W"], cfg["H"], cfg["nr_h"], cfg["nb_p"], r, b, v, w, h, S, span, ahead, relative)
             for r, b in zip(st["robots"], st["balls"])] for v in range(cfg["nr_h"] + cfg["nr_g"])]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("config", ego.CONFIGS, ids=lambda c: "%dx%d-S%d-span%g-ahead%g" % c)
@pytest.mark.parametrize("preset", ["G", "Dwide", "T"])
def test_emulated_source_matches_the_reference_on_recorded_states(golden_dir, preset, config, f32):
    st = _states(golden_dir, preset)
    n = len(st["step"])
    w, h, S, span, ahead = config
    worst = 0.0
    for v, frames in enumerate(_reference(golden_dir, preset, config)):
        got = emu.render(preset, st["robots"], st["balls"], w, h, S, span, ahead, viewers=[v] * n, relative=True, f32=f32)
        worst = max([worst] + [ego.check(got[k], want, dist, S, (preset, config, v, k)) for k, (want, dist) in enumerate(frames)])
        assert any((f != 255).any() for f in got)  # (not a white sheet)
    print(f"{preset} {config} {'f32' if f32 else 'f64'} records: {n} states x {v + 1} viewers, worst exempt share {100 * worst:.3f} %")


# ---- crafted arenas (G's shape: 2 + 2 robots, 4 + 4 balls, 800 x 800).  256 pixels over 256 arena units: pixel (row j, column i) is the
# sample p = i - 127.5 to the right of the viewer's centre and fwd = 127.5 - j in front of it (ahead = 0).
FAR = -1000.0
PX = 256


def _arena(robots, balls, nr=4, nb=8):
    r, b = np.zeros((nr, 10)), np.zeros((nb, 8))
    r[:, 0], r[:, 1] = -5000.0, -5000.0
    b[:, 0], b[:, 1] = FAR, 50.0
    for k, (x, y, rot) in robots.items():
        r[k, 0], r[k, 1], r[k, 6] = x, y, rot
    for k, (x, y) in balls.items():
        b[k, 0], b[k, 1] = x, y
    return r, b


def _pixel_of(pose, x, y):
    """(row, column) of the arena point (x, y) in the 256-pixel view of a robot at pose (cx, cy, rot): the camera convention, restated"""
    cx, cy, rot = pose
    th = math.radians(360.0 - rot)
    front, side = (math.cos(th), math.sin(th)), (-math.sin(th), math.cos(th))  # the robot's +u and +v directions in the arena
    fwd = (x - cx) * front[0] + (y - cy) * front[1]
    p = (x - cx) * side[0] + (y - cy) * side[1]
    return int(math.floor(PX / 2 - fwd)), int(math.floor(p + PX / 2))


# pose of the viewer (it faces a wall 50 - 60 units away), a point inside a goal it can see, and that goal's colour for a happy viewer
CRAFTED = {0.0: ((740.3, 600.4, 0.0), (790.0, 700.0), ref.GOAL_HAPPY), 90.0: ((200.3, 60.4, 90.0), (100.0, 10.0), ref.GOAL_GRUMPY),
           180.0: ((60.4, 200.3, 180.0), (10.0, 100.0), ref.GOAL_GRUMPY), 270.0: ((600.4, 740.3, 270.0), (700.0, 790.0), ref.GOAL_HAPPY),
           33.3: ((750.3, 600.4, 33.3), (790.0, 700.0), ref.GOAL_HAPPY)}


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("viewer", [0, 2], ids=["happy", "grumpy"])
@pytest.mark.parametrize("rot", sorted(CRAFTED))
def test_front_is_up_and_plus_v_is_right_at_every_angle(rot, viewer, f32):
    pose, goal_pt, goal_col = CRAFTED[rot]
    cx, cy, _ = pose
    th = math.radians(360.0 - rot)
    c, s = math.cos(th), math.sin(th)
    r, b = _arena({viewer: pose}, {0: (cx + 50.0 * c, cy + 50.0 * s), 5: (cx - 50.0 * s, cy + 50.0 * c)})  # 50 ahead; 50 to the +v side
    img = emu.render("G", r[None], b[None], PX, PX, 1, float(PX), 0.0, viewers=[viewer], relative=True, f32=f32)[0]
    want, dist = ego.frame(800.0, 800.0, 2, 4, r, b, viewer, PX, PX, 1, float(PX), 0.0, True)
    ego.check(img, want, dist, 1, (rot, viewer))
    mine = viewer >= 2  # a grumpy viewer sees the pairs swapped: its own team is blue, the ball that scores for it is green, ...
    swap = lambda col: tuple(ego.swap_palette(np.array([col]))[0]) if mine else col  # noqa: E731
    assert tuple(img[127, 128]) == ref.TEAM_HAPPY and tuple(img[127, 127]) == ref.TEAM_HAPPY  # the viewer, in "my" colour for either team
    assert tuple(img[119, 128]) == ref.FRONT and tuple(img[136, 128]) == ref.TEAM_HAPPY       # the front stripe is ABOVE the centre, not below
    assert tuple(img[118, 128]) == ref.BLACK and tuple(img[117, 128]) == ref.BACKGROUND       # its outline, then the field
    assert tuple(img[77, 128]) == swap(ref.BALL_POS) and tuple(img[178, 128]) != swap(ref.BALL_POS)  # the ball ahead: above the centre
    assert tuple(img[127, 178]) == swap(ref.BALL_NEG) and tuple(img[127, 77]) != swap(ref.BALL_NEG)  # the ball on the +v side: to the right
    assert _pixel_of(pose, *b[0, :2]) in ((77, 128), (78, 128), (77, 127), (78, 127)) and _pixel_of(pose, *b[5, :2])[1] in (177, 178)
    assert tuple(img[57, 128]) == ego.OUTSIDE and tuple(img[0, 128]) == ego.OUTSIDE  # beyond the wall it faces (70.5 and 127.5 ahead)
    row, col = _pixel_of(pose, *goal_pt)
    assert 0 <= row < PX and 0 <= col < PX and tuple(img[row, col]) == swap(goal_col), (row, col)
    assert tuple(ego.frame(800.0, 800.0, 2, 4, r, b, viewer, PX, PX, 1, float(PX), 0.0, True)[0][row, col]) == swap(goal_col)


def test_relative_colours_are_the_absolute_frame_with_the_three_pairs_swapped(golden_dir):
    st = _states(golden_dir, "G")
    n = len(st["step"])
    for v in range(4):
        absolute = emu.render("G", st["robots"], st["balls"], 64, 64, 1, 400.0, 0.0, viewers=[v] * n, relative=False)
        relative = emu.render("G", st["robots"], st["balls"], 64, 64, 1, 400.0, 0.0, viewers=[v] * n, relative=True)
        if v < 2:
            assert np.array_equal(relative, absolute)  # a happy viewer: the flag changes nothing
        else:
            assert np.array_equal(relative, ego.swap_palette(absolute)) and not np.array_equal(relative, absolute)


@pytest.mark.parametrize("S", [1, 4])
def test_planar_is_the_interleaved_frame_permuted(golden_dir, S):
    st = _states(golden_dir, "G")
    viewers = np.arange(len(st["step"])) % 4
    kw = dict(viewers=viewers, relative=True)
    inter = emu.render("G", st["robots"], st["balls"], 64, 48, S, 400.0, 100.0, **kw)
    planar = emu.render("G", st["robots"], st["balls"], 64, 48, S, 400.0, 100.0, planar=True, **kw)
    assert planar.shape == (len(viewers), 3, 48, 64) and np.array_equal(planar, inter.transpose(0, 3, 1, 2))


@pytest.mark.parametrize("S,size", [(2, 32), (4, 24)])
def test_supersampled_frame_is_the_box_filter_of_the_larger_frame_bit_for_bit(golden_dir, S, size):
    st = _states(golden_dir, "G")
    viewers = np.arange(len(st["step"])) % 4
    fine = emu.render("G", st["robots"], st["balls"], size * S, size * S, 1, 400.0, 100.0, viewers=viewers)
    got = emu.render("G", st["robots"], st["balls"], size, size, S, 400.0, 100.0, viewers=viewers)
    assert np.array_equal(got, ref.box_filter(fine, S))
    fine = emu.render("G", st["robots"], st["balls"], 16 * S, 12 * S, 1, 300.0, -20.0, viewers=viewers)  # a non-square frame
    assert np.array_equal(emu.render("G", st["robots"], st["balls"], 16, 12, S, 300.0, -20.0, viewers=viewers), ref.box_filter(fine, S))


def test_indices_out_of_range_and_a_nan_viewer_are_black_frames_and_duplicates_are_equal(golden_dir):
    st = _states(golden_dir, "G")
    n = len(st["robots"])
    robots = st["robots"].copy()
    robots[3, 1, 0] = np.nan   # arena 3: robot 1 has a NaN x, robot 2 a NaN rot, robot 3 an infinite y
    robots[3, 2, 6] = np.nan
    robots[3, 3, 1] = np.inf
    lo, hi = -2 ** 31, 2 ** 31 - 1
    arenas = [n - 1, 0, 0, 5, 3, -1, n, hi, lo, 0, 0, 0, 0, 3, 3, 3, lo, hi]
    viewers = [3, 1, 1, 0, 0, 0, 0, 0, 0, -1, 4, hi, lo, 1, 2, 3, hi, lo]
    for planar in (False, True):
        got = emu.render("G", robots, st["balls"], 64, 48, 1, 400.0, 0.0, arenas=arenas, viewers=viewers, planar=planar)
        assert not got[5:].any()
        assert all(g.any() for g in got[:5])  # arena 3 seen from its finite robot 0 is a picture
        assert np.array_equal(got[1], got[2])
        for k in range(4):
            one = emu.render("G", st["robots"], st["balls"], 64, 48, 1, 400.0, 0.0, arenas=[arenas[k]], viewers=[viewers[k]], planar=planar)
            assert np.array_equal(got[k], one[0])
    # without lists: arena k, robot 0
    base = emu.render("G", st["robots"], st["balls"], 64, 48, 1, 400.0, 0.0)
    assert np.array_equal(base, emu.render("G", st["robots"], st["balls"], 64, 48, 1, 400.0, 0.0, arenas=np.arange(n), viewers=[0] * n))


def test_a_consumed_ball_never_shows_even_in_a_view_that_contains_it():
    r, b = _arena({0: (400.5, 400.5, 10.0), 2: (300.5, 500.5, 100.0)}, {0: (420.0, 380.0)})
    b2 = b.copy()
    b2[3, :2] = (-1000.0, 300.0)   # consumed by goal scoring: parked there, inside a span-4096 view, but OUTSIDE is on top
    b2[4, :2] = (-1003.0, 420.0)
    for span, w in ((4096.0, 512), (4000.0, 64)):
        a = emu.render("G", r[None], b[None], w, w, 1, span, 0.0)
        assert np.array_equal(emu.render("G", r[None], b2[None], w, w, 1, span, 0.0), a)
        assert (a[0] == np.array(ego.OUTSIDE, np.uint8)).all(axis=-1).mean() > 0.9


@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
def test_the_smallest_frame_writes_its_twelve_bytes_and_nothing_else(planar):
    r, b = _arena({0: (400.5, 400.5, 10.0)}, {0: (420.0, 380.0)})
    for fill in (0xAB, 0x54):
        buf = np.full(64, fill, np.uint8)
        got = emu.render("G", r[None], b[None], 4, 1, 1, 100.0, 0.0, planar=planar, out=buf)
        assert (buf[12:] == fill).all()
        assert np.array_equal(got, emu.render("G", r[None], b[None], 4, 1, 1, 100.0, 0.0, planar=planar))


def test_the_emulation_refuses_what_the_entry_refuses():
    r, b = _arena({0: (400.5, 400.5, 10.0)}, {})
    bad = [dict(width=0), dict(width=62), dict(width=1028), dict(height=0), dict(height=1025), dict(samples=3), dict(span=8.0),
           dict(span=20000.0), dict(span=float("nan")), dict(span=float("inf")), dict(ahead=float("nan")), dict(ahead=9000.0), dict(ahead=-9000.0)]
    for kw in bad:
        args = dict(width=64, height=48, samples=1, span=400.0, ahead=0.0)
        args.update(kw)
        buf = np.full(1028 * 1025 * 3 if max(args["width"], args["height"]) > 1000 else 64 * 48 * 3, 0xAB, np.uint8)
        assert emu.render("G", r[None], b[None], rc=True, out=buf, **args) == -1, kw
        assert (buf == 0xAB).all()
