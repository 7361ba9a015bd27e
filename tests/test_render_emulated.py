"""The frame kernel's source (csrc/rr_render.hpp: draw-list builder, shading core, byte packing) compiled with g++ and walked over
k_render's grid on the host (tests/emu/rr_render_emu.cpp), against tests/render_ref.py -- the independent fp64 restatement of the picture
include/roborugby_amd.h specifies -- under that module's rule: exact outside a 1e-3 band around the layer boundaries, at most 0.2 % of a
frame's pixels inside it.  tests/test_gpu_render.py holds the device to the same reference on the same states."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import render_emu_lib as emu
import render_ref as ref

SIZES = {"G": [(800, 800), (96, 96), (64, 48), (4, 4)], "Dwide": [(1000, 640), (96, 64)], "T": [(96, 96)],
         "W": [(96, 96)], "R": [(96, 96)]}  # 11 balls / 8 robots in the draw list (it holds 16 of each kind)


@functools.lru_cache(maxsize=None)
def _states(golden_dir, preset):
    return ref.golden_states(golden_dir, preset)


@functools.lru_cache(maxsize=None)
def _reference(golden_dir, preset, width, height):
    """the reference's frames of a fixture's states, computed once and shared by the fp64 and the fp32 case"""
    cfg, st = ol.PRESETS[preset], _states(golden_dir, preset)
    return [ref.frame(cfg["W"], cfg["H"], cfg["nr_h"], cfg["nb_p"], r, b, width, height) for r, b in zip(st["robots"], st["balls"])]


def _frame_ref(preset, robots, balls, width, height, S=1):
    cfg = ol.PRESETS[preset]
    return ref.frame(cfg["W"], cfg["H"], cfg["nr_h"], cfg["nb_p"], robots, balls, width, height, S)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("preset,size", [(p, s) for p in SIZES for s in SIZES[p]], ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_emulated_source_matches_the_reference_on_recorded_states(golden_dir, preset, size, f32):
    st = _states(golden_dir, preset)
    got = emu.render(preset, st["robots"], st["balls"], size[0], size[1], f32=f32)
    worst = max(ref.check(got[k], want, dist, 1, (preset, size, k)) for k, (want, dist) in enumerate(_reference(golden_dir, preset, *size)))
    print(f"{preset} {size[0]}x{size[1]} {'f32' if f32 else 'f64'} records: {len(got)} frames, worst exempt share {100 * worst:.3f} %")
    if size != (4, 4):
        assert any((f != 255).any() for f in got)  # (not a white sheet)


# ---- crafted arenas (G's shape: 2 + 2 robots, 4 + 4 balls, 800 x 800; native size, so pixel (i, j) is the sample (i + .5, j + .5))
FAR = -1000.0


def _arena(robots, balls, nr=4, nb=8):
    r, b = np.zeros((nr, 10)), np.zeros((nb, 8))
    r[:, 0], r[:, 1] = -5000.0, -5000.0
    b[:, 0], b[:, 1] = FAR, 50.0
    for k, (x, y, rot) in robots.items():
        r[k, 0], r[k, 1], r[k, 6] = x, y, rot
    for k, (x, y) in balls.items():
        b[k, 0], b[k, 1] = x, y
    return r, b


def _native(preset, r, b, f32=False):
    cfg = ol.PRESETS[preset]
    w, h = int(cfg["W"]), int(cfg["H"])
    got = emu.render(preset, r[None], b[None], w, h, f32=f32)[0]
    want, dist = _frame_ref(preset, r, b, w, h)
    ref.check(got, want, dist, 1, preset)
    return got


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_robots_at_four_angles_and_a_ball_on_a_robot(f32):
    r, b = _arena({0: (300.25, 400.25, 0.0), 1: (500.75, 410.125, 45.0), 2: (500.5, 200.25, 90.0), 3: (200.3, 619.6, 359.999)},
                  {0: (300.25, 400.25), 5: (500.5, 200.25)})
    img = _native("G", r, b, f32)
    assert tuple(img[400, 300]) == ref.BALL_POS and tuple(img[200, 500]) == ref.BALL_NEG      # the ball wins over the robot under it
    assert tuple(img[400, 292]) == ref.TEAM_HAPPY and tuple(img[400, 308]) == ref.FRONT         # rot 0: the front is the right side
    assert tuple(img[385, 300]) == ref.TEAM_HAPPY and tuple(img[380, 300]) == ref.BLACK and tuple(img[379, 300]) == ref.BACKGROUND
    assert tuple(img[200, 515]) == ref.TEAM_GRUMPY and tuple(img[192, 500]) == ref.FRONT        # rot 90: long side along x, front up
    assert tuple(img[619, 192]) == ref.TEAM_GRUMPY and tuple(img[619, 208]) == ref.FRONT        # rot 359.999: as good as rot 0


def test_robot_one_is_drawn_over_robot_zero():
    r, b = _arena({0: (400.3, 300.7, 0.0), 1: (403.3, 302.7, 90.0)}, {}, nr=2, nb=2)
    img = _native("D", r, b)
    assert tuple(img[302, 403]) == ref.TEAM_GRUMPY   # robot 1's body, inside robot 0's rectangle
    assert tuple(img[285, 400]) == ref.TEAM_HAPPY    # robot 0 where robot 1 is not
    assert tuple(img[294, 403]) == ref.FRONT         # robot 1's front (up) over robot 0's body


def test_a_robot_across_a_goal_edge_and_the_goals():
    r, b = _arena({0: (120.3, 119.6, 30.0), 2: (680.4, 690.2, 200.0)}, {})
    img = _native("G", r, b)
    assert tuple(img[119, 120]) == ref.TEAM_HAPPY and tuple(img[690, 680]) == ref.TEAM_GRUMPY
    assert tuple(img[10, 10]) == ref.GOAL_GRUMPY and tuple(img[790, 790]) == ref.GOAL_HAPPY
    assert tuple(img[100, 139]) == ref.GOAL_GRUMPY and tuple(img[100, 140]) == ref.BACKGROUND   # 139.5 + 100.5 = 240: closed


def test_a_clipped_ball_a_consumed_ball_and_a_nan_robot_draw_what_is_left_of_them():
    r, b = _arena({0: (400.5, 400.5, 10.0)}, {0: (3.0, 300.5), 1: (400.0, -3.0), 2: (797.5, 803.0)})
    img = _native("G", r, b)
    assert tuple(img[300, 0]) == ref.BALL_POS and tuple(img[300, 9]) == ref.BLACK and tuple(img[300, 10]) == ref.BACKGROUND
    assert tuple(img[0, 400]) == ref.BALL_POS and tuple(img[3, 400]) == ref.BLACK
    # a ball parked at x = -1000 (consumed by goal scoring), a NaN robot and a NaN ball leave the frame as it is without them
    r2, b2 = r.copy(), b.copy()
    b2[3, :2] = (-1000.0, 300.0)
    r2[1, [0, 1, 6]] = (np.nan, 300.0, 10.0)
    r2[2, [0, 1, 6]] = (300.0, 300.0, np.nan)
    r2[3, [0, 1, 6]] = (np.inf, 300.0, 10.0)
    b2[4, :2] = (np.nan, 300.0)
    assert np.array_equal(_native("G", r2, b2), img)
    assert np.array_equal(_native("G", r2, b2, f32=True), img)


@pytest.mark.parametrize("S,size", [(2, 48), (4, 24)])
def test_supersampled_frame_is_the_box_filter_of_the_larger_frame_bit_for_bit(golden_dir, S, size):
    st = _states(golden_dir, "G")
    fine = emu.render("G", st["robots"], st["balls"], 96, 96, 1)
    got = emu.render("G", st["robots"], st["balls"], size, size, S)
    assert np.array_equal(got, ref.box_filter(fine, S))
    for k in range(0, len(got), 5):  # ... and the reference's own supersampled frame, under its rule
        want, dist = _frame_ref("G", st["robots"][k], st["balls"][k], size, size, S)
        ref.check(got[k], want, dist, S, (S, k))


def test_an_arena_index_out_of_range_is_a_black_frame_and_duplicates_are_equal(golden_dir):
    st = _states(golden_dir, "G")
    n = len(st["robots"])
    idx = [n - 1, 0, 0, 5, -1, n, 2 ** 31 - 1, -2 ** 31]
    got = emu.render("G", st["robots"], st["balls"], 64, 48, arenas=idx)
    base = emu.render("G", st["robots"], st["balls"], 64, 48)
    assert not got[4:].any()
    assert np.array_equal(got[1], got[2]) and all(np.array_equal(got[k], base[idx[k]]) for k in range(4))
    assert not (base == 0xAB).all(axis=(1, 2, 3)).any()


def test_the_picture_shows_the_rectangle_robot_corners_draws():
    """the link to the existing host picture: render.robot_corners pulled 10 % toward the centre are on the robot, pushed 10 % outward
    they are on the white field"""
    from roborugby_amd import render
    poses = {0: (300.25, 400.5, 0.0), 1: (500.75, 410.125, 45.0), 2: (500.5, 200.25, 90.0), 3: (200.3, 619.6, 359.999)}
    r, b = _arena(poses, {})
    img = _native("G", r, b)
    for cx, cy, rot in list(poses.values()) + [(600.1, 600.9, 123.4)]:
        if rot == 123.4:
            r, b = _arena({0: (cx, cy, rot)}, {})
            img = _native("G", r, b)
        for x, y in render.robot_corners(cx, cy, rot):
            xi, yi = cx + 0.9 * (x - cx), cy + 0.9 * (y - cy)
            xo, yo = cx + 1.1 * (x - cx), cy + 1.1 * (y - cy)
            assert tuple(img[int(yi), int(xi)]) != ref.BACKGROUND, (cx, cy, rot)
            assert tuple(img[int(yo), int(xo)]) == ref.BACKGROUND, (cx, cy, rot)
