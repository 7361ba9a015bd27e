"""Import the unmodified Python reference from /root/reference -- TEST INFRASTRUCTURE ONLY.

Only usable in the build container (the reference never travels to the GPU
box).  One preset per process: the reference's constants are module globals
(RR_Constants.py:4 `GAME_MODE`), so preset T is obtained by exec-ing the text of
RR_Constants.py with that one assignment flipped into a module object that is
registered before anything else imports it.  Preset D (the 1+1 / 1+1 duel) keeps
GAME_MODE = True and sets the four entity counts of RR_Constants.py:30-34 to 1 the
same way; preset X sets them to 2 + 1 robots and 2 + 3 balls (a shape outside the
library's built list: odd counts, unequal teams), W to 1 + 1 robots and 4 + 7 balls,
R to 4 + 4 robots and 2 + 2 balls (the limits of the one-shape library: 11 balls,
8 robots, 32 ball-robot pairs).  The non-square ids of ARENA
(Dwide: D at 1000 x 640, Ttall: T at 480 x 720) replace the two arena-size
assignments of RR_Constants.py:6-7 the same way, on top of their base preset's
patches; the sizes are integers, as the reference's own are (its reset draws them
through random.randint).  Nothing on disk changes.
"""
import os
import sys
import types

REF_ROOT = os.environ.get("RR_REFERENCE_ROOT", "/root/reference")
# (NUM_ROBOTS_HAPPY, NUM_ROBOTS_GRUMPY, NUM_BALL_POS, NUM_BALL_NEG) patched in; G and T keep the reference's own
COUNTS = {"D": (1, 1, 1, 1), "X": (2, 1, 2, 3), "W": (1, 1, 4, 7), "R": (4, 4, 2, 2)}
BASE = {"Dwide": "D", "Ttall": "T"}                    # preset whose constants and entity counts the id keeps
ARENA = {"Dwide": (1000, 640), "Ttall": (480, 720)}    # (ARENA_WIDTH, ARENA_HEIGHT) patched in; every other id keeps the reference's


def reference_available():
    return os.path.isfile(os.path.join(REF_ROOT, "MyUtils.py"))


def load_reference(preset):
    """Returns a namespace with the reference modules for preset 'G', 'T', 'D', 'X', 'W', 'R' or one of the non-square ids of ARENA."""
    ident, preset = preset, BASE.get(preset, preset)
    assert preset in ("G", "T") or preset in COUNTS
    counts = COUNTS.get(preset, (2, 2, 4, 4) if preset == "G" else (1, 0, 1, 0))
    arena = ARENA.get(ident)
    if not reference_available():
        raise RuntimeError("reference tree not present at %s" % REF_ROOT)
    sys.dont_write_bytecode = True
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import standins
    standins.install()
    if REF_ROOT not in sys.path:
        sys.path.insert(0, REF_ROOT)
    if "robo_rugby.gym_env.RR_Constants" in sys.modules:
        const = sys.modules["robo_rugby.gym_env.RR_Constants"]
        have = (bool(const.GAME_MODE), const.NUM_ROBOTS_HAPPY, const.NUM_ROBOTS_GRUMPY, const.NUM_BALL_POS, const.NUM_BALL_NEG)
        size = (const.ARENA_WIDTH, const.ARENA_HEIGHT)
        if have != (preset != "T",) + counts or size != (arena or ((800, 800) if const.GAME_MODE else (600, 600))):
            raise RuntimeError("reference already loaded with other constants (%s at %d x %d) in this process" % ((have,) + size))
    elif preset != "G":  # (every id of ARENA is based on one of these)
        pkg = types.ModuleType("robo_rugby")
        pkg.__path__ = [os.path.join(REF_ROOT, "robo_rugby")]
        sub = types.ModuleType("robo_rugby.gym_env")
        sub.__path__ = [os.path.join(REF_ROOT, "robo_rugby", "gym_env")]
        path = os.path.join(REF_ROOT, "robo_rugby", "gym_env", "RR_Constants.py")
        text = open(path).read()
        if preset == "T":
            assert text.count("GAME_MODE = True") == 1
            text = text.replace("GAME_MODE = True", "GAME_MODE = False", 1)
        else:  # the four entity counts of COUNTS
            want = dict(zip(("NUM_ROBOTS_HAPPY", "NUM_ROBOTS_GRUMPY", "NUM_BALL_POS", "NUM_BALL_NEG"), counts))
            for name, was in (("NUM_BALL_POS", "4 if GAME_MODE else 1"), ("NUM_BALL_NEG", "4 if GAME_MODE else 0"),
                              ("NUM_ROBOTS_HAPPY", "2 if GAME_MODE else 1"), ("NUM_ROBOTS_GRUMPY", "2 if GAME_MODE else 0")):
                line = f"{name} = {was}"
                assert text.count(line) == 1, line
                text = text.replace(line, f"{name} = {want[name]}", 1)
        if arena:
            for name, value in zip(("ARENA_WIDTH", "ARENA_HEIGHT"), arena):
                line = f"{name} = 800 if GAME_MODE else 600"
                assert text.count(line) == 1, line
                text = text.replace(line, f"{name} = {int(value)}", 1)
        const = types.ModuleType("robo_rugby.gym_env.RR_Constants")
        const.__file__ = path
        exec(compile(text, path, "exec"), const.__dict__)
        sys.modules["robo_rugby"] = pkg
        sys.modules["robo_rugby.gym_env"] = sub
        sys.modules["robo_rugby.gym_env.RR_Constants"] = const
        sub.RR_Constants = const
    import MyUtils
    import robo_rugby.gym_env.RR_Constants as const
    import robo_rugby.gym_env.RR_EnvBase as base
    import robo_rugby.gym_env.RR_TrashyPhysics as tp
    import robo_rugby.gym_env.RR_Environments as envs
    import robo_rugby.gym_env.RR_Robot as robot
    import robo_rugby.gym_env.RR_Ball as ball
    import robo_rugby.gym_env.RR_Goal as goal
    import robo_rugby.gym_env.RR_ScoreKeepers as sk
    import robo_rugby.gym_env.RR_Observers as obs
    assert bool(const.GAME_MODE) == (preset != "T")
    assert (const.NUM_ROBOTS_HAPPY, const.NUM_ROBOTS_GRUMPY, const.NUM_BALL_POS, const.NUM_BALL_NEG) == counts
    assert const.NUM_ROBOTS_TOTAL == counts[0] + counts[1]
    assert arena is None or (const.ARENA_WIDTH, const.ARENA_HEIGHT) == arena
    ns = types.SimpleNamespace(MyUtils=MyUtils, const=const, base=base, tp=tp, envs=envs, robot=robot,
                               ball=ball, goal=goal, sk=sk, obs=obs, preset=ident)
    return ns
