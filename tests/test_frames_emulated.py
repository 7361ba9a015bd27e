"""The g++ build of csrc/rr_frames.hpp (tests/emu/rr_frames_emu.cpp walks both kernels' grids on the host) against tests/frames_ref.py,
byte for byte, over the case grid tests/test_gpu_frames.py runs on the device; the guards; and the stand-alone sanitizer program."""
import subprocess

import numpy as np
import pytest

import frames_emu_lib as fe
import frames_ref as fr


def _same_ring(a, b, label):
    assert a.head == b.head
    for f in fr.RING_FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (label, f)


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("extra", [1, 3])
@pytest.mark.parametrize("stack", [1, 2, 4])
@pytest.mark.parametrize("fb", [16, 48, 12288])
def test_every_explicit_index_equals_the_reference(fb, stack, extra, rows):
    slots = stack + extra
    rng = np.random.default_rng(fb + 10 * stack + extra + 100 * rows)
    ref, emu = fr.Ring(rows, slots, fb), fr.Ring(rows, slots, fb)
    pushes = 3 * slots + 1
    for n, args in enumerate(fr.random_stream(rng, rows, fb, pushes)):
        fr.push(ref, *args)
        assert fe.push(emu, args[0], None, *args[1:]) == 0
        _same_ring(ref, emu, n)
        if n + 1 in (1, slots, slots + 1, pushes):
            index = fr.every_index(n + 1, rows)
            rc, got = fe.sample(emu, stack, len(index), index=index)
            assert rc == 0
            fr.assert_outputs(got, fr.sample(ref, stack, len(index), index=index), len(index), (n, "explicit"))


@pytest.mark.parametrize("batch", [1, 64, 257])
@pytest.mark.parametrize("density", [1.0, 0.5, 0.02, 0.0])
def test_draw_mode_equals_the_reference(density, batch):
    rows, slots, stack, fb = 37, 9, 4, 48
    rng = np.random.default_rng(int(density * 100) + batch)
    ref, emu = fr.Ring(rows, slots, fb), fr.Ring(rows, slots, fb)
    for args in fr.random_stream(rng, rows, fb, 2 * slots + 3, p_valid=density):
        fr.push(ref, *args)
        assert fe.push(emu, args[0], None, *args[1:]) == 0
    rc, got = fe.sample(emu, stack, batch, seed=2 ** 64 - 3, call=11)
    assert rc == 0
    want = fr.sample(ref, stack, batch, seed=2 ** 64 - 3, call=11)
    fr.assert_outputs(got, want, batch, (density, batch))
    assert int(want["ok"].sum()) == (batch if density == 1.0 else 0 if density == 0.0 else int(want["ok"].sum()))
    rc, again = fe.sample(emu, stack, batch, seed=2 ** 64 - 3, call=11)
    assert all(again[f].tobytes() == got[f].tobytes() for f in fr.OUT_FIELDS)
    if density == 1.0 and batch > 1:
        rc, other = fe.sample(emu, stack, batch, seed=2 ** 64 - 3, call=12)
        assert other["picked"].tobytes() != got["picked"].tobytes()


def test_strided_source_and_bare_pushes():
    rows, stack, fb = 3, 4, 48
    rng = np.random.default_rng(8)
    ref, emu = fr.Ring(rows, 6, fb), fr.Ring(rows, 6, fb)
    for n in range(8):
        obs = rng.integers(0, 256, (rows, stack, fb), dtype=np.uint8)
        meta = fr.random_stream(rng, rows, fb, 1)[0][1:]
        first, rest = (None, (None,) * 4) if n % 3 == 2 else (meta[0], meta[1:])
        fr.push(ref, obs[:, -1], first, *rest)
        assert fe.push(emu, obs, stack * fb, first, *rest, offset=(stack - 1) * fb) == 0
        _same_ring(ref, emu, n)


def test_guards_refuse_and_touch_nothing():
    rows, slots, stack, fb, batch = 5, 6, 4, 48, 4
    rng = np.random.default_rng(1)
    ring = fr.Ring(rows, slots, fb)
    stream = fr.random_stream(rng, rows, fb, 8)
    for args in stream:
        assert fe.push(ring, args[0], None, *args[1:]) == 0
    before = {f: getattr(ring, f).copy() for f in fr.RING_FIELDS}
    src, first, action, reward, done, valid = stream[0]
    wide = np.zeros((rows, fb + 8), np.uint8)

    def pushed(**kw):
        r = fr.Ring(rows, slots, fb)
        r.__dict__.update(ring.__dict__)
        for k in ("rows", "slots", "frame_bytes", "head"):
            if k in kw:
                setattr(r, k, kw.pop(k))
        a = dict(src=src, stride=None, first=first, action=action, reward=reward, done=done, valid=valid, offset=0)
        a.update(kw)
        return fe.push(r, a.pop("src"), a.pop("stride"), **a)

    assert pushed(rows=0) == -1 and pushed(rows=(1 << 22) + 1) == -1
    assert pushed(frame_bytes=0) == -1 and pushed(frame_bytes=40) == -1 and pushed(frame_bytes=(1 << 20) + 16) == -1
    assert pushed(stride=fb - 16) == -1 and pushed(src=wide, stride=fb + 8) == -1
    assert pushed(offset=4) == -1
    assert pushed(slots=1) == -1 and pushed(head=-1) == -1
    assert pushed(action=None) == -1 and pushed(valid=None) == -1 and pushed(action=None, reward=None, done=None) == -1
    for f in fr.RING_FIELDS:
        assert getattr(ring, f).tobytes() == before[f].tobytes(), f

    def sampled(stack=stack, batch=batch, index=None, **kw):
        r = fr.Ring(1, 2, 16)
        r.__dict__.update(ring.__dict__)
        r.__dict__.update(kw)
        rc, out = fe.sample(r, stack, batch, index=index, pad=0)
        fresh = fr.poisoned_outputs(batch, stack, fb, 0)
        assert rc == 0 or all(out[f].tobytes() == fresh[f].tobytes() for f in fr.OUT_FIELDS)
        return rc

    assert sampled() == 0
    assert sampled(stack=0) == -1 and sampled(stack=9) == -1
    assert sampled(slots=4) == -1  # slots < stack + 1
    assert sampled(rows=0) == -1 and sampled(head=-1) == -1 and sampled(slots=1, stack=1) == -1
    assert sampled(head=1) == -1 and sampled(head=0) == -1  # draw mode: an empty window
    assert sampled(head=1, index=np.zeros((batch, 2), np.int64)) == 0  # ... explicit: every row ok = 0
    out = fr.poisoned_outputs(batch, stack, fb, 0)
    assert fe.lib().frames_sample_emu(None, *[None] * 4, rows, fb, slots, 8, stack, batch, None, 0, 0, *[fe._p(out[f]) for f in fr.OUT_FIELDS]) == -1
    assert fe.sample(ring, stack, 0, pad=1)[0] == -1 and fe.sample(ring, stack, (1 << 20) + 1, out=out)[0] == -1
    for f in ("state", "next_state", "action", "ok"):  # a null required output
        holed = dict(out, **{f: None})
        assert fe.lib().frames_sample_emu(*[fe._p(getattr(ring, g)) for g in fr.RING_FIELDS], rows, fb, slots, 8, stack, batch, None, 0, 0,
                                          *[fe._p(holed[g]) for g in fr.OUT_FIELDS]) == -1
    fresh = fr.poisoned_outputs(batch, stack, fb, 0)
    assert all(out[f].tobytes() == fresh[f].tobytes() for f in fr.OUT_FIELDS)


def test_sanitizer_program_runs_clean(tmp_path):
    """the same source with its own main under AddressSanitizer + UBSan: every ring and output a heap block of exactly its size"""
    exe = fe.build_program(str(tmp_path / "rr_frames_emu_san"), extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "rr_frames_emu:" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
