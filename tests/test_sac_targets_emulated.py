"""csrc/rr_sac.hpp's per-row arithmetic of rr_sac_targets, compiled with g++ under -Wall -Wextra -Werror (tests/emu/rr_sac_targets_emu.cpp),
against tests/sac_targets_ref.py: the draw on stream word 0x5A7A bit-equal in its uniforms and within 4 E in its normals, the gather's
bounds rule at both ends of the ring, the two closing formulas bit-equal to the float32 numpy restatement.  The same source runs once as
a stand-alone program under AddressSanitizer + UBSan.  CPU only."""
import subprocess

import numpy as np
import pytest

import sac_emu_lib as se
import sac_targets_emu_lib as ste
import sac_targets_ref as tr


def test_stream_word():
    assert ste.stream_word() == tr.TARGETS_STREAM == 0x5A7A


@pytest.mark.parametrize("seed,call,n", tr.GPU_DRAWS + ((0, 1, 4096),))
def test_uniforms_bit_equal_and_draws_within_the_bar(seed, call, n):
    u = ste.uniforms(seed, n, call)
    assert np.array_equal(u.astype(np.float64), tr.row_uniforms(seed, n, call))
    z = ste.draw(seed, n, call)
    z64 = tr.draw64(seed, n, call)
    E = float(np.abs(tr.draw32(seed, n, call) - z64).max())
    err = float(np.abs(z - z64).max())
    print(f"seed {seed:#x} call {call:#x}: emulated draw max err {err:.3g}, E {E:.3g}")
    assert err <= 4 * E


def test_the_stream_argument_defaults_to_the_acting_word():
    assert np.array_equal(ste.draw(2, 256, 7, stream_default=True), se.draw(2, 256, 7))
    assert not np.array_equal(ste.draw(2, 256, 7), se.draw(2, 256, 7))


def test_bounds_rule_at_both_ends():
    M = tr.M
    assert np.array_equal(ste.ring_row_ok([-1, 0, M - 1, M], M), [0, 1, 1, 0])
    assert np.array_equal(ste.ring_row_ok([-1, 0, 1, -2 ** 63, 2 ** 63 - 1, 2 ** 32], 1), [0, 1, 0, 0, 0, 0])
    idx = np.arange(-70, M + 70)
    assert np.array_equal(ste.ring_row_ok(idx, M).astype(bool), tr.ring_row_ok(idx, M))


@pytest.mark.parametrize("scale,gamma", [(2.0, 0.99), (3.0, 0.5)])
def test_closing_formulas_bit_equal_to_the_restatement(scale, gamma):
    _, rings, index = tr.case(2)
    reward, terminal = rings[3], rings[4]
    n = 4096
    idx = index[:n].copy()
    idx[5], idx[77] = -1, tr.M
    z = tr.draw32(2, n, 7)
    q1, q2, lp, v = z[:, 0].copy(), z[:, 1].copy(), (3.0 * z[:, 2]).astype(np.float32), (5.0 * z[:, 3]).astype(np.float32)
    rc, vt, qh = ste.close(idx, tr.M, reward, terminal, q1, q2, lp, v, scale, gamma)
    assert rc == 0
    inside = tr.ring_row_ok(idx, tr.M)
    assert list(np.flatnonzero(~inside)) == [5, 77] and np.all(np.isnan(vt[~inside])) and np.all(np.isnan(qh[~inside]))
    safe = np.where(inside, idx, 0)
    want_vt, want_qh = tr.value_target32(q1, q2, lp), tr.q_hat32(scale, reward[safe], gamma, terminal[safe], v)
    assert np.array_equal(vt[inside].view(np.uint32), want_vt[inside].view(np.uint32))
    assert np.array_equal(qh[inside].view(np.uint32), want_qh[inside].view(np.uint32))
    done = inside & terminal[safe]
    assert done.any() and np.array_equal(qh[done], np.float32(scale) * reward[safe][done])  # terminal: exactly fl(reward_scale * r)
    # against float64: one rounding per operation
    t64 = scale * reward[safe].astype(np.float64) + gamma * np.where(terminal[safe], 0.0, v.astype(np.float64))
    assert np.all(np.abs(qh[inside] - t64[inside]) <= 2.0 ** -22 * (np.abs(scale * reward[safe]) + np.abs(gamma * v))[inside] + 1e-30)


def test_refusals():
    one = np.zeros(1, np.float32)
    assert ste.close([0], 0, np.zeros(1), np.zeros(1), one, one, one, one, 2.0, 0.99)[0] == -1


def test_sanitizer_program_runs_clean(tmp_path):
    """the same source with its own main under AddressSanitizer + UBSan: every input and output a heap block of exactly its size"""
    exe = ste.build_program(str(tmp_path / "rr_sac_targets_emu_san"), extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "rr_sac_targets_emu:" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
