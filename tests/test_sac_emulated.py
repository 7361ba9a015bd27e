"""csrc/rr_sac.hpp's draw and squash, compiled with g++ (tests/emu/rr_sac_emu.cpp), against tests/sac_ref.py: u1 and u2 bit-equal, the
draws, actions and log-probabilities within the GPU tests' bars (4 E, E = the float32 numpy restatement's largest error on the same rows).
The same source runs once as a stand-alone program under AddressSanitizer + UBSan.  CPU only."""
import subprocess

import numpy as np
import pytest

import sac_emu_lib as se
import sac_ref


@pytest.mark.parametrize("seed,call,n", sac_ref.DRAW_SEEDS + ((2, 0xFFFFFFFF, 4096),))
def test_uniforms_bit_equal_and_draws_within_the_bar(seed, call, n):
    u = se.uniforms(seed, n, call)
    assert np.array_equal(u.astype(np.float64), sac_ref.row_uniforms(seed, n, call))
    z = se.draw(seed, n, call)
    z64 = sac_ref.draw64(seed, n, call)
    E = float(np.abs(sac_ref.draw32(seed, n, call) - z64).max())
    err = float(np.abs(z - z64).max())
    print(f"seed {seed:#x} call {call:#x}: emulated draw max err {err:.3g}, E {E:.3g}")
    assert err <= 4 * E


@pytest.mark.parametrize("max_action", [1.0, 0.5])
@pytest.mark.parametrize("A", [2, 4])
def test_squash_within_the_bars(A, max_action):
    n = 4096
    head = sac_ref.case_head64(A)[:n].astype(np.float32)
    z = se.draw(0x1234ABCD00000002, n, 1)[:, :A].copy()
    rc, a, lp = se.squash(head, z, max_action)
    assert rc == 0
    a64, lp64, _ = sac_ref.squash64(head, z, max_action)
    E_a, E_lp = sac_ref.squash_E(head, z, max_action)
    rows = sac_ref.well_conditioned_rows(a64, max_action)
    err_a, err_lp = float(np.abs(a - a64).max()), float(np.abs(lp - lp64)[rows].max())
    print(f"A = {A} max_action {max_action}: actions {err_a:.3g} (E {E_a:.3g}), log_prob {err_lp:.3g} (E {E_lp:.3g}) on {int(rows.sum())}/{n} rows")
    assert err_a <= max(4 * E_a, 2.0 ** -22 * max_action)
    assert err_lp <= 4 * E_lp
    assert np.all(np.isfinite(lp))


def test_clamp_arms_and_refusals():
    head = np.array([[0.25, -0.5, -1.0, 7.0]], np.float32)   # A = 2: sigma raw -1 -> 1e-6, 7 -> exactly 1
    z = np.array([[1.5, -2.0]], np.float32)
    rc, a, lp = se.squash(head, z)
    assert rc == 0
    assert abs(float(a[0, 0]) - np.tanh(0.25 + 1e-6 * 1.5)) <= 2.0 ** -23
    assert abs(float(a[0, 1]) - np.tanh(-0.5 + 1.0 * -2.0)) <= 2.0 ** -23
    assert se.squash(np.zeros((1, 6), np.float32), np.zeros((1, 3), np.float32))[0] == -1  # A = 3


def test_sanitizer_program_runs_clean(tmp_path):
    """the same source with its own main under AddressSanitizer + UBSan: every input and output a heap block of exactly its size"""
    exe = se.build_program(str(tmp_path / "rr_sac_emu_san"), extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "rr_sac_emu:" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
