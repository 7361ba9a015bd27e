"""The kernels of roborugby_amd/csrc/rr_dqn.hip against independent references (tests/dqn_ref.py: fp64 forward, fp64 Adam, a plain
Philox, a row-by-row ring store; fp64 autograd for the gradient) at the shapes tests/test_gpu_dqn_fused.py leaves out: uneven tile
splits and more than two tiles per workgroup (RR_DQN_WGS), batch_index = NULL, the act kernel's qvalues and ties, the epsilon draw
bit for bit, the store kernel beyond one chunk per scan thread and at its edges, the Adam step isolated from the gradient, and the
argument guards.  Where dqn.py does not expose an argument (qvalues, batch_index = NULL, count_out, mem_cntr) the C ABI is called
through ctypes, as a C caller would.  A case sizes every buffer for the n it passes."""
import copy
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import dqn_ref  # noqa: E402
from test_gpu_dqn_fused import _agent, _rows_off_the_relu_knife_edge, _torch_grads  # noqa: E402

DEV = "cuda:0"
GRAD_NAMES = ("fc2.weight", "fc1.weight", "fc3.weight", "fc1.bias", "fc2.bias", "fc3.bias")  # the handle's flat order (rr_dqn_grads)
U = 2.0 ** -24      # largest relative error of one fp32 rounding to nearest
TINY = 2.0 ** -149  # ... and its absolute error where the result is subnormal


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _small_agent(seed=2, **kw):
    from roborugby_amd.dqn import BatchedDQNAgent
    ag = BatchedDQNAgent(batch_size=64, device=DEV, seed=seed, max_mem_size=64, **kw)
    assert ag.fused
    return ag


def _last_error(ag):
    return ag._rrlib.rr_dqn_last_error() or b""


# ------------------------------------------------------------------------------------------------------------ A. gradient
def _grads_flat(ag, idx, null_index=False):
    """rr_dqn_grads through the C ABI: (flat gradient [param_count], loss); the output starts as NaN so an unwritten entry shows"""
    flat = torch.full((ag._rrlib.rr_dqn_param_count(),), float("nan"), device=DEV)
    ag._fused_loss.fill_(float("nan"))
    args = ag._fused_args(idx)
    if null_index:
        args.batch_index = None
    rc = ag._rrlib.rr_dqn_grads(ag._fused_h, C.byref(args), _ptr(flat), _stream())
    assert rc == 0, _last_error(ag)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(flat).any())
    return flat, float(ag._fused_loss[0])


def _split(ag, flat):
    shapes, out, off = dict(ag.Q_eval.named_parameters()), {}, 0
    for nm in GRAD_NAMES:
        k = shapes[nm].numel()
        out[nm] = flat[off:off + k].view_as(shapes[nm])
        off += k
    assert off == flat.numel()
    return out


def _assert_gradient(label, got, loss, ref, ref_loss, t32):
    """the yardstick of test_fused_gradient_matches_autograd, unchanged: fp64 autograd is the reference"""
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (label, loss, ref_loss)
    for k in ref:
        scale = float(ref[k].abs().max())
        err = float((got[k].double() - ref[k]).abs().max())
        err32 = float((t32[k].double() - ref[k]).abs().max())
        print(f"  {label} {k}: fused {err / scale:.2e}, fp32 autograd {err32 / scale:.2e} of the gradient's scale (vs fp64 autograd)")
        assert scale > 0 and err <= max(1e-5 * scale, 1.25 * err32), (label, k, err, err32, scale)


def _check_against_autograd(label, ag, idx, null_index=False, ref_rows=None):
    ref_rows = idx if ref_rows is None else ref_rows
    ref, ref_loss = _torch_grads(ag, ref_rows, torch.float64)
    t32, _ = _torch_grads(ag, ref_rows, torch.float32)
    flat, loss = _grads_flat(ag, idx, null_index)
    _assert_gradient(label, _split(ag, flat), loss, ref, ref_loss, t32)
    return flat, loss


def _grid_agent(monkeypatch, wgs, tiles):
    """an agent whose handle was created under RR_DQN_WGS = wgs (None: unset, one workgroup per CU), and `tiles` 64-sample tiles of rows"""
    if wgs is None:
        monkeypatch.delenv("RR_DQN_WGS", raising=False)
    else:
        monkeypatch.setenv("RR_DQN_WGS", str(wgs))  # read by getenv in rr_dqn_create
    batch = 64 * tiles
    ag, g = _agent(batch)
    assert ag.fused
    return ag, g, _rows_off_the_relu_knife_edge(ag, g, batch)


# (RR_DQN_WGS, tiles): the default grid with half of the workgroups at two tiles and half at one; 4 + 3 + 3 tiles; one workgroup
# with seven tiles (the longest sequential fp32 accumulation: 448 samples in the register accumulators); fewer tiles than workgroups
GRIDS = [(None, None), (3, 10), (1, 7), (5, 3)]


@pytest.mark.parametrize("wgs,tiles", GRIDS, ids=["default-1.5-tiles-per-cu", "wgs3-10-tiles", "wgs1-7-tiles", "wgs5-3-tiles"])
def test_gradient_at_uneven_and_deep_tile_splits(monkeypatch, wgs, tiles):
    tiles = tiles or (_cus() + _cus() // 2)
    ag, g, idx = _grid_agent(monkeypatch, wgs, tiles)
    _check_against_autograd(f"WGS={wgs} tiles={tiles}", ag, idx)


def test_null_batch_index_reads_rows_0_to_batch(monkeypatch):
    """the chosen rows copied to the front of the five memories: batch_index = arange(B) and batch_index = NULL are the same batch, so
    the two results must agree bit for bit (and with fp64 autograd) -- 4 + 3 + 3 tiles, so a NULL path that reads a wrong row shows"""
    ag, g, idx = _grid_agent(monkeypatch, 3, 10)
    B = idx.numel()
    for name in dqn_ref.MEMORIES:
        mem = getattr(ag, name)
        mem[:B] = mem[idx]
    front = torch.arange(B, device=DEV)
    with_idx, loss_idx = _check_against_autograd("arange", ag, front)
    with_null, loss_null = _check_against_autograd("NULL", ag, front, null_index=True)
    assert torch.equal(with_idx, with_null) and loss_idx == loss_null


def test_a_row_repeated_64_times_gives_that_samples_gradient():
    ag, g = _agent(64)
    rows = _rows_off_the_relu_knife_edge(ag, g, 64)
    row = rows[~ag.terminal_memory[rows]][:1].contiguous()  # (not terminal: the bootstrap term is part of what is checked)
    assert row.numel() == 1
    # the mean over 64 copies is the sample's own gradient: the reference is autograd on the single sample
    _check_against_autograd("64 x one row", ag, row.repeat(64).contiguous(), ref_rows=row)


def test_one_sampled_action_leaves_the_other_fc3_rows_exactly_zero(monkeypatch):
    ag, g, idx = _grid_agent(monkeypatch, 3, 10)
    ag.action_memory.fill_(5)
    flat, _ = _check_against_autograd("all actions 5", ag, idx)
    got = _split(ag, flat)
    others = [a for a in range(8) if a != 5]
    assert bool((got["fc3.weight"][others] == 0.0).all()) and bool((got["fc3.bias"][others] == 0.0).all())
    assert float(got["fc3.weight"][5].abs().max()) > 0.0 and float(got["fc3.bias"][5].abs()) > 0.0


def test_all_terminal_and_gamma_zero_both_regress_on_the_reward(monkeypatch):
    """every row terminal, and gamma = 0: the target is the reward alone, so both are the gradient of MSE(Q(s)[a], r) -- against fp64
    autograd of exactly that, and the two fused results against each other bit for bit"""
    ag, g, idx = _grid_agent(monkeypatch, 3, 10)

    def regress(dtype):
        net = copy.deepcopy(ag.Q_eval).to(dtype)
        x = ag.state_memory[idx].to(dtype)
        q = net.fc3(torch.relu(net.fc2(torch.relu(net.fc1(x))))).gather(1, ag.action_memory[idx].view(-1, 1)).squeeze(1)
        loss = torch.nn.functional.mse_loss(q, ag.reward_memory[idx].to(dtype))
        loss.backward()
        return {k: p.grad.clone() for k, p in net.named_parameters()}, float(loss.detach())
    ref, ref_loss = regress(torch.float64)
    t32, _ = regress(torch.float32)
    terminal = ag.terminal_memory.clone()
    ag.terminal_memory.fill_(True)
    flat_t, loss_t = _grads_flat(ag, idx)
    _assert_gradient("all terminal", _split(ag, flat_t), loss_t, ref, ref_loss, t32)
    ag.terminal_memory.copy_(terminal)
    assert not bool(ag.terminal_memory[idx].all())
    ag.gamma = 0.0
    flat_g, loss_g = _grads_flat(ag, idx)
    _assert_gradient("gamma = 0", _split(ag, flat_g), loss_g, ref, ref_loss, t32)
    assert torch.equal(flat_t, flat_g) and loss_t == loss_g


def test_grads_is_deterministic_and_touches_no_state(monkeypatch):
    """the reduction is in workgroup order (no atomics): the same call twice gives the same bits; rr_dqn_grads leaves the six parameter
    tensors, both Adam moments and the step count as they were (the moments made non-trivial by one update first)"""
    tiles = _cus() + _cus() // 2
    ag, g, idx = _grid_agent(monkeypatch, None, tiles)
    assert ag._rrlib.rr_dqn_update(ag._fused_h, C.byref(ag._fused_args(idx)), _stream()) == 0
    torch.cuda.synchronize()
    params = [p.detach().clone() for p in ag.Q_eval.parameters()]
    target = [p.detach().clone() for p in ag.Q_target.parameters()]
    adam = ag._fused_adam()
    assert adam["step"] == 1 and float(adam["exp_avg"].abs().max()) > 0.0
    first, loss1 = _grads_flat(ag, idx)
    second, loss2 = _grads_flat(ag, idx)
    assert torch.equal(first, second) and loss1 == loss2
    after = ag._fused_adam()
    assert after["step"] == 1 and torch.equal(after["exp_avg"], adam["exp_avg"]) and torch.equal(after["exp_avg_sq"], adam["exp_avg_sq"])
    for p, q in zip(list(ag.Q_eval.parameters()) + list(ag.Q_target.parameters()), params + target):
        assert torch.equal(p.detach(), q)


# ------------------------------------------------------------------------------------------- B. act kernel: forward and argmax
def _act(ag, params, obs, epsilon, seed=0, call=1, want_q=True):
    """rr_dqn_act through the C ABI; actions start as -7 and qvalues as NaN, so a row no workgroup wrote shows"""
    n = obs.shape[0]
    actions = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    q = torch.full((n, 8), float("nan"), device=DEV) if want_q else None
    ptrs = (C.c_void_p * 6)(*[p.data_ptr() for p in params])
    rc = ag._rrlib.rr_dqn_act(ag._fused_h, C.byref(ptrs), _ptr(obs), n, epsilon, seed, call, _ptr(actions), _ptr(q), _stream())
    assert rc == 0, _last_error(ag)
    torch.cuda.synchronize()
    a = actions.cpu().numpy()
    assert a.min() >= 0 and a.max() <= 7, "a row of `actions` was not written (or holds no action)"
    if want_q:
        assert not bool(torch.isnan(q).any()), "a row of `qvalues` was not written"
    return a, (q.cpu().numpy() if want_q else None)


def _obs(n, seed=8):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(n, 11, generator=g, device=DEV) * 360.0 - 50.0  # scaled like _agent's replay rows


def _params(ag):
    return [p.detach() for p in ag.Q_eval.parameters()]


def _assert_forward_and_argmax(label, ag, obs, a, q):
    q64 = dqn_ref.forward64(_params(ag), obs).numpy()
    with torch.no_grad():
        q32 = ag.Q_eval(obs).double().cpu().numpy()
    err, err32, scale = float(np.abs(q - q64).max()), float(np.abs(q32 - q64).max()), float(np.abs(q64).max())
    print(f"  {label}: act kernel {err / scale:.2e}, torch fp32 forward {err32 / scale:.2e} of max |q| = {scale:.3g} (vs fp64 forward)")
    assert err <= max(1e-5 * scale, 1.25 * err32), (label, err, err32, scale)
    assert np.array_equal(a, dqn_ref.first_argmax(q)), label  # every row, the kernel's own Q values: no exceptions


@pytest.mark.parametrize("wgs,n", [(None, 64), (None, None), (None, 65536), (2, 64 * 9)], ids=["n64", "one-tile-more-than-cus", "n65536", "wgs2-9-tiles"])
def test_act_qvalues_match_fp64_forward_and_actions_are_their_first_argmax(monkeypatch, wgs, n):
    n = n or 64 * (_cus() + 1)  # one workgroup takes a second tile
    if wgs is None:
        monkeypatch.delenv("RR_DQN_WGS", raising=False)
    else:
        monkeypatch.setenv("RR_DQN_WGS", str(wgs))  # 5 + 4 tiles on two workgroups
    ag = _small_agent()
    obs = _obs(n)
    a, q = _act(ag, _params(ag), obs, 0.0)
    _assert_forward_and_argmax(f"WGS={wgs} n={n}", ag, obs, a, q)
    a_null, _ = _act(ag, _params(ag), obs, 0.0, want_q=False)  # qvalues = NULL: the same actions
    assert np.array_equal(a, a_null)


def test_act_takes_the_first_of_equal_maxima():
    ag = _small_agent()
    obs = _obs(64 * (_cus() + 1))
    params = [p.clone() for p in _params(ag)]
    params[4].zero_()  # fc3.weight = 0: Q is fc3.bias in every row, exactly
    for bias, want in (([1, 3, 3, 0, 3, -1, 3, 2], 1), ([2.5] * 8, 0), ([-1, -1, -4, -1, -1, -1, -1, -1], 0), ([0, 0, 0, 0, 0, 0, 0, 1], 7)):
        params[5].copy_(torch.tensor(bias, dtype=torch.float32))
        a, q = _act(ag, params, obs, 0.0)
        assert np.array_equal(q, np.tile(np.array(bias, dtype=np.float32), (obs.shape[0], 1)))
        assert (a == want).all(), (bias, np.unique(a))


# ------------------------------------------------------------------------------------------------------ C. epsilon draw, exactly
SEED_HI = (0x1234ABCD << 32) | 2  # same low word as seed 2


def _expected_actions(q, seed, call, epsilon):
    u, rand = dqn_ref.act_draw_rows(seed, q.shape[0], call)
    explore = u <= np.float32(epsilon)  # fp32 compare, as the kernel's
    return np.where(explore, rand, dqn_ref.first_argmax(q)).astype(np.int32), explore


@pytest.mark.parametrize("seed,call", [(2, 1), (SEED_HI, 1), (SEED_HI, 0xFFFFFFFF), (2 ** 64 - 1, 7)],
                         ids=["seed2-call1", "seed-above-2^32-call1", "seed-above-2^32-call-0xffffffff", "seed-all-ones-call7"])
def test_epsilon_draw_is_philox_of_seed_row_call(seed, call):
    ag = _small_agent()
    obs = _obs(64 * (_cus() + 1))
    a, q = _act(ag, _params(ag), obs, 0.3, seed=seed, call=call)
    want, explore = _expected_actions(q, seed, call, 0.3)
    assert np.array_equal(a, want), (seed, call, int((a != want).sum()))
    assert abs(float(explore.mean()) - 0.3) < 0.03 and int((a != dqn_ref.first_argmax(q)).sum()) > 0  # (the check is not vacuous)
    ones, q1 = _act(ag, _params(ag), obs, 1.0, seed=seed, call=call)  # epsilon = 1: every row explores
    assert np.array_equal(ones, dqn_ref.act_draw_rows(seed, obs.shape[0], call)[1]) and np.array_equal(q1, q)


def test_the_high_word_of_the_seed_and_the_call_change_the_draws():
    ag = _small_agent()
    obs = _obs(64 * 8)
    base, _ = _act(ag, _params(ag), obs, 1.0, seed=2, call=1)
    for seed, call in ((SEED_HI, 1), (2, 2), (3, 1)):
        other, _ = _act(ag, _params(ag), obs, 1.0, seed=seed, call=call)
        assert not np.array_equal(base, other), (seed, call)


def test_choose_action_draws_with_the_incremented_call_counter_and_a_restored_agent_continues_the_stream():
    ag = _small_agent(seed=SEED_HI)
    obs = _obs(64 * (_cus() + 1))
    _, q = _act(ag, _params(ag), obs, 0.0)
    assert ag._act_calls == 0
    for start in (0, 41, 0xFFFFFFFF + 5):  # the counter is kept whole and its low 32 bits are passed
        ag._act_calls = start
        a = ag.choose_action(obs, epsilon_override=0.3)
        torch.cuda.synchronize()
        assert ag._act_calls == start + 1 and a.dtype == torch.int32
        want, _ = _expected_actions(q, SEED_HI, (start + 1) & 0xFFFFFFFF, 0.3)
        assert np.array_equal(a.cpu().numpy(), want), start
    ag._act_calls = 41
    ag.choose_action(obs, epsilon_override=0.3)
    twin = _small_agent(seed=SEED_HI)  # (the seed is a constructor argument, the counter travels in the checkpoint)
    twin.load_state_dict(ag.state_dict())
    assert twin._act_calls == 42
    nxt, nxt_twin = ag.choose_action(obs, epsilon_override=0.3), twin.choose_action(obs, epsilon_override=0.3)
    torch.cuda.synchronize()
    assert torch.equal(nxt, nxt_twin)
    assert np.array_equal(nxt.cpu().numpy(), _expected_actions(q, SEED_HI, 43, 0.3)[0])


# ------------------------------------------------------------------------------------------------------------ D. store kernel
def _store_case(ag, label, n, mem_size, mem_cntr, valid, seed=0):
    """one rr_dqn_store call into sentinel-filled memories against dqn_ref.ring_store: all five memories bit for bit (so the rows
    the call must not touch are checked too) and count_out.  valid: None, or a bool array [n]."""
    g = torch.Generator(device=DEV).manual_seed(1000 + seed)
    s, s2 = torch.rand(n, 11, generator=g, device=DEV), torch.rand(n, 11, generator=g, device=DEV)
    a = torch.randint(0, 8, (n,), generator=g, device=DEV, dtype=torch.int32)
    r, d = torch.randn(n, generator=g, device=DEV), torch.rand(n, generator=g, device=DEV) < 0.3
    v = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, dtype=np.bool_)).to(DEV)
    # sentinels no transition holds: negative states / rewards that differ from row to row, action -1 - row, terminal byte 7
    mem = dict(state_memory=-1.0 - torch.arange(mem_size * 11, device=DEV, dtype=torch.float32).view(mem_size, 11),
               new_state_memory=-0.5 - torch.arange(mem_size * 11, device=DEV, dtype=torch.float32).view(mem_size, 11),
               action_memory=-1 - torch.arange(mem_size, device=DEV, dtype=torch.int64),
               reward_memory=1e6 + torch.arange(mem_size, device=DEV, dtype=torch.float32),
               terminal_memory=torch.full((mem_size,), 7, device=DEV, dtype=torch.uint8))
    before = {k: t.cpu().numpy() for k, t in mem.items()}
    count = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    rc = ag._rrlib.rr_dqn_store(ag._fused_h, _ptr(s), _ptr(a), _ptr(r), _ptr(s2), _ptr(d), _ptr(v), n, mem_cntr, mem_size,
                                _ptr(mem["state_memory"]), _ptr(mem["new_state_memory"]), _ptr(mem["action_memory"]),
                                _ptr(mem["reward_memory"]), _ptr(mem["terminal_memory"]), _ptr(count), _stream())
    assert rc == 0, (label, _last_error(ag))
    torch.cuda.synchronize()
    want, cntr = dqn_ref.ring_store(before, mem_cntr, mem_size, (s.cpu().numpy(), a.cpu().numpy(), r.cpu().numpy(), s2.cpu().numpy(),
                                                                d.cpu().numpy()), valid)
    n_valid = n if valid is None else int(np.count_nonzero(valid))
    assert cntr - mem_cntr == n_valid
    assert int(count[0]) == n_valid, (label, int(count[0]), n_valid)
    for k in dqn_ref.MEMORIES:
        got = mem[k].cpu().numpy()
        assert got.dtype == want[k].dtype and got.tobytes() == want[k].tobytes(), (label, k, int((got != want[k]).sum()))
    if n_valid == 0:
        assert all(before[k].tobytes() == mem[k].cpu().numpy().tobytes() for k in dqn_ref.MEMORIES)


def _mask(n, seed, p=0.9):
    return np.random.default_rng(seed).random(n) < p


def test_store_at_chunk_edges_and_degenerate_masks():
    ag = _small_agent()
    for n in (1, 63, 64, 65):
        _store_case(ag, f"n={n} all", n, 500, 0, None, seed=n)
        _store_case(ag, f"n={n} masked", n, 500, 3, _mask(n, n, 0.7), seed=n)
        _store_case(ag, f"n={n} none valid", n, 500, 7, np.zeros(n, dtype=bool), seed=n)
        last = np.zeros(n, dtype=bool)
        last[-1] = True
        _store_case(ag, f"n={n} last row only", n, 500, 499, last, seed=n)


def test_store_wraps_inside_a_chunk_fills_the_ring_and_takes_a_64_bit_counter():
    ag = _small_agent()
    # ring position 1000 is reached by row 100: lane 36 of the second 64-row chunk
    _store_case(ag, "wrap mid-chunk", 300, 1000, 900, None, seed=1)
    _store_case(ag, "wrap mid-chunk, masked", 300, 1000, 900 + 1000 * 7, _mask(300, 5), seed=2)
    _store_case(ag, "n == mem_size", 1000, 1000, 137, None, seed=3)
    _store_case(ag, "n == mem_size, masked", 1000, 1000, 137, _mask(1000, 6), seed=4)
    _store_case(ag, "mem_cntr > 2^32", 3000, 10_000, 5_000_000_000 + 17, _mask(3000, 7), seed=5)
    _store_case(ag, "mem_cntr > 2^32, wraps", 3000, 10_000, 5_000_000_000 + 9_000, None, seed=6)


def test_store_with_two_chunks_per_scan_thread():
    """n > 65,536: k_dqn_store_scan's 1,024 threads take two 64-row chunks each (config 5 at 131,072 arenas stores this way)"""
    ag = _small_agent()
    n, mem_size = 65_536 + 64 + 1, 200_000
    _store_case(ag, "all valid", n, mem_size, 12_345, None, seed=1)
    _store_case(ag, "90 % valid", n, mem_size, 199_000, _mask(n, 11), seed=2)
    holes = _mask(n, 12)
    for ch in (0, 1, 2, 5, 500, 501, 1023, 1024, 1025):  # whole chunks without a valid row: first / second chunk of a scan thread, the tail
        holes[64 * ch:64 * (ch + 1)] = False
    holes[64 * 700:64 * 760] = False
    _store_case(ag, "whole chunks invalid", n, mem_size, 150_000, holes, seed=3)
    _store_case(ag, "none valid", n, mem_size, 5, np.zeros(n, dtype=bool), seed=4)
    _store_case(ag, "a small call after a large one", 65, 500, 0, _mask(65, 13), seed=5)  # (the chunk scratch is larger than this call needs)


# ----------------------------------------------------------------------------------------------------------- E. reduce + Adam
def _flat_params(ag):
    params = list(ag.Q_eval.parameters())
    return torch.cat([params[k].detach().reshape(-1) for k in ag._FUSED_ORDER]).clone()


def _assert_adam_step(label, ag, idx):
    """One rr_dqn_update against dqn_ref.adam64 fed the gradient rr_dqn_grads returns for the same batch and parameters: both sides
    start from the same fp32 g, m, v, p, so every entry is held to the rounding of k_dqn_reduce_adam alone.

    Roundings of the kernel, each at most u = 2^-24 relative to its own result (the library is built with -ffp-contract=off: nothing
    fuses; 1 - beta is exact for beta in [0.5, 1]; division and sqrtf are correctly rounded):
      m' = fl(fl(b1 m) + fl((1 - b1) g))                  3 roundings: |m' - m64| <= 3 u (|b1 m| + |(1 - b1) g|)
                                                          (the two terms may cancel, so the unit is the sum of their magnitudes --
                                                          which is |m'| itself whenever m and g agree in sign or m = 0)
      v' = fl(fl(b2 v) + fl(fl((1 - b2) g) g))            4 roundings, every term >= 0: |v' - v64| <= 4 u v64
      d  = fl(fl(lr / bc1) * fl(m' / fl(fl(fl(sqrt v') / sbc2) + eps)))  with bc1, sbc2 rounded to fp32 by the host: 8 roundings,
           and v' brings 4 u / 2 through the square root: 10 u |d|, + 1 u for the second-order terms, + the error of m' scaled by
           lr / (bc1 denom)
      p' = fl(p - d)                                      1 rounding: u |p'| (half an ulp)
    Results in the subnormal range add 2^-149 per rounding.  lr, betas and eps are the fp32 values the ABI receives.
    Measured on an MI355X: the worst entry sits at 0.32 - 0.63 (m'), 0.48 - 0.68 (v') and 0.82 - 0.95 (p') of these bounds.  Held to
    3 u |m'| alone, the worst entry of m' is at 0.32 at step 1 (m = 0: nothing cancels) and at 425 / 929 / 613 at steps 2 / 3 /
    100,001: fl(b1 m) and fl((1 - b1) g) are each rounded before they cancel, as in any fp32 Adam (printed below, not asserted)."""
    lr, b1, b2, eps = (float(np.float32(x)) for x in (ag._lr, ag._betas[0], ag._betas[1], ag._adam_eps))
    ref_loss = _torch_grads(ag, idx, torch.float64)[1]
    g, _ = _grads_flat(ag, idx)
    before, p0 = ag._fused_adam(), _flat_params(ag)
    ag._fused_loss.fill_(float("nan"))
    rc = ag._rrlib.rr_dqn_update(ag._fused_h, C.byref(ag._fused_args(idx)), _stream())
    assert rc == 0, _last_error(ag)
    torch.cuda.synchronize()
    loss = float(ag._fused_loss[0])
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (label, loss, ref_loss)
    after, p1 = ag._fused_adam(), _flat_params(ag)
    step = before["step"] + 1
    assert after["step"] == step
    p64, m64, v64 = dqn_ref.adam64(p0, g, before["exp_avg"], before["exp_avg_sq"], step, lr, b1, b2, eps)
    g64, m0, p0_64 = g.cpu().double(), before["exp_avg"].cpu().double(), p0.cpu().double()
    bound_m = 3 * U * ((b1 * m0).abs() + ((1.0 - b1) * g64).abs()) + 3 * TINY
    bound_v = 4 * U * v64 + 4 * TINY
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = v64.sqrt() / bc2 ** 0.5 + eps
    bound_p = U * p64.abs() + 11 * U * (p64 - p0_64).abs() + (lr / bc1) / denom * bound_m + TINY
    for name, got, want, bound in (("exp_avg", after["exp_avg"], m64, bound_m), ("exp_avg_sq", after["exp_avg_sq"], v64, bound_v),
                                   ("param", p1, p64, bound_p)):
        err = (got.cpu().double() - want).abs()
        worst = int((err / bound).argmax())
        print(f"  {label} {name}: worst entry at {float(err[worst] / bound[worst]):.3f} of its bound, max |error| {float(err.max()):.3e}")
        assert bool((err <= bound).all()), (label, name, worst, float(err[worst]), float(bound[worst]))
    own = (after["exp_avg"].cpu().double() - m64).abs() / (3 * U * m64.abs() + 3 * TINY)
    print(f"  {label} exp_avg against 3 u |m'| alone (no allowance for cancellation): worst entry at {float(own.max()):.3g}")
    moved = (p1 != p0).float().mean()
    assert float(moved) > 0.5, (label, float(moved))  # (the step is not below half an ulp of the parameters: the check has something to see)


def test_adam_steps_1_2_3_from_a_fresh_handle_match_fp64_adam_entry_by_entry():
    batch = 4096
    ag, g = _agent(batch, seed=3)
    for step in (1, 2, 3):
        idx = torch.randint(0, ag.mem_size, (batch,), generator=g, device=DEV).contiguous()
        _assert_adam_step(f"step {step}", ag, idx)


def test_adam_step_after_restored_moments_at_step_100000():
    """rr_dqn_adam_state(set = 1): random moments (v >= 0) and a step count at which neither beta1^step nor beta2^step is near 1"""
    batch = 4096
    ag, g = _agent(batch, seed=4)
    n = ag._rrlib.rr_dqn_param_count()
    m = torch.randn(n, generator=g, device=DEV) * 1e-3
    v = torch.rand(n, generator=g, device=DEV) * 1e-6
    ag._fused_adam(dict(exp_avg=m, exp_avg_sq=v, step=100_000))
    back = ag._fused_adam()
    assert back["step"] == 100_000 and torch.equal(back["exp_avg"], m) and torch.equal(back["exp_avg_sq"], v)
    idx = torch.randint(0, ag.mem_size, (batch,), generator=g, device=DEV).contiguous()
    _assert_adam_step("step 100,001", ag, idx)


# ------------------------------------------------------------------------------------------------------------------ F. guards
def test_entry_points_reject_misuse_before_any_launch():
    """every call below returns -1 before it launches anything (csrc/rr_dqn.hip: the checks of dqn_run, rr_dqn_act and rr_dqn_store
    precede the first launch), names the reason in rr_dqn_last_error() and leaves outputs, parameters and Adam state as they were.
    Every pointer that is passed is a valid device pointer of sufficient size."""
    ag, g = _agent(128, mem=4096)
    lib, h = ag._rrlib, ag._fused_h
    idx = torch.arange(128, device=DEV)
    params = [p.detach().clone() for p in ag.Q_eval.parameters()]
    flat = torch.full((lib.rr_dqn_param_count(),), 123.0, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        st = ag._fused_adam()
        return (bool((flat == 123.0).all()) and float(ag._fused_loss[0]) == -77.0 and st["step"] == 0
                and float(st["exp_avg"].abs().max()) == 0.0 and all(torch.equal(p.detach(), q) for p, q in zip(ag.Q_eval.parameters(), params)))

    def bad_args(case):
        a = ag._fused_args(idx)
        if case.startswith("batch"):
            a.batch = int(case.split("=")[1])
        elif case == "struct_size":
            a.struct_size += 4
        elif case == "eval param":
            a.eval_params[3] = None
        elif case == "target param":
            a.target_params[0] = None
        return a
    for case, word in (("batch=0", b"multiple of 64"), ("batch=63", b"multiple of 64"), ("batch=100", b"multiple of 64"),
                       ("struct_size", b"struct_size"), ("eval param", b"null parameter"), ("target param", b"null parameter")):
        for fn in ("rr_dqn_grads", "rr_dqn_update"):
            ag._fused_loss.fill_(-77.0)
            a = bad_args(case)
            rc = lib.rr_dqn_grads(h, C.byref(a), _ptr(flat), _stream()) if fn == "rr_dqn_grads" else lib.rr_dqn_update(h, C.byref(a), _stream())
            assert rc == -1 and word in _last_error(ag), (case, fn, rc, _last_error(ag))
            assert untouched(), (case, fn)
    ag._fused_loss.fill_(-77.0)
    assert lib.rr_dqn_grads(h, C.byref(ag._fused_args(idx)), None, _stream()) == -1 and b"null output" in _last_error(ag) and untouched()

    # rr_dqn_act
    obs = _obs(128)
    actions = torch.full((128,), -7, dtype=torch.int32, device=DEV)
    q = torch.full((128, 8), -9.0, device=DEV)
    ptrs = (C.c_void_p * 6)(*[p.data_ptr() for p in ag.Q_eval.parameters()])
    for n, eps, word in ((100, 0.5, b"multiple of 64"), (0, 0.5, b"multiple of 64"), (128, -0.1, b"epsilon"), (128, 1.5, b"epsilon"),
                         (128, float("nan"), b"epsilon")):
        rc = lib.rr_dqn_act(h, C.byref(ptrs), _ptr(obs), n, eps, 1, 1, _ptr(actions), _ptr(q), _stream())
        torch.cuda.synchronize()
        assert rc == -1 and word in _last_error(ag), (n, eps, rc, _last_error(ag))
        assert bool((actions == -7).all()) and bool((q == -9.0).all()), (n, eps)
    nulled = (C.c_void_p * 6)(*[p.data_ptr() for p in ag.Q_eval.parameters()])
    nulled[5] = None
    assert lib.rr_dqn_act(h, C.byref(nulled), _ptr(obs), 128, 0.5, 1, 1, _ptr(actions), _ptr(q), _stream()) == -1
    torch.cuda.synchronize()
    assert b"null parameter" in _last_error(ag) and bool((actions == -7).all()) and bool((q == -9.0).all())

    # rr_dqn_store
    n, mem_size = 128, 100
    s, a32, r = torch.rand(n, 11, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV), torch.rand(n, device=DEV)
    d = torch.zeros(n, dtype=torch.bool, device=DEV)
    mem = [torch.full((n, 11), -3.0, device=DEV), torch.full((n, 11), -3.0, device=DEV), torch.full((n,), -3, dtype=torch.int64, device=DEV),
           torch.full((n,), -3.0, device=DEV), torch.full((n,), 7, dtype=torch.uint8, device=DEV)]  # (n rows each: more than mem_size)
    count = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    for nn, cntr, size in ((0, 0, mem_size), (mem_size + 1, 0, mem_size), (64, -1, mem_size), (64, 0, 0), (-64, 0, mem_size)):
        rc = lib.rr_dqn_store(h, _ptr(s), _ptr(a32), _ptr(r), _ptr(s), _ptr(d), None, nn, cntr, size, *[_ptr(t) for t in mem], _ptr(count), _stream())
        torch.cuda.synchronize()
        assert rc == -1 and b"bad sizes" in _last_error(ag), (nn, cntr, size, rc, _last_error(ag))
        assert int(count[0]) == -5 and all(bool((t == (7 if t.dtype == torch.uint8 else -3)).all()) for t in mem), (nn, cntr, size)


def test_choose_action_off_the_tile_size_takes_the_pytorch_path():
    ag = _small_agent()
    calls = ag._act_calls
    for eps in (0.0, 0.5):
        a = ag.choose_action(_obs(100), epsilon_override=eps)
        assert a.dtype == torch.int32 and a.shape == (100,) and int(a.min()) >= 0 and int(a.max()) <= 7
    assert ag._act_calls == calls  # (the fused kernel's call counter is not spent)
    with torch.no_grad():
        assert torch.equal(ag.choose_action(_obs(100), epsilon_override=0.0).long(), ag.Q_eval(_obs(100)).argmax(dim=1))
