"""The yardsticks of tests/test_gpu_dqn_kernels.py (tests/dqn_ref.py) checked on their own, without a GPU: Philox against the
published known answers, the ring store against the agent's PyTorch path, the fp64 forward and Adam against torch itself."""
import numpy as np
import pytest
import torch

import dqn_ref
from roborugby_amd.dqn import BatchedDQNAgent

# Random123 (D. E. Shaw Research) kat_vectors, philox4x32 with 10 rounds: counter, key -> output
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", PHILOX_KAT)
def test_philox_known_answers(counter, key, want):
    assert dqn_ref.philox4x32_10(counter, key) == want
    got = dqn_ref.philox4x32_10_rows(*(np.array([c, c]) for c in counter), *key)
    assert [int(w[1]) for w in got] == list(want)


def test_act_draw_rows_is_act_draw_per_row():
    seed, call, n = (0xDEADBEEF << 32) | 0x12345678, 0xFFFFFFFF, 300
    u, a = dqn_ref.act_draw_rows(seed, n, call)
    assert u.dtype == np.float32 and a.dtype == np.int32
    for i in range(n):
        ui, ai = dqn_ref.act_draw(seed, i, call)
        assert ui == u[i] and ai == a[i]
    # the stream is the Philox output at counter (row, call, 0x0AC7, 0) under key (seed low, seed high)
    w = dqn_ref.philox4x32_10((7, call, 0x0AC7, 0), (0x12345678, 0xDEADBEEF))
    assert dqn_ref.act_draw(seed, 7, call) == (np.float32(w[0]) * np.float32(2.0 ** -32), w[1] & 7)
    assert 0.0 <= float(u.min()) and float(u.max()) <= 1.0 and set(a.tolist()) == set(range(8))
    # word -> u: rounded to nearest in fp32 (the largest word becomes 1.0, never more)
    assert dqn_ref._u_from_word(0xFFFFFFFF) == np.float32(1.0) and dqn_ref._u_from_word(0) == np.float32(0.0)
    assert dqn_ref._u_from_word(0x80000000) == np.float32(0.5)
    # the high word of the seed and the call both matter
    assert not np.array_equal(u, dqn_ref.act_draw_rows(seed & 0xFFFFFFFF, n, call)[0])
    assert not np.array_equal(u, dqn_ref.act_draw_rows(seed, n, 1)[0])


def test_first_argmax_takes_the_first_of_equal_maxima():
    q = np.array([[1, 3, 3, 0, 3, -1, 3, 2], [2, 2, 2, 2, 2, 2, 2, 2], [0, 1, 2, 3, 4, 5, 6, 7], [-1, -2, -3, -1, -5, -1, -7, -8]], dtype=np.float32)
    assert dqn_ref.first_argmax(q).tolist() == [1, 0, 7, 0]
    g = np.random.default_rng(0).standard_normal((1000, 8)).astype(np.float32)
    assert np.array_equal(dqn_ref.first_argmax(g), torch.from_numpy(g).argmax(dim=1).numpy())


def test_ring_store_equals_the_agents_pytorch_path():
    mem_size = 250
    ag = BatchedDQNAgent(device="cpu", fused=False, batch_size=64, max_mem_size=mem_size)
    g = torch.Generator().manual_seed(4)
    mem = {k: getattr(ag, k).numpy().copy() for k in dqn_ref.MEMORIES}
    cntr = 0
    for it, n in enumerate((100, 90, 170, 64, 250, 33, 250, 120)):  # a 250-row ring: wraps three times, one call fills it whole, some store nothing
        s, s2 = torch.rand(n, 11, generator=g), torch.rand(n, 11, generator=g)
        a = torch.randint(0, 8, (n,), generator=g, dtype=torch.int32)
        r, d = torch.randn(n, generator=g), torch.rand(n, generator=g) < 0.2
        v = None if it % 3 == 0 else (torch.rand(n, generator=g) < (0.8 if it % 3 == 1 else 0.0))
        ag.store_transition(s, a, r, s2, d, valid=v)
        mem, cntr = dqn_ref.ring_store(mem, cntr, mem_size, (s.numpy(), a.numpy(), r.numpy(), s2.numpy(), d.numpy()),
                                       None if v is None else v.numpy())
        assert cntr == ag.mem_cntr
        for k in dqn_ref.MEMORIES:
            assert mem[k].dtype == getattr(ag, k).numpy().dtype and np.array_equal(mem[k], getattr(ag, k).numpy()), (it, k)
    assert cntr > 2 * mem_size


def test_forward64_is_the_networks_forward_in_double():
    ag = BatchedDQNAgent(device="cpu", fused=False, seed=3)
    x = torch.rand(200, 11, generator=torch.Generator().manual_seed(1)) * 360.0 - 50.0
    net = ag.Q_eval.double()
    with torch.no_grad():
        want = net.fc3(torch.relu(net.fc2(torch.relu(net.fc1(x.double())))))
    got = dqn_ref.forward64(list(net.parameters()), x)
    assert got.dtype == torch.float64 and got.shape == (200, 8)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_adam64_is_torch_adam_on_doubles():
    g = torch.Generator().manual_seed(2)
    p = torch.randn(500, generator=g, dtype=torch.float64).requires_grad_()
    lr, b1, b2, eps = 5e-4, 0.9, 0.999, 1e-8
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    q, m, v = p.detach().clone(), torch.zeros(500, dtype=torch.float64), torch.zeros(500, dtype=torch.float64)
    for step in (1, 2, 3):
        grad = torch.randn(500, generator=g, dtype=torch.float64) * 10.0 ** float(step - 3)
        p.grad = grad.clone()
        opt.step()
        q, m, v = dqn_ref.adam64(q, grad, m, v, step, lr, b1, b2, eps)
        st = opt.state[p]
        assert float((m - st["exp_avg"]).abs().max()) <= 1e-15 * float(m.abs().max())
        assert float((v - st["exp_avg_sq"]).abs().max()) <= 1e-15 * float(v.abs().max())
        assert float((q - p.detach()).abs().max()) <= 1e-14, step  # steps of ~lr on parameters of ~1
