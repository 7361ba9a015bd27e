"""The yardstick of rr_cnn_act checked on its own (no GPU): tests/cnn_ref.py against PixelQNetwork, the size of the bf16 effect, and --
for every input set tests/test_gpu_cnn_act.py uses -- that the bars made from the reference still discriminate: 4 E stays under 5 % of the
spread of Q across actions, and the rows whose greedy action the contract leaves open (top-two gap <= 8 E) are at most a quarter.
Also the pixel agent's torch path end to end on the CPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cnn_ref  # noqa: E402


def _module(params, channels, dtype):
    from roborugby_amd.dqn import PixelQNetwork
    net = PixelQNetwork(channels).to(dtype)
    with torch.no_grad():
        for p, v in zip(net.parameters(), params):
            p.copy_(torch.as_tensor(v).to(dtype))
    return net


def test_bf16_rounding_known_answers():
    f = lambda bits: np.array([bits], dtype=np.uint32).view(np.float32)  # noqa: E731
    for bits, want in ((0x3F800000, 0x3F800000), (0x3F808000, 0x3F800000),  # tie: to even (down)
                       (0x3F818000, 0x3F820000),                            # tie: to even (up)
                       (0x3F808001, 0x3F810000), (0x3F807FFF, 0x3F800000), (0xBF818000, 0xBF820000), (0x00000000, 0x00000000),
                       (0x7F7FFFFF, 0x7F800000)):                           # the largest fp32 rounds to infinity
        assert cnn_ref.bf16_rne(f(bits)).view(np.uint32)[0] == want, hex(bits)
    x = np.arange(256, dtype=np.float32)
    assert np.array_equal(cnn_ref.bf16_rne(x), x)  # pixels are exact


@pytest.mark.parametrize("channels", [3, 12])
def test_reference_without_roundings_is_the_torch_module(channels):
    params = cnn_ref.make_params(channels, 5, 3.0)
    pixels = cnn_ref.random_images(6, channels, 9)
    q, _ = cnn_ref.forward(params, pixels, "exact")
    with torch.no_grad():
        qt = _module(params, channels, torch.float64)(torch.as_tensor(pixels)).numpy()
    assert np.abs(q - qt).max() <= 1e-12
    # ... and the module takes the eight tensors in the order the kernel is given
    names = [n for n, _ in _module(params, channels, torch.float32).named_parameters()]
    assert names == ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]


@pytest.mark.parametrize("name", sorted(cnn_ref.CASES))
def test_bars_discriminate_on_every_input_set(name):
    ref = cnn_ref.case(name)
    q_exact, _ = cnn_ref.forward(ref.params, ref.pixels, "exact")
    bf16_effect = float(np.abs(q_exact - ref.q).max())
    undecided = 1.0 - float(ref.decided().mean())
    print(f"{name}: E {ref.E:.3g}, E99 {ref.E99:.3g}, floor max {ref.floor.max():.3g}, spread {ref.spread:.3g}, 4E/spread "
          f"{4 * ref.E / ref.spread:.3g}, bf16 effect/spread {bf16_effect / ref.spread:.3g}, rows with gap <= 8E {undecided:.3f}")
    assert ref.spread > 0
    assert bf16_effect < 0.05 * ref.spread
    assert 4 * ref.E < 0.05 * ref.spread
    assert float(ref.bars()[0].max()) < 0.05 * ref.spread
    assert undecided <= 0.25


@pytest.mark.parametrize("channels", [3, 6, 9, 12])
def test_one_pixel_rows_move_q_exactly_where_the_network_looks(channels):
    """a pixel in rows / columns 0..59 moves Q by far more than the bar (so a misplaced read shows); one in 60..63 reaches only conv1's
    last row / column, which conv2 never reads: Q is the all-black Q exactly"""
    ref = cnn_ref.case(f"c{channels}-onepixel")
    black, _ = cnn_ref.forward(ref.params, np.zeros((1, channels, 64, 64), dtype=np.uint8), "A")
    effect = np.abs(ref.q - black).max(axis=1)
    bar = float(ref.bars()[0].max())
    ys, xs = ref.pixels.max(axis=1).reshape(len(effect), -1).argmax(axis=1) // 64, ref.pixels.max(axis=1).reshape(len(effect), -1).argmax(axis=1) % 64
    seen = (ys < 60) & (xs < 60)
    assert seen.sum() >= 40 and (~seen).sum() >= 20
    assert np.all(effect[~seen] == 0.0)
    assert np.all(effect[seen] > 20 * bar), (effect[seen].min(), bar)
    # every residue of the stride, both ends of the channel range
    assert {(int(y) % 4, int(x) % 4) for y, x in zip(ys[seen], xs[seen])} == {(a, b) for a in range(4) for b in range(4)}
    assert ref.pixels[0::2, 0].max() == 255 and ref.pixels[1::2, channels - 1].max() == 255


def test_pixel_agent_torch_path_on_the_cpu():
    from roborugby_amd.dqn import PixelDQNAgent
    n, c = 8, 6
    ag = PixelDQNAgent(channels=c, batch_size=8, max_mem_size=32, device="cpu", seed=3)
    assert not ag.fused
    g = torch.Generator().manual_seed(1)
    s = torch.randint(0, 256, (n, c, 64, 64), dtype=torch.uint8, generator=g)
    s2 = torch.randint(0, 256, (n, c, 64, 64), dtype=torch.uint8, generator=g)
    greedy = ag.choose_action(s, epsilon_override=0.0)
    assert greedy.dtype == torch.int32 and greedy.shape == (n,)
    ref_q, _ = cnn_ref.forward([p.detach().numpy() for p in ag.Q_eval.parameters()], s.numpy(), "exact")
    top = np.sort(ref_q, axis=1)
    sure = (top[:, -1] - top[:, -2]) > 1e-5
    assert np.array_equal(greedy.numpy()[sure], cnn_ref.first_argmax(ref_q)[sure])
    assert torch.equal(ag.choose_action(s.view(4, 2, c, 64, 64), epsilon_override=0.0), greedy)  # [N, R, C, 64, 64] flattens
    a = ag.choose_action(s)  # epsilon = 1: explores
    assert int(a.min()) >= 0 and int(a.max()) <= 7
    valid = torch.tensor([1, 1, 0, 1, 1, 1, 1, 1], dtype=torch.bool)
    ag.store_transition(s, a, torch.arange(n, dtype=torch.float32), s2, torch.zeros(n, dtype=torch.bool), valid=valid)
    assert ag.mem_cntr == 7 and ag.learn() is None
    assert torch.equal(ag.state_memory[2], s[3]) and torch.equal(ag.new_state_memory[6], s2[7]) and float(ag.reward_memory[2]) == 3.0
    ag.store_transition(s, a, torch.ones(n), s2, torch.ones(n, dtype=torch.bool))
    before = [p.detach().clone() for p in ag.Q_eval.parameters()]
    loss = ag.learn()
    assert loss is not None and bool(torch.isfinite(loss)) and ag.updates == 1
    assert any(not torch.equal(p, q) for p, q in zip(ag.Q_eval.parameters(), before))
    assert ag.epsilon < 1.0
    other = PixelDQNAgent(channels=c, batch_size=8, max_mem_size=32, device="cpu", seed=99)
    other.load_state_dict(ag.state_dict())
    assert torch.equal(other.choose_action(s, epsilon_override=0.0), ag.choose_action(s, epsilon_override=0.0))
    assert other._act_calls == ag._act_calls and other.epsilon == ag.epsilon
    with pytest.raises(ValueError):
        ag.choose_action(s[:, :3])
    with pytest.raises(ValueError):
        PixelDQNAgent(channels=c, device="cpu", fused=True)


def test_train_pixels_refuses_a_step_budget():
    from roborugby_amd.dqn import train_pixels
    with pytest.raises(ValueError, match="budget"):
        train_pixels(num_envs=64, steps=1, step_budget_clocks=1000)
