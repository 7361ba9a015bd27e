"""The seeded trace of both DQN agents (tools/agent_trace.py) on the torch path against tests/golden/agent_trace.json, written by the same
tool before BatchedDQNAgent and PixelDQNAgent were folded onto one base: everything that depends on integer arithmetic and the CPU
generator alone -- the actions drawn at epsilon 1, the rows a learn() samples, ring positions and contents, every counter after every
call, the keys and value types of state_dict() -- must be equal; the epsilons agree to 1e-12 (the bar of tests/test_dqn_agent.py: one
math.pow per learn()).  Losses and parameter hashes are not in the fixture: another CPU may round a convolution differently."""
import json
import os
import sys

import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_both_agents_trace_equals_the_recorded_one(golden_dir):
    import agent_trace
    threads = torch.get_num_threads()
    try:
        got = agent_trace.trace("cpu")
    finally:
        torch.set_num_threads(threads)
    with open(os.path.join(golden_dir, "agent_trace.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(got))  # (as the file holds it: tuples are lists)
    assert set(got["exact"]) == set(want["exact"]) == {"vector", "pixel"}
    for kind in ("vector", "pixel"):
        for key in sorted(set(want["exact"][kind]) | set(got["exact"][kind])):
            assert got["exact"][kind].get(key) == want["exact"][kind].get(key), (kind, key)
        eps, floats = want["epsilon"][kind], got["floats"][kind]
        assert len(floats["epsilon"]) == len(eps["after_learn"]) == 3
        for a, b in zip(floats["epsilon"] + [floats["fresh_epsilon"]], eps["after_learn"] + [eps["restored"]]):
            assert abs(a - b) < 1e-12, (kind, a, b)
        assert all(x is not None for x in floats["losses"]) and floats["target_equals_eval"]
        assert floats["fresh_parameters"] == floats["parameters_after_3_updates"] != floats["initial_parameters"]
