"""Provenance of tests/golden/hive_{G,X}.npz: where the reference tree is present the generator (tools/gen_hive_golden.py) is run
again -- one fresh process per preset, its own invocation line -- into a scratch directory and must reproduce the committed file
array for array.  Skipped where the reference does not exist (the GPU box)."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle", "refgen"))
from load_reference import reference_available  # noqa: E402  (reads no reference code: only checks that the tree exists)

pytestmark = pytest.mark.skipif(not reference_available(), reason="reference tree not present")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("preset", ["G", "X"])
def test_generator_reproduces_the_committed_hive_fixture(tmp_path, golden_dir, preset):
    env = dict(os.environ, RR_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(REPO, "tools", "gen_hive_golden.py"), preset], env=env,
                          stdout=subprocess.DEVNULL, timeout=540)
    name = f"hive_{preset}.npz"
    new, old = np.load(tmp_path / name), np.load(os.path.join(golden_dir, name))
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        if k == "meta":
            continue
        assert np.array_equal(new[k], old[k], equal_nan=(new[k].dtype.kind == "f")), k
    assert os.path.getsize(os.path.join(golden_dir, name)) < (1 << 20)
