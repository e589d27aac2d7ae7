"""CPU (-m "not gpu"): the four augmentation samplers draw, bit for bit, the records of
tests/golden/augment_records.npz (tests/tools/make_augment_records.py, run at the commit in front
of the host-side tidy-up of augment.py).  Equality is exact: nothing numerical may move."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _load("make_augment_records")


@pytest.mark.parametrize("seed", M.SEEDS)
def test_samplers_draw_the_recorded_records(ua, golden, seed):
    want = golden("augment_records")
    keys = sorted(k[len(f"s{seed}/"):] for k in want.files if k.startswith(f"s{seed}/"))
    got = M.records(ua.augment, seed)
    assert sorted(got) == keys and len(keys) == 32
    for key in keys:
        a, b = got[key], want[f"s{seed}/{key}"]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert np.array_equal(a, b), key


def test_every_member_fires_in_the_fixture(golden):
    """the fixture exercises every branch of the samplers: each of the 22 members fires for at
    least 6 of the 32 samples on both seeds"""
    want = golden("augment_records")
    fired = {k: int(want[k].sum()) for k in want.files if "/applied_" in k}
    assert len(fired) == 22 * len(M.SEEDS)
    assert min(fired.values()) >= 6, min(fired, key=fired.get)
