"""bench.py --dump-outputs on CPU tensors: the computational domain of each staggering, float64, within the byte budget, and
the same seeded sample positions in every run (so two builds can be compared value for value)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from mom6_amd import abi  # noqa: E402


def _fields(d):
    g = torch.Generator().manual_seed(5)
    return {"u": torch.randn(d.shape3(), dtype=torch.float64, generator=g),
            "v": torch.randn(d.shape3(), dtype=torch.float64, generator=g),
            "h": torch.randn(d.shape3(), dtype=torch.float64, generator=g),
            "eta_av": torch.randn(d.shape2(), dtype=torch.float64, generator=g)}


def test_dump_whole_domain_when_it_fits(tmp_path):
    d = abi.dims_init(12, 9, 3)
    f = _fields(d)
    shapes = bench.dump_outputs(str(tmp_path), d, f)
    assert shapes == {"u": [3, 9, 13], "v": [3, 10, 12], "h": [3, 9, 12], "eta_av": [9, 12]}
    np.testing.assert_array_equal(np.load(tmp_path / "u.npy"), f["u"][:, d.joff:d.joff + 9, d.ioff - 1:d.ioff + 12].numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "v.npy"), f["v"][:, d.joff - 1:d.joff + 9, d.ioff:d.ioff + 12].numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "eta_av.npy"), f["eta_av"][d.joff:d.joff + 9, d.ioff:d.ioff + 12].numpy())


def test_dump_sample_is_fixed_and_within_budget(tmp_path):
    d = abi.dims_init(40, 30, 6)
    f = _fields(d)
    budget = 8 * 4 * 500
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), d, f, budget=budget)
    bench.dump_outputs(str(b), d, {k: v.clone() for k, v in f.items()}, budget=budget)
    data = sum(np.load(a / (n + ".npy")).nbytes for n in f)
    assert data <= budget
    for n in f:
        x = np.load(a / (n + ".npy"))
        assert x.dtype == np.float64 and x.shape == (500,)
        np.testing.assert_array_equal(x, np.load(b / (n + ".npy")))
    # the sample is the seeded positions of the h-point domain, flattened k, j, i
    dom = f["h"][:, d.joff:d.joff + 30, d.ioff:d.ioff + 40].reshape(-1).numpy()
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(dom.size, 500, replace=False))
    np.testing.assert_array_equal(np.load(a / "h.npy"), dom[idx])
