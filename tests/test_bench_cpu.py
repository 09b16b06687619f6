"""bench.py's host-side pieces that need no GPU: the --dump-outputs writer and the --steps check."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hotpath(big):
    g = torch.Generator().manual_seed(0)
    ngp = torch.nn.Linear(4, 3)
    return types.SimpleNamespace(ngp=ngp, last_outputs={"loss": torch.tensor(0.25), "img": torch.rand(1, 3, 4, 4, generator=g),
                                                        "big": torch.rand(big, generator=g, dtype=torch.float64)})


def test_dump_outputs_writes_float32_npy_and_samples_large_arrays(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    hp = _hotpath(1000)
    index = bench.dump_outputs(hp, str(tmp_path / "a"))
    assert set(index) == {"loss", "img", "big", "ngp.weight", "ngp.bias"}
    for name, entry in index.items():
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == np.float32
        if name == "big":
            assert entry == {"shape": [1000], "sampled": True} and a.shape == (100,)
            assert np.all(np.isin(a, hp.last_outputs["big"].float().numpy()))
        else:
            assert not entry["sampled"] and list(a.shape) == entry["shape"]
    assert np.array_equal(np.load(tmp_path / "a" / "img.npy"), hp.last_outputs["img"].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "ngp.weight.npy"), hp.ngp.weight.detach().numpy())
    # the sample of a large array is the same index set on every run
    bench.dump_outputs(hp, str(tmp_path / "b"))
    assert np.array_equal(np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy"))


def test_dump_outputs_refuses_more_than_the_byte_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1024)
    with pytest.raises(SystemExit, match="exceed"):
        bench.dump_outputs(_hotpath(1000), str(tmp_path))


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 2 and "--steps must be at least 1" in out.stderr


@pytest.mark.parametrize("value,want", [("16", 16), (" 8 ", 8), ("16,4", 16), ("", None), ("abc", None), ("0", None)])
def test_cpu_threads_parses_omp_num_threads(monkeypatch, value, want):
    monkeypatch.setenv("OMP_NUM_THREADS", value)
    assert bench.cpu_threads() == (want if want is not None else len(os.sched_getaffinity(0)))
