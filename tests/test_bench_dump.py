"""bench.py --dump-outputs: what the last timed step computed, written as <name>.npy (float32 / float64, at most 64 MB, larger
arrays as a fixed seeded sample), so that two builds can be compared output for output; and --steps K times K steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float_arrays_and_samples_large_ones_reproducibly(tmp_path):
    import bench
    lin = torch.nn.Linear(4, 3).double()
    big = torch.nn.Parameter(torch.zeros(bench.DUMP_MAX_ELEMS + 5))
    big.grad = torch.arange(big.numel(), dtype=torch.float32)
    mod = torch.nn.Module()
    mod.lin, mod.big = lin, big
    lin(torch.ones(2, 4, dtype=torch.float64)).sum().backward()
    outputs = {"rgb": torch.rand(1, 8, 3, dtype=torch.float16), "loss.all": torch.tensor(2.5)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outputs, [("m", mod)])
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == ["grad.m.big", "grad.m.lin.bias", "grad.m.lin.weight", "loss.all", "rgb"]
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in names}
    assert a["rgb"].dtype == np.float32 and a["rgb"].shape == (1, 8, 3)
    assert a["grad.m.lin.weight"].dtype == np.float64
    np.testing.assert_array_equal(a["rgb"], outputs["rgb"].float().numpy())
    np.testing.assert_array_equal(a["grad.m.lin.weight"], lin.weight.grad.numpy())
    s = a["grad.m.big"]                       # the gradient is its own index: the sample shows which entries were taken
    assert s.shape == (bench.DUMP_MAX_ELEMS,) and np.all(np.diff(s) > 0) and s[-1] < big.numel()
    for n in names:
        np.testing.assert_array_equal(a[n], b[n])


@pytest.mark.gpu
def test_bench_dump_outputs_eager_equals_graph(tmp_path):
    """the same arguments -> the same inputs: the eager run and the hipGraph replay dump the same outputs and gradients"""
    runs = {}
    for launch in ("eager", "graph"):
        d = tmp_path / launch
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "2", "--rays", "256",
                              "--samples", "32", "--no-cpu-baseline", "--launch", launch, "--dump-outputs", str(d)],
                             cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        assert not {"roofline", "eager_profiled_ms_per_step", "mirror_upkeep", "cpu_baseline"} & set(line)    # --full only
        arrays = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert {"rgb", "normals", "depth_mlp", "loss.all"} <= set(arrays)
        assert any(k.startswith("grad.sdf.") for k in arrays) and any(k.startswith("grad.rad.") for k in arrays)
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert all(np.isfinite(a).all() for a in arrays.values())
        runs[launch] = arrays
    assert set(runs["eager"]) == set(runs["graph"])
    for k, ref in runs["eager"].items():
        got = runs["graph"][k].astype(np.float64)
        ref = ref.astype(np.float64)
        assert got.shape == ref.shape, k
        assert np.abs(got - ref).max() <= 1e-5 * (np.abs(ref).max() + 1e-30), k
