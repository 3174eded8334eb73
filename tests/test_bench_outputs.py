"""bench.py's plain run, `--full` and `--dump-outputs`: the options parse as documented, the dump
writes float64 .npy files under its size cap (a fixed seeded row sample above it), and a plain
run on the GPU prints one short headline line and dumps what its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps",
                 "warmup", "n_gpus")
FULL_ONLY_KEYS = ("roofline", "pcie_inclusive", "ellipsoid_parity", "cpu_baseline", "c4_sharded",
                  "roofline_sweep", "dropin_step_c2", "planning_qp", "v8_milp")


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_writes_float64_under_the_cap(tmp_path, monkeypatch):
    rng = np.random.default_rng(3)
    arrs = {"a": rng.normal(size=(5, 4)).astype(np.float32), "b": rng.normal(size=(40, 8, 2))}
    bench.dump_outputs(str(tmp_path / "whole"), arrs)
    got = {n: np.load(tmp_path / "whole" / f"{n}.npy") for n in arrs}
    for n, a in arrs.items():
        assert got[n].dtype == np.float64 and np.array_equal(got[n], a.astype(np.float64))
    # over the cap: each array keeps its share as whole rows, the same rows on every run
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 2 * 10 * 8 * 2 * 8)
    bench.dump_outputs(str(tmp_path / "cut1"), arrs)
    bench.dump_outputs(str(tmp_path / "cut2"), arrs)
    b1, b2 = np.load(tmp_path / "cut1" / "b.npy"), np.load(tmp_path / "cut2" / "b.npy")
    assert b1.shape == (10, 8, 2) and np.array_equal(b1, b2)
    rows = [int(np.flatnonzero((arrs["b"] == r).all(axis=(1, 2)))[0]) for r in b1]
    assert rows == sorted(set(rows))
    assert np.array_equal(np.load(tmp_path / "cut1" / "a.npy"), arrs["a"].astype(np.float64))
    total = sum(os.path.getsize(tmp_path / "cut1" / f) for f in os.listdir(tmp_path / "cut1"))
    assert total <= bench.DUMP_CAP_BYTES + 2 * 128      # + the .npy headers


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_last_step(gpu, tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR` in a fresh process: one JSON
    line under 4 KB with the headline keys and none of --full's, 3 timed steps, and the dumped
    arrays equal to the same cycle run here on the same seeded scene: the integer record fields
    exactly, the means to 1e-11 relative (a float64 sum of 5 000 same-signed coordinates in any
    order: <= n eps = 5.6e-13)."""
    import torch
    from ccmpc import cycle, engine, synthetic
    d = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0].encode()) < 4096, out.stdout[:300]
    rep = json.loads(lines[0])
    assert all(k in rep for k in HEADLINE_KEYS) and not any(k in rep for k in FULL_ONLY_KEYS)
    assert rep["steps"] == 3 and rep["warmup"] == 1 and rep["ms_per_step"] > 0
    assert rep["value"] == pytest.approx(1e3 / rep["ms_per_step"], rel=1e-3)

    a = bench.parse([])
    ovs, ref, _ = synthetic.scene(a.seed, O=a.O, N=a.N, T=a.T)
    store = engine.ParticleStore.from_cells([c for o in ovs for c in o], device=gpu)
    cyc = cycle.MinkowskiCycle(store, [len(o) for o in ovs], ref)
    cyc.run()
    torch.cuda.synchronize(gpu)
    want = bench.cycle_outputs(cyc)
    got = {n: np.load(d / f"{n}.npy") for n in want}
    names = list(engine._lib.HALFSPACE_DTYPE.names)
    ints = [names.index(n) for n in ("which", "side", "status", "t_tau")]
    for n in want:
        assert got[n].dtype == np.float64 and got[n].shape == want[n].shape, n
    assert got["records"].shape == (cyc.n_constraints, len(names))
    assert np.array_equal(got["records"][:, ints], want["records"][:, ints])
    np.testing.assert_allclose(got["mean"], want["mean"], rtol=1e-11, atol=0)
