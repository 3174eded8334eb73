"""Every kernel whose helpers take the workgroup's thread count as a compile-time constant
(gram.hpp NTH: combine_waves / combine4, tree_climb, gather_root, finalize_cell, minkowski_cell),
and the half-space tail's prefetch of a cell's reference row and risk constants (moments.hip
prefetch_tail), at the smallest shapes where a wrong count or a wrong prefetch address shows:

  fused cycle      T = 8 and T = 2 (16-row tile, 256 threads), T = 12 (4-row blocks), T = 16
                   (two row blocks), f64 and f32 store; one store holds cells of one item (the
                   nit == 1 path: combined in LDS), 2, 17 and 33 items of 256 with ragged last
                   items (one group in each thread | two groups in the halves of a wave or
                   through LDS | three groups through LDS).  A stride that is not the
                   workgroup's size leaves slab entries unsummed or covariance entries unwritten.
  T = 40           five row blocks, 512 threads, balanced mode at small counts: cells of
                   2 .. 64 items take the deferred root (root_finalize_kernel), a larger one
                   the combine tree; the half-spaces are the rows launch.
  ideal rollout    engine.ideal_minkowski_cycle at T = 7 with a few thousand samples.
  two scenes       cells reading different reference trajectories, every cell its own risk
                   constants, at T = 2 and T = 24 (prefetch lanes 0 .. 6 and 0 .. 50): a
                   mis-selected prefetch address changes records.

Checks, with the tolerances of the tests they come from: moments against NumPy (ddof = 1) at
test_gpu_c3_sweep.py's rtol 1e-10 / atol 1e-12 (means: test_gpu_root_gather.py's rtol 1e-13);
record status, (t, tau) order, `which` and `side` against the oracle's generator; the fused
launch against the two-call path, a second launch and a graph replay, bit for bit.
"""
import numpy as np
import pytest
import torch

from oracle import ccmpc_oracle as orc

pytestmark = pytest.mark.gpu

ITEM = 256


def _counts(items):
    # a ragged last item: 1 .. 255 particles, different for every cell
    return [(k - 1) * ITEM + 1 + (37 * (i + 1)) % (ITEM - 1) for i, k in enumerate(items)]


_CLOUDS = {}


def _clouds(T, counts, seed):
    """(cells, past, ref) for one OV whose modes are the cells; built once per shape."""
    key = (T, tuple(counts), seed)
    if key not in _CLOUDS:
        from ccmpc import synthetic
        rng = np.random.default_rng(np.random.Philox(seed))
        p0 = np.array([190.0, -80.0])
        cells = [synthetic.mode_cloud(rng, n, T, p0) for n in counts]
        for c in cells:
            c.setflags(write=False)
        _CLOUDS[key] = (cells, p0 - np.array([2.0, 0.5]), synthetic.ego_ref(seed, T))
    return _CLOUDS[key]


def _run_all(cyc):
    cyc.rec.zero_()
    cyc.run()
    return cyc.mean.clone(), cyc.cov.clone(), cyc.rec.clone(), cyc.prob_lower.clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _launch_forms_agree(gpu, cyc):
    """The fused launch, a second one, the two-call path and a graph replay: the same bits."""
    first = _run_all(cyc)
    assert _same(first, _run_all(cyc))
    cyc.rec.zero_()
    cyc.run_unfused()
    assert _same(first, (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower))
    cyc.rec.zero_()
    cyc.capture()
    cyc.replay()
    torch.cuda.synchronize(gpu)
    assert _same(first, (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower))
    return first


def _moments_match_numpy(first, seen, T, mean_rtol=1e-13):
    mean, cov = first[0].cpu().numpy(), first[1].cpu().numpy()
    for j, traj in enumerate(seen):
        X = traj.reshape(len(traj), 2 * T)
        np.testing.assert_allclose(cov[j], np.cov(X, rowvar=False), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(mean[j].reshape(-1), X.mean(0), rtol=mean_rtol)


def _oracle_ov(seen, past, T):
    p = np.asarray(past, float).reshape(1, 2)
    C = len(seen)
    return orc.OVehicle(T, p, np.ones(C) / C, seen, [orc._step_yaws(c, p[-1], T) for c in seen],
                        np.zeros((C, 2)), np.array([4.5, 2.5]))


def _decisions_match(h, want):
    h = h.reshape(-1)
    assert len(h) == len(want)
    assert np.all(h["status"] == 0)
    np.testing.assert_array_equal(np.stack((h["t_tau"] >> 16, h["t_tau"] & 0xFFFF), 1),
                                  [(r["t"], r["tau"]) for r in want])
    np.testing.assert_array_equal(h["which"], [r["which"] for r in want])
    np.testing.assert_array_equal(h["side"], [r["side"] for r in want])


def _check_one_ov(gpu, T, counts, dtype, capacity=None, seed=None):
    from ccmpc import cycle, engine
    cells, past, ref = _clouds(T, counts, 9100 + T if seed is None else seed)
    C = len(cells)
    origin = np.array([c[:, 0].mean(0) for c in cells]) if dtype == torch.float32 else None
    store = engine.ParticleStore.from_cells(cells, device=gpu, dtype=dtype, origin=origin,
                                            capacity=capacity)
    cyc = cycle.MinkowskiCycle(store, [C], ref)
    first = _launch_forms_agree(gpu, cyc)
    seen = [store.cell_positions(j) if dtype == torch.float32 else cells[j] for j in range(C)]
    _moments_match_numpy(first, seen, T)
    want = orc.minkowski_generator([_oracle_ov(seen, past, T)], T, T, ref,
                                   with_l4=False)["records"]
    assert len(want) == C * T * (T - 1) // 2
    _decisions_match(cyc.records(), want)
    return store


# a one-item cell everywhere (200 particles), a cell of at most 1024 particles (one item up to
# T = 8, where such a cell is combined whole in LDS; four items above), then 2, 17 and 33 items
FUSED_COUNTS = [200, 1000] + _counts((2, 17, 33))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("T", [8, 12, 16, 2])
def test_fused_cycle_thread_counts(gpu, T, dtype):
    store = _check_one_ov(gpu, T, FUSED_COUNTS, dtype)
    assert store.n_bound <= 2 ** 15          # the plain launch with whole-cell items at T <= 8


def test_t40_deferred_root_tree_and_rows_launch(gpu):
    """T = 40 in balanced mode (the capacity alone selects it; the chunk follows the counts):
    the 2600-particle cell is cut into more than 64 items and climbs the tree, the others are
    summed by root_finalize_kernel, the 12-particle one is a single item (the chunk is 16 or 32
    particles, by the device's resident grid)."""
    counts = [37, 900, 12, 2600, 260]
    store = _check_one_ov(gpu, 40, counts, torch.float64, capacity=2 ** 18 + 64)
    assert store.n_bound > 2 ** 18


def test_fused_ideal_rollout_t7(gpu):
    """ideal_gram_kernel (its own thread-count constant): the fused cycle against ideal_moments +
    minkowski and a second launch bit for bit, against NumPy and the oracle's generator on the
    materialised rollout of the same seed."""
    from ccmpc import engine as e, risk
    T_src, Tn, ns = 8, 7, 3000
    rng = np.random.default_rng(4)
    cells = [190 + np.cumsum(rng.normal(0, 0.4, size=(n, T_src, 2)), axis=1) for n in (900, 1500)]
    mean, cov = e.moments(e.ParticleStore.from_cells(cells, device=gpu))
    src = torch.tensor([0, 1], dtype=torch.int32, device=gpu)
    cr = torch.as_tensor(risk.cell_risk(risk.eps_ura([2]), [2], Tn), device=gpu)
    ref_np = np.array([170.0, 5.0]) + np.arange(1, Tn + 1)[:, None] * [4.0, 0.5]
    ref = torch.as_tensor(ref_np[None], device=gpu)
    m1, c1, st1 = e.ideal_moments(mean, cov, src, Tn, ns, seed=5)
    r1, pl1 = e.minkowski(m1, c1, ref, cr)
    got = e.ideal_minkowski_cycle(mean, cov, src, Tn, ns, ref, cr, seed=5)
    again = e.ideal_minkowski_cycle(mean, cov, src, Tn, ns, ref, cr, seed=5)
    assert _same(got, again)
    assert _same(got, (m1, c1, st1, r1, pl1))
    assert got[2].cpu().tolist() == [0, 0]
    rolled, st = e.ideal_rollout(mean, cov, src, Tn, ns, seed=5)
    assert st.cpu().tolist() == [0, 0]
    seen = [rolled.cell_positions(j) for j in range(2)]
    # (the mean at test_gpu_core.py's tolerance for the fused rollout against the materialised one)
    _moments_match_numpy(got, seen, Tn, mean_rtol=1e-12)
    want = orc.minkowski_generator([_oracle_ov(seen, np.array([168.0, 4.5]), Tn)], Tn, Tn, ref_np,
                                   with_l4=False)["records"]
    _decisions_match(e.halfspaces(got[3]), want)


@pytest.mark.parametrize("T", [2, 24])
def test_two_scenes_own_reference_and_risk_per_cell(gpu, T):
    """Two scenes in one store: scene 1's cells read reference row 1, and (second half) every
    cell gets risk constants of its own.  The prefetch is lanes 0 .. 2T - 1 (the cell's reference
    row) and 2T .. 2T + 2 (its risk row): the two-call path reads both tables from global
    memory in another kernel, so a wrong address in either shows as different bits."""
    from ccmpc import cycle, engine, synthetic
    seeds = (9300 + T, 9400 + T)
    scenes = [synthetic.scene(s, O=2, N=600, T=T) for s in seeds]
    cells = [c for ovs, _, _ in scenes for o in ovs for c in o]
    scene_K = [[len(o) for o in ovs] for ovs, _, _ in scenes]
    refs = np.array([ref for _, ref, _ in scenes])
    assert not np.array_equal(refs[0], refs[1])
    store = engine.ParticleStore.from_cells(cells, device=gpu)
    K = [k for Ks in scene_K for k in Ks]
    cyc = cycle.MinkowskiCycle(store, K, refs, scene_K=scene_K)
    ref_of = cyc.cell_ref.cpu().numpy()
    assert ref_of.min() == 0 and ref_of.max() == 1
    first = _launch_forms_agree(gpu, cyc)
    _moments_match_numpy(first, cells, T)
    h = cyc.records()
    c0 = 0
    for (ovs, ref, pasts), Ks in zip(scenes, scene_K):
        want = orc.minkowski_generator([_oracle_ov(o, p, T) for o, p in zip(ovs, pasts)], T, T,
                                       ref, with_l4=False)["records"]
        _decisions_match(h[c0:c0 + sum(Ks)], want)
        c0 += sum(Ks)
    # every cell reading row 0 changes scene 1's records and leaves scene 0's bits
    wrong = cycle.MinkowskiCycle(store, K, refs, cell_ref=np.zeros(store.n_cells, np.int64),
                                 scene_K=scene_K)
    wrong.run()
    hw, n0 = wrong.records(), sum(scene_K[0])
    assert np.array_equal(hw[:n0].view(np.uint8), h[:n0].view(np.uint8))
    assert not np.array_equal(hw[n0:]["d"], h[n0:]["d"])
    # risk constants of its own for every cell: chi_r, chi_p, gamma all different across cells
    base = cyc.risk.clone()
    scale = 1.0 + 0.02 * torch.arange(1, store.n_cells + 1, dtype=torch.float64, device=gpu)
    cyc.risk = base * scale[:, None]
    assert len({tuple(r) for r in cyc.risk.cpu().tolist()}) == store.n_cells
    cyc.graph = None
    own = _launch_forms_agree(gpu, cyc)
    ho = cyc.records()
    assert np.all(ho["status"] == 0)
    for j in range(store.n_cells):       # every cell's records moved with its own constants
        assert not np.array_equal(ho[j]["q00"], h[j]["q00"]), j
    assert not np.array_equal(ho["lower_bound"], h["lower_bound"])
    assert torch.equal(own[0], first[0]) and torch.equal(own[1], first[1])
