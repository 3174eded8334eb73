"""The stream loop's sub-step schedule and the late issue of the half-space tail's inputs
(moments.hip: the fences between a load group's sub-steps in mfma_group, CCMPC_SUBSTEP_FENCE, and
prefetch_tail issued behind the item's first load group, CCMPC_TAIL_LATE).  Neither changes a
value, so every check here holds on the library without them too.

  sub-step boundaries   A sub-step is 16 particles, a lane's quad 4, a wave's group 64, an item
                        256.  One OV whose cells end one under, on and one over every quad and
                        sub-step boundary of a group (1, 3, 4, 5, 15 .. 65): alone, above 256 (a
                        whole-cell item whose round-robin groups end inside each sub-step) and
                        above the whole-cell cap of 1024 (a late wave of a multi-item cell), at
                        T = 8 on both stores (the TC = 8 instances) and T = 7 (the generic one).
  the tail's inputs     Two scenes in one store, scene 1's cells reading reference row 1 and every
                        cell risk constants of its own, at T = 8 and T = 7: a prefetch that lands
                        in another cell's slot, or is stored to LDS before it has landed, changes
                        records, and the two-call path (whose rows kernel reads both tables in
                        another launch) then differs in bits.
  two groups per wave   Cells large enough that a wave's ring loop runs: 1024 particles as one
                        whole-cell item (four round-robin groups per wave, the tiny-input path) and
                        one ragged sub-step under and over it; the same counts at T = 12 (Scheme4's
                        ring) and at T = 16 (two row blocks, RB = 2: two sub-steps per group).

Checks are test_gpu_block_const.py's, with its tolerances: moments against NumPy (ddof = 1) at
rtol 1e-10 / atol 1e-12, means at rtol 1e-13; the fused launch, a second launch, the two-call path
and a graph replay bit for bit; status, (t, tau) order, `which` and `side` against the oracle's
generator.  The oracle's decisions are compared on the cells with more than 2 T particles: with
n - 1 < 2 T samples the 2T x 2T covariance is singular by construction (rank n - 1; a 1-particle
cell's is 0 / 0), and which side of a degenerate ellipse a half-space takes is decided by
rounding in the oracle as in the kernel.  Those cells keep the moments check (NaN for NaN at
n = 1) and the bit-for-bit agreement of the four launch forms.
"""
import warnings

import numpy as np
import pytest
import torch

from oracle import ccmpc_oracle as orc
from test_gpu_block_const import (_clouds, _decisions_match, _launch_forms_agree,
                                  _moments_match_numpy, _oracle_ov, _run_all)

pytestmark = pytest.mark.gpu

# one under, on and one over every quad (4) / sub-step (16) / group (64) boundary of a group
EDGES = [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]
SUBSTEP_COUNTS = EDGES + [256 + e for e in EDGES] + [1024 + e for e in EDGES]

STORES = [(8, torch.float64), (8, torch.float32), (7, torch.float64)]
STORE_IDS = ["T8-f64", "T8-f32", "T7-f64"]


def _bits(ts):
    return [t.contiguous().view(torch.uint8) for t in ts]


def _same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _forms_agree_bits(gpu, cyc):
    """test_gpu_block_const._launch_forms_agree on the outputs' bytes, so that the NaN covariance
    of a 1-particle cell compares equal to itself: the fused launch, a second one, the two-call
    path and a graph replay."""
    first = _run_all(cyc)
    assert _same_bits(first, _run_all(cyc))
    cyc.rec.zero_()
    cyc.run_unfused()
    assert _same_bits(first, (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower))
    cyc.rec.zero_()
    cyc.capture()
    cyc.replay()
    torch.cuda.synchronize(gpu)
    assert _same_bits(first, (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower))
    return first


def _check_ov(gpu, T, counts, dtype, seed):
    """test_gpu_block_const._check_one_ov, with the oracle's decisions on the cells whose
    covariance has full rank (module docstring)."""
    from ccmpc import cycle, engine
    cells, past, ref = _clouds(T, counts, seed)
    C = len(cells)
    origin = np.array([c[:, 0].mean(0) for c in cells]) if dtype == torch.float32 else None
    store = engine.ParticleStore.from_cells(cells, device=gpu, dtype=dtype, origin=origin)
    cyc = cycle.MinkowskiCycle(store, [C], ref)
    first = _forms_agree_bits(gpu, cyc)
    seen = [store.cell_positions(j) if dtype == torch.float32 else cells[j] for j in range(C)]
    with warnings.catch_warnings():          # np.cov of one sample: 0 / 0, as the kernel's
        warnings.simplefilter("ignore", RuntimeWarning)
        _moments_match_numpy(first, seen, T)
    full = [j for j in range(C) if counts[j] > 2 * T]
    assert len(full) >= C - 6
    want = orc.minkowski_generator([_oracle_ov([seen[j] for j in full], past, T)], T, T, ref,
                                   with_l4=False)["records"]
    P = T * (T - 1) // 2
    assert len(want) == len(full) * P
    _decisions_match(cyc.records().reshape(C, P)[full], want)
    return store


@pytest.mark.parametrize("T,dtype", STORES, ids=STORE_IDS)
def test_cells_ending_inside_every_substep(gpu, T, dtype):
    store = _check_ov(gpu, T, SUBSTEP_COUNTS, dtype, seed=9600 + T)
    assert store.n_bound <= 2 ** 15          # the plain launch, whole-cell items up to 1024


@pytest.mark.parametrize("T", [8, 7])
def test_tail_inputs_per_cell_reference_and_risk(gpu, T):
    """Scene 1's cells read reference row 1 and every cell has risk constants of its own; the
    records match the oracle's decisions per scene and equal run_unfused()'s bit for bit, integer
    fields included."""
    from ccmpc import cycle, engine, synthetic
    scenes = [synthetic.scene(s, O=2, N=600, T=T) for s in (9700 + T, 9800 + T)]
    cells = [c for ovs, _, _ in scenes for o in ovs for c in o]
    scene_K = [[len(o) for o in ovs] for ovs, _, _ in scenes]
    refs = np.array([ref for _, ref, _ in scenes])
    assert not np.array_equal(refs[0], refs[1])
    store = engine.ParticleStore.from_cells(cells, device=gpu)
    K = [k for Ks in scene_K for k in Ks]
    cyc = cycle.MinkowskiCycle(store, K, refs, scene_K=scene_K)
    ref_of = cyc.cell_ref.cpu().numpy()
    assert ref_of.min() == 0 and ref_of.max() == 1
    scale = 1.0 + 0.02 * torch.arange(1, store.n_cells + 1, dtype=torch.float64, device=gpu)
    shared = _run_all(cyc)
    cyc.risk = cyc.risk * scale[:, None]
    assert len({tuple(r) for r in cyc.risk.cpu().tolist()}) == store.n_cells
    first = _launch_forms_agree(gpu, cyc)    # the fused launch == run_unfused() == a replay
    _moments_match_numpy(first, cells, T)
    h = cyc.records()
    c0 = 0
    for (ovs, ref, pasts), Ks in zip(scenes, scene_K):
        want = orc.minkowski_generator([_oracle_ov(o, p, T) for o, p in zip(ovs, pasts)], T, T,
                                       ref, with_l4=False)["records"]
        _decisions_match(h[c0:c0 + sum(Ks)], want)
        c0 += sum(Ks)
    # the records are a view of the launch's bytes: every field, the integer ones included
    cyc.rec.zero_()
    cyc.run_unfused()
    assert np.array_equal(cyc.records().view(np.uint8), h.view(np.uint8))
    # every cell's own constants were the ones read: its records moved against the shared ones
    hs = engine.halfspaces(shared[2]).reshape(h.shape)
    for j in range(store.n_cells):
        assert not np.array_equal(h[j]["q00"], hs[j]["q00"]), j
    # and every cell reading row 0 changes scene 1's records and leaves scene 0's bits
    wrong = cycle.MinkowskiCycle(store, K, refs, cell_ref=np.zeros(store.n_cells, np.int64),
                                 scene_K=scene_K)
    wrong.risk = cyc.risk
    wrong.run()
    hw, n0 = wrong.records(), sum(scene_K[0])
    assert np.array_equal(hw[:n0].view(np.uint8), h[:n0].view(np.uint8))
    assert not np.array_equal(hw[n0:]["d"], h[n0:]["d"])


# the whole-cell cap and a ragged group under and over it (1040: one sub-step into a fifth item)
RING_COUNTS = [1024, 1009, 1040]


@pytest.mark.parametrize("T,dtype", [(8, torch.float64), (8, torch.float32), (12, torch.float64),
                                     (16, torch.float64)],
                         ids=["T8-f64", "T8-f32", "T12-f64", "T16-f64"])
def test_two_groups_per_wave(gpu, T, dtype):
    """1024 particles at T <= 8 are one whole-cell item on the tiny-input path: 16 groups dealt
    round-robin, four per wave, so the ring loop runs twice; at T = 12 (Scheme4) and T = 16
    (RB = 2) an item is 256 particles of 32-particle (f64) groups, two per wave."""
    store = _check_ov(gpu, T, RING_COUNTS, dtype, seed=9900 + T)
    assert store.n_bound <= 2 ** 15
