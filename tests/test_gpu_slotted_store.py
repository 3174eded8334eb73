"""The cycle kernel on a slotted particle store (every cell_off[c] == c * slot_cap; moments.hip's
SLOT instances, reached through ccmpc_minkowski_cycle_args) against the packed store of the same
cells: mean, cov, prob_lower and every record byte are the same bits.

The slotted front requests each wave's first load group before it knows the cell's count -- the
loads are not clamped to the cell's last run, and a workgroup whose chunk holds no item leaves
before it touches a counter or a slab -- so the cases walk the item arithmetic (empty, one group,
one item, the whole-cell cap of 1024, 16 / 17 / 33 slabs, a cell that fills its slot to the store's
last column), poison everything a slot holds past its cell, launch twice on one workspace, and
check that the host turns a bad slot_cap or ld away with an error code and no launch.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# every branch of the item arithmetic at a 256-particle chunk; slots of 1280 (5 items each)
EDGE_COUNTS = (0, 1, 3, 63, 64, 65, 255, 256, 257, 1024, 1025)
# 16 / 17 slabs, the 33-slab gather, and last a cell that IS its slot (8448 = 33 chunks): its
# last run ends with the slot and the slot with the store
TREE_COUNTS = (16 * 256, 16 * 256 + 1, 32 * 256 + 1, 33 * 256)
# no cell too small for a 16 x 16 covariance: every record's status is 0
POISON_COUNTS = (63, 64, 65, 255, 257, 1025, 1300, 2049)
C2_LIKE_COUNTS = (5000, 1391, 3609, 2220, 1474, 1306, 5000, 600, 3400)

CCMPC_ERR_ARG = -1      # include/ccmpc.h

STORES = [(8, False), (8, True), (7, False), (7, True)]
STORE_IDS = ["T8-f64", "T8-f32", "T7-f64", "T7-f32"]


@functools.lru_cache(maxsize=None)
def _inputs(T, counts, seed):
    rng = np.random.default_rng(seed)
    cells = [190 + 6 * (j % 7) + np.cumsum(rng.normal(0, 0.5, size=(n, T, 2)), axis=1)
             for j, n in enumerate(counts)]
    origin = np.array([[120.5 + 3 * (j % 5), -40.25 - 2 * (j % 3)] for j in range(len(counts))])
    ref = np.array([[[170.0 + 4.0 * (t + 1), 10.0 + 0.5 * (t + 1)] for t in range(T)],
                    [[150.0 + 3.0 * (t + 1), 35.0 - 0.25 * (t + 1)] for t in range(T)]])
    for a in cells + [origin, ref]:
        a.setflags(write=False)
    return cells, origin, ref


def _store(gpu, T, counts, seed, f32, slots):
    from ccmpc import engine
    cells, origin, _ = _inputs(T, counts, seed)
    return engine.ParticleStore.from_cells(
        list(cells), device=gpu, dtype=torch.float32 if f32 else torch.float64,
        origin=origin.copy() if f32 else None, slots=slots)


def _cycle(store, T, counts, seed, with_ref):
    from ccmpc import cycle
    _, _, ref = _inputs(T, counts, seed)
    if with_ref:
        return cycle.MinkowskiCycle(store, [len(counts)], ref.copy(),
                                    cell_ref=[(j + 1) % 2 for j in range(len(counts))])
    return cycle.MinkowskiCycle(store, [len(counts)], ref[0].copy())


def _bytes(cyc):
    torch.cuda.synchronize()
    return tuple(x.contiguous().view(torch.uint8).cpu().numpy().copy()
                 for x in (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower))


def _launch(cyc):
    """The struct path on a slotted store, the positional path on a packed one."""
    for x in (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower):
        x.view(torch.uint8).fill_(0x5A)
    cyc.bind().launch() if cyc.store.slot_cap else cyc.run()
    return _bytes(cyc)


def _assert_same(got, want):
    for name, a, b in zip(("mean", "cov", "rec", "prob_lower"), got, want):
        np.testing.assert_array_equal(a, b, err_msg=name)


def _check_layout(store, counts):
    cap = store.slot_cap
    assert cap > 0 and cap % 256 == 0 and cap >= max(counts)
    assert store.offsets == [j * cap for j in range(len(counts))]
    assert store.cell_off.cpu().tolist() == store.offsets
    assert store.ld >= len(counts) * cap


def _pair(gpu, T, counts, seed, f32, with_ref):
    packed = _store(gpu, T, counts, seed, f32, slots=False)
    slotted = _store(gpu, T, counts, seed, f32, slots=True)
    _check_layout(slotted, counts)
    assert packed.slot_cap == 0 and packed.n_bound == slotted.n_bound <= 2 ** 15
    want = _launch(_cycle(packed, T, counts, seed, with_ref))
    cyc = _cycle(slotted, T, counts, seed, with_ref)
    return want, cyc


@pytest.mark.parametrize("with_ref", [False, True], ids=["ref0", "cell_ref"])
@pytest.mark.parametrize("T,f32", STORES, ids=STORE_IDS)
@pytest.mark.parametrize("counts", [EDGE_COUNTS, TREE_COUNTS], ids=["edges", "tree"])
def test_slotted_equals_packed_bitwise(gpu, counts, T, f32, with_ref):
    want, cyc = _pair(gpu, T, counts, 4100 + T, f32, with_ref)
    if counts is TREE_COUNTS:       # the last cell fills its slot, and the slot ends the store
        assert cyc.store.counts[-1] == cyc.store.slot_cap
        assert cyc.store.ld == len(counts) * cyc.store.slot_cap
    _assert_same(_launch(cyc), want)


@pytest.mark.parametrize("counts", [(700,), C2_LIKE_COUNTS, (300,) * 64],
                         ids=["1cell", "9cells", "64x300"])
def test_launch_sizes(gpu, counts):
    want, cyc = _pair(gpu, 8, counts, 4200, False, True)
    _assert_same(_launch(cyc), want)


@pytest.mark.parametrize("poison", [float("nan"), 1e300], ids=["nan", "1e300"])
@pytest.mark.parametrize("T,f32", STORES, ids=STORE_IDS)
def test_poison_past_every_cell(gpu, T, f32, poison):
    """Every column of a slot at or past its cell's count holds the poison: the unclamped first
    load group reads it, and none of it reaches a result."""
    counts = POISON_COUNTS
    want, cyc = _pair(gpu, T, counts, 4300 + T, f32, True)
    st = cyc.store
    if f32 and np.isfinite(poison):         # 1e300 is no float32: the largest one stands in
        poison = float(np.finfo(np.float32).max)
    for j, n in enumerate(counts):
        st.pos[:, j * st.slot_cap + n:(j + 1) * st.slot_cap] = poison
    st.pos[:, len(counts) * st.slot_cap:] = poison
    got = _launch(cyc)
    _assert_same(got, want)
    assert np.all(cyc.records()["status"] == 0)


def test_two_launches_on_one_workspace(gpu):
    """The second launch finds every arrival counter at zero: the last arrivers reset them and
    the workgroups without an item took no ticket."""
    want, cyc = _pair(gpu, 8, EDGE_COUNTS + TREE_COUNTS[:2], 4400, False, True)
    _assert_same(_launch(cyc), want)
    _assert_same(_launch(cyc), want)
    cyc.run()                                   # run() takes the struct path on a slotted store
    _assert_same(_bytes(cyc), want)


@pytest.mark.parametrize("what", ["slot_cap", "ld"])
def test_host_rejects_a_bad_slot(gpu, what):
    from ccmpc import _lib
    counts = (1300, 300, 40)
    _, cyc = _pair(gpu, 8, counts, 4500, False, True)
    cyc.bind()
    if what == "slot_cap":
        cyc._argst.slot_cap = cyc.store.slot_cap + 32      # no multiple of the 256-particle chunk
    else:
        cyc._argst.ld = len(counts) * cyc.store.slot_cap - 32
    for x in (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower):
        x.view(torch.uint8).fill_(0x5A)
    rc = cyc._fn(*cyc._args)
    assert rc == CCMPC_ERR_ARG
    for x in _bytes(cyc):                                  # nothing was launched
        assert np.all(x == 0x5A)
    with pytest.raises(_lib.CcmpcError):
        cyc.launch()


@pytest.mark.parametrize("T,f32", STORES, ids=STORE_IDS)
def test_positional_entry_runs_the_packed_path(gpu, T, f32):
    """engine.minkowski_cycle has no slot_cap: it reads the slotted store's honest tables."""
    from ccmpc import engine
    counts = EDGE_COUNTS
    want, cyc = _pair(gpu, T, counts, 4600 + T, f32, True)
    _assert_same(_launch(cyc), want)
    for x in (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower):
        x.view(torch.uint8).fill_(0x5A)
    engine.minkowski_cycle(cyc.store, cyc.ref, cyc.risk, cell_ref=cyc.cell_ref, R=cyc.R,
                           tol=cyc.tol, maxiter=cyc.maxiter, workspace=cyc.ws, out_mean=cyc.mean,
                           out_cov=cyc.cov, out_rec=cyc.rec, out_prob_lower=cyc.prob_lower)
    _assert_same(_bytes(cyc), want)
