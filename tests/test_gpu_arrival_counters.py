"""The combine tree's arrival counters (gram.hpp: tree_layout, tree_climb, arrive_last) with the
counters spread one per kCounterStride words, at every root width and tree depth.

A cell of k work items meets in a root of k slabs through one arrival counter (k <= 64) or, at
65 items, through five level-0 counters and a level-1 one.  The single-cell stores are built with
a particle bound just above 2^15, where a cell of any size is cut into 256-particle items (below
it a cell of <= 1024 particles is one item and takes no ticket at all), so `256 k - 3` particles
are exactly k items at T <= 12; at T = 25 an item is 512 particles.  The nine-cell mix keeps its
natural bound, as the benchmark's scene does: 256-particle items, small cells whole.

For every shape: the one-launch cycle and the moments launch, each on a fresh workspace, against
the two-call path, bit for bit; moments against NumPy (ddof = 1) at test_gpu_root_gather.py's
tolerance; three launches in a row on one workspace (counters must be back at zero).  Then calls
of different shapes alternating on one grow-only workspace against fresh-workspace calls, and a
workspace 256 bytes short of the size function's answer, which must be refused before anything
is launched.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ABOVE_WHOLE = 2 ** 15 + 64      # particle bound: no whole-cell items, still 256-particle items
CCMPC_ERR_WORKSPACE = -3

# (T, items per cell, particles per item, store dtype, particle bound or None for the natural one)
SINGLE_T8 = [(8, (k,), 256, torch.float64, ABOVE_WHOLE) for k in (1, 2, 16, 17, 32, 33, 64, 65)]
MIX = (8, (5, 9, 20, 3, 14, 7, 11, 2, 8), 256, torch.float64, None)
OTHERS = [(1, (17,), 256, torch.float64, ABOVE_WHOLE),
          (12, (33,), 256, torch.float64, ABOVE_WHOLE),       # 4-row blocks
          (25, (17,), 512, torch.float64, None),              # four row blocks, 8-wave items
          (8, (33,), 256, torch.float32, ABOVE_WHOLE)]

_CLOUDS = {}


def _case(shape):
    """(cells, ref) of a shape, built once; every cell's last item is 3 particles short."""
    T, items, per, _, _ = shape
    key = (T, items, per)
    if key not in _CLOUDS:
        from ccmpc import synthetic
        rng = np.random.default_rng(np.random.Philox(9000 + 31 * T + len(items)))
        p0 = np.array([190.0, -80.0])
        cells = [synthetic.mode_cloud(rng, per * k - 3, T, p0) for k in items]
        for c in cells:
            c.setflags(write=False)
        _CLOUDS[key] = (cells, synthetic.ego_ref(9000 + T, T))
    return _CLOUDS[key]


def _store(gpu, shape):
    from ccmpc import engine
    _, _, _, dtype, bound = shape
    cells, _ = _case(shape)
    origin = np.array([c[:, 0].mean(0) for c in cells]) if dtype == torch.float32 else None
    return engine.ParticleStore.from_cells(cells, device=gpu, dtype=dtype, origin=origin,
                                           capacity=bound)


def _cycle(gpu, shape, store=None):
    from ccmpc import cycle
    store = store if store is not None else _store(gpu, shape)
    return cycle.MinkowskiCycle(store, [store.n_cells], _case(shape)[1])


def _outputs(cyc):
    return cyc.mean.clone(), cyc.cov.clone(), cyc.rec.clone(), cyc.prob_lower.clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _check(gpu, shape):
    from ccmpc import engine
    T, items, per, dtype, _ = shape
    store = _store(gpu, shape)
    assert [-(-n // per) for n in store.counts] == list(items)

    # the two-call path, then the one-launch cycle on a workspace of its own: same bits
    two = _cycle(gpu, shape, store)
    two.rec.zero_()
    two.run_unfused()
    want = _outputs(two)
    cyc = _cycle(gpu, shape, store)
    cyc.rec.zero_()
    cyc.run()
    assert _same(want, _outputs(cyc))
    # the moments launch on a fresh workspace
    m, c = engine.moments(store)
    assert torch.equal(m, want[0]) and torch.equal(c, want[1])

    # three launches in a row on one workspace: every launch left its counters at zero
    for _ in range(3):
        cyc.mean.zero_()
        cyc.cov.zero_()
        cyc.rec.zero_()
        cyc.prob_lower.zero_()
        cyc.run()
        assert _same(want, _outputs(cyc))

    # NumPy on the positions the store holds
    cells, _ = _case(shape)
    mean, cov = want[0].cpu().numpy(), want[1].cpu().numpy()
    for j in range(store.n_cells):
        traj = store.cell_positions(j) if dtype == torch.float32 else cells[j]
        X = traj.reshape(len(traj), 2 * T)
        np.testing.assert_allclose(cov[j], np.cov(X, rowvar=False), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(mean[j].reshape(-1), X.mean(0), rtol=1e-13)
    if 1 < T <= 12:
        assert np.all(cyc.records()["status"] == 0)


@pytest.mark.parametrize("shape", SINGLE_T8, ids=lambda s: f"{s[1][0]}items")
def test_single_cell_root_widths(gpu, shape):
    _check(gpu, shape)


def test_nine_cell_mix_with_a_20_item_cell(gpu):
    _check(gpu, MIX)


@pytest.mark.parametrize("shape", OTHERS,
                         ids=["T1-17items", "T12-33items", "T25-17items", "f32-33items"])
def test_other_geometries(gpu, shape):
    _check(gpu, shape)


def test_shapes_alternating_on_one_workspace(gpu):
    """Two tree levels, the nine-cell mix and a 4-row-block cell taking turns on ONE grow-only
    workspace: the buffer grows on the way, so a shape meets its counters at different places,
    and none may find another's slabs there.  Bits of fresh-workspace calls."""
    from ccmpc import engine
    shapes = {"A": SINGLE_T8[-1], "B": MIX, "C": OTHERS[1]}
    cycs, want = {}, {}
    for name, shape in shapes.items():
        cycs[name] = _cycle(gpu, shape)
        cycs[name].rec.zero_()
        cycs[name].run()                                      # on its own fresh workspace
        want[name] = _outputs(cycs[name])
    shared = engine.Workspace(gpu)
    for step, name in enumerate("BACACBA"):
        cyc = cycs[name]
        cyc.ws = shared
        for t in (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower):
            t.zero_()
        if step % 3 == 2:                                     # the moments launch shares it too
            m, c = engine.moments(cyc.store, workspace=shared)
            assert torch.equal(m, want[name][0]) and torch.equal(c, want[name][1]), (step, name)
        cyc.run()
        assert _same(want[name], _outputs(cyc)), (step, name)


@pytest.mark.parametrize("shape", [SINGLE_T8[-1], MIX], ids=["65items", "mix"])
def test_short_workspace_is_refused_before_any_launch(gpu, shape):
    from ccmpc import _lib, engine
    lib = _lib.load()
    T = shape[0]
    store = _store(gpu, shape)
    cyc = _cycle(gpu, shape, store)
    C = store.n_cells
    need = int(lib.ccmpc_moments_workspace_bytes(T, C, store.n_bound))
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    p = engine._p

    def moments(nbytes):
        return lib.ccmpc_moments(p(store.pos), store.ccmpc_dtype, store.ld, T, p(store.origin),
                                 p(store.cell_off), p(store.cell_cnt), C, store.n_bound, p(ws),
                                 nbytes, p(cyc.mean), p(cyc.cov), engine._stream())

    def fused(nbytes):
        return lib.ccmpc_minkowski_cycle(
            p(store.pos), store.ccmpc_dtype, store.ld, T, p(store.origin), p(store.cell_off),
            p(store.cell_cnt), C, store.n_bound, p(ws), nbytes, p(cyc.ref), p(cyc.cell_ref),
            p(cyc.risk), float(cyc.R), float(cyc.tol), int(cyc.maxiter), p(cyc.mean), p(cyc.cov),
            p(cyc.rec), p(cyc.prob_lower), engine._stream())

    for call in (moments, fused):
        for t in (cyc.mean, cyc.cov, cyc.prob_lower):
            t.fill_(7.0)
        cyc.rec.fill_(7)
        assert call(need - 256) == CCMPC_ERR_WORKSPACE
        torch.cuda.synchronize(gpu)
        assert bool((cyc.mean == 7.0).all()) and bool((cyc.cov == 7.0).all())
        assert bool((cyc.rec == 7).all()) and bool((cyc.prob_lower == 7.0).all())
        assert not bool(ws.any())                             # nothing was written to it either
    # premise: the size function's answer itself is enough
    assert moments(need) == 0 and fused(need) == 0
    torch.cuda.synchronize(gpu)
    assert bool(torch.isfinite(cyc.cov).all())
