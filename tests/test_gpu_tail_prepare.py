"""The fused half-space tail (constraints.hpp minkowski_cell) against the unfused rows launch,
bit for bit, at every layout of the tail:

  T = 1    P = 0    no record, the lower-bound wave still writes prob_lower
  T = 2    P = 1    one record lane, one lower-bound lane
  T = 8    P = 28   the benchmark's shape
  T = 12   P = 66   two pairs on the first lanes of the lower-bound wave (4-row-block kernel)
  T = 25   P = 300  the looped layout (every thread takes whole pairs), on the fused rollout's
                    tail; the particle-store cycle runs the rows launch itself above T = 24

Each particle-store case holds cells of several work items (the tail follows an arrival ticket
and a root gather, of one group and of two) and a cell of one item (it follows the workgroup's own
combine).

Written for a split of the tail into an index step ahead of the arrival's waits and a run step,
with the MVOE fixed point testing its exit once per two updates (profiles/r09: built, measured,
not kept).  A loop of that form must not let a lane finished by the first update of a pair take
the second, so the T = 8 case holds fixed points that end on an odd and on an even update:
counted on the oracle's compute_mvoe and asserted as a premise.
"""
import numpy as np
import pytest
import torch

from oracle import ccmpc_oracle as orc

pytestmark = pytest.mark.gpu


def _clouds(T, counts, seed):
    from ccmpc import synthetic
    rng = np.random.default_rng(np.random.Philox(seed))
    p0 = np.array([190.0, -80.0])
    return [synthetic.mode_cloud(rng, n, T, p0) for n in counts], synthetic.ego_ref(seed, T)


def _fused_and_two_calls(gpu, T, counts, seed):
    from ccmpc import cycle, engine
    cells, ref = _clouds(T, counts, seed)
    store = engine.ParticleStore.from_cells(cells, device=gpu)
    cyc = cycle.MinkowskiCycle(store, [len(cells)], ref)
    for t in (cyc.rec, cyc.prob_lower):
        t.zero_()
    cyc.run_unfused()
    want = (cyc.mean.clone(), cyc.cov.clone(), cyc.rec.clone(), cyc.prob_lower.clone())
    for t in (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower):
        t.zero_()
    cyc.run()
    got = (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    P = T * (T - 1) // 2
    if P:
        w, g = engine.halfspaces(want[2]).reshape(-1), cyc.records().reshape(-1)
        assert len(g) == len(cells) * P
        for f in ("which", "side", "status", "t_tau"):
            np.testing.assert_array_equal(g[f], w[f])
        assert np.all(g["status"] == 0)
    pl = cyc.prob_lower.cpu().numpy()
    assert np.all(pl[:, 0] == 1.0) and np.all((pl >= 0.0) & (pl <= 1.0))
    return cells, cyc


@pytest.mark.parametrize("T", [1, 2, 8, 12])
def test_fused_tail_equals_rows_launch(gpu, T):
    # 5 items + a ragged one, one whole item, 17 items (a two-group root)
    _fused_and_two_calls(gpu, T, (1400, 200, 4200), 300 + T)


def test_mvoe_exit_on_odd_and_even_updates(gpu):
    from ccmpc import risk
    T = 8
    cells, cyc = _fused_and_two_calls(gpu, T, (1400, 3000), 77)
    cr = cyc.risk.cpu().numpy()
    parities = []
    for j, c in enumerate(cells):
        C = np.cov(c.reshape(len(c), 2 * T), rowvar=False)
        seen = set()
        for t in range(1, T):
            for tau in range(t):
                idx = [2 * t, 2 * t + 1, 2 * tau, 2 * tau + 1]
                S = C[np.ix_(idx, idx)]
                c_t, c_x, c_tau = S[:2, :2], S[:2, 2:], S[2:, 2:]
                cov_mu = c_x @ np.linalg.inv(c_tau) @ c_x.T
                _, Q, it1 = orc.compute_mvoe(cr[j, 0] * (c_t - cov_mu), cr[j, 1] * cov_mu)
                _, _, it2 = orc.compute_mvoe(Q, risk.R_COLLISION ** 2 * np.eye(2))
                seen |= {it1 % 2, it2 % 2}
        parities.append(seen)
    # premise: every cell holds fixed points of both parities (4 to 6 updates on these clouds)
    assert all(s == {0, 1} for s in parities), parities


def test_looped_layout_on_the_rollout_tail(gpu):
    """P = 300 at T = 25: the fused ideal rollout's tail against ideal_moments + the rows launch."""
    from ccmpc import engine as e, risk
    T_src, Tn, ns = 26, 25, 20_000
    rng = np.random.default_rng(41)
    cells = [190 + np.cumsum(rng.normal(0, 0.4, size=(n, T_src, 2)), axis=1) for n in (900, 1500)]
    store = e.ParticleStore.from_cells(cells, device=gpu)
    mean, cov = e.moments(store)
    src = torch.tensor([0, 1], dtype=torch.int32, device=gpu)
    cr = torch.as_tensor(risk.cell_risk(risk.eps_ura([2]), [2], T_src), device=gpu)
    ref = torch.as_tensor((np.array([170.0, 5.0]) + np.arange(1, Tn + 1)[:, None] * [4.0, 0.5])
                          [None], device=gpu)
    m1, c1, _ = e.ideal_moments(mean, cov, src, Tn, ns, seed=9)
    r1, pl1 = e.minkowski(m1, c1, ref, cr)
    m2, c2, st2, r2, pl2 = e.ideal_minkowski_cycle(mean, cov, src, Tn, ns, ref, cr, seed=9)
    assert torch.equal(m1, m2) and torch.equal(c1, c2)
    assert torch.equal(r1, r2) and torch.equal(pl1, pl2)
    assert st2.cpu().tolist() == [0, 0]
    h = e.halfspaces(r2).reshape(-1)
    assert len(h) == 2 * 300
