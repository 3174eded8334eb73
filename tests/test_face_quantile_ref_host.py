"""tests/_face_quantile_ref.py against itself (host only): the selection restated against a
plain sort, the counting identity of an order statistic, the cut's support identity and that the
cut is the arg particle's own face half-space."""
import numpy as np
import pytest

import _face_audit_ref as ar
import _face_quantile_ref as qr
from _l4_ref import LD, store_world

CASES = [(8, False), (9, True), (1, False), (2, True)]
HLON = 0.5 * ar.LON + 0.5 * ar.CAR_R


@pytest.mark.parametrize("T,f32", CASES)
def test_selection_is_the_plain_sort_and_counts_as_an_order_statistic(T, f32):
    ref = ar.reference(T, f32)
    seen = 0
    for k in range(len(qr.M_NAMES)):
        for r, d in zip(ref, qr.reference(T, f32, k)):
            assert d["status"] == qr.status_of(d["n"], d["m"])
            if d["status"]:
                assert d["m"] < 0 or d["m"] >= d["n"]
                continue
            seen += 1
            n, m = d["n"], d["m"]
            for v, q, arg in ((r["v64"], d["q64"], d["arg64"]), (r["vld"], d["qld"], d["argld"])):
                w = v + v.dtype.type(0)
                assert np.array_equal(q, np.sort(w, axis=0)[n - 1 - m])
                if n <= 65:                               # an independent sort, value by value
                    for t in range(T):
                        for f in range(4):
                            assert q[t, f] == sorted(w[:, t, f].tolist())[n - 1 - m]
                assert np.all((w > q[None]).sum(0) <= m)
                assert np.all((w >= q[None]).sum(0) > m)
                tt, ff = np.meshgrid(np.arange(T), np.arange(4), indexing="ij")
                assert np.array_equal(w[arg, tt, ff], q)
                first = np.argmax(w == q[None], axis=0)
                assert np.array_equal(arg, first)
    assert seen > 0


def test_allows_cover_every_status():
    sts = {qr.status_of(n, m) for n in ar.counts_of(False) for m in qr.allows_of(n)}
    assert sts == {0, qr.VACUOUS, qr.SKIPPED}
    assert qr.allows_of(1024) == (0, 1, 3, 1023, 1024, -1)
    assert qr.status_of(0, 0) == qr.VACUOUS and qr.status_of(0, -1) == qr.SKIPPED


@pytest.mark.parametrize("T,f32", CASES)
@pytest.mark.parametrize("margin", [0.0, 1e-6, 0.25])
def test_cut_supports_q_and_is_the_arg_particles_own_half_space(T, f32, margin):
    inp = ar.inputs(T, f32)
    ref = ar.reference(T, f32)
    world = store_world(inp["cells"], bool(f32), inp["origin"])
    rng = np.random.default_rng(3)
    worst = 0.0
    for j, (r, d) in enumerate(zip(ref, qr.reference(T, f32, 2))):
        if d["status"]:
            continue
        plan = inp["plan"][inp["cell_plan"][j]]
        n64, rhs64 = qr.cut(world[j], inp["past"][j], plan, d["q64"], d["arg64"], margin)
        # support: n . P - rhs == q + margin, to rounding of the terms it is made of
        P = plan[:T, :2].astype(LD)
        sup = n64[..., 0].astype(LD) * P[:, None, 0] + n64[..., 1].astype(LD) * P[:, None, 1] - rhs64
        terms = (np.abs(n64[..., 0] * plan[:T, None, 0]) + np.abs(n64[..., 1] * plan[:T, None, 1])
                 + np.abs(d["q64"]) + margin)
        e = np.abs(sup - d["q64"].astype(LD) - LD(margin)) / terms
        worst = max(worst, float(e.max()))
        assert np.all(e <= 1e-15)
        # the cut is v_f's own half-space: v_f(x; arg) == n . x - rhs - margin for any x
        for _ in range(3):
            x = plan[:T, :2] + rng.uniform(-30, 30, size=(T, 2))
            v, ex, ey = ar.values(world[j], inp["past"][j], x, ld=True)
            tt, ff = np.meshgrid(np.arange(T), np.arange(4), indexing="ij")
            a = d["arg64"]
            lin = (n64[..., 0].astype(LD) * x[:, None, 0] + n64[..., 1].astype(LD) * x[:, None, 1]
                   - rhs64 - LD(margin))
            scale = (np.abs(ex[a, tt]) + np.abs(ey[a, tt]) + HLON
                     + np.abs(plan[:T, None, 0] - x[:, None, 0])
                     + np.abs(plan[:T, None, 1] - x[:, None, 1]))
            assert np.all(np.abs(v[a, tt, ff] - lin) <= 1e-13 * scale)
    print("support identity, worst relative error:", worst)


def test_tie_cells_hold_every_value_twice():
    cells, past, plan, _ = qr.tie_store_cells()
    v, _, _ = ar.values(cells[0], past[0], plan[0], ar.TIE_EXTENT, ar.TIE_CAR_R)
    assert np.array_equal(v[:12], v[12:])
    for m in (0, 1, 2, 3, 5, 23):
        q, arg = qr.select(v, m)
        assert np.all(arg < 12)
        assert np.all((v + 0.0 == q[None]).sum(0) >= 2)
