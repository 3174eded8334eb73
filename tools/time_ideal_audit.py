"""Time ccmpc_ideal_risk_audit beside its parent and beside the materialised path.

    python tools/time_ideal_audit.py [--out ideal_audit_time.json] [--rounds 25] [--per-graph 10]

Shapes: 2 cells x 1e6 samples at T = 7 (DESIGN 4.3's shape) and 9 cells x 1e6 at T = 7, source
moments of T_src = 8.  On each shape the series alternate in one process, every series a
captured graph of `per-graph` calls timed with device events, `rounds` replays each after a
warm-up of every graph:
  moments_a / moments_b   ccmpc_ideal_moments, twice: the parent (the same sample generation,
                          with the Gram); its two readings give the spread
  materialised            ccmpc_ideal_rollout + ccmpc_risk_audit (plan and records) on the store
  ideal_plan              ccmpc_ideal_risk_audit, plan only
  ideal_plan_rec          ccmpc_ideal_risk_audit, plan + the cycle's own half-space records
The statement under test, reported either way: ideal_plan_rec is not slower than materialised
by more than three times the moments' spread.  The materialised path writes and re-reads
32 T n bytes per cell; the fused call moves none."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cc-mpc_amd")]

import torch  # noqa: E402

from ccmpc import _lib, engine, risk  # noqa: E402

SHAPES = {"2 x 1e6, T = 7": (2, 1_000_000, 7), "9 x 1e6, T = 7": (9, 1_000_000, 7)}
T_SRC = 8


def graph_of(fn, per_graph, dev):
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            fn()
    return g


def build(C, n, T, dev):
    """Source moments of a small random-walk store, the frame's own records and a plan row per
    cell: its mean path displaced by R along x, so the disc's edge passes through the cloud."""
    rng = np.random.default_rng(7)
    cells = [np.array([190.0 + 3 * c, 5.0 - 2 * c]) + np.cumsum(
        rng.normal([1.5, 0.1 * c], 0.6, size=(5000, T_SRC, 2)), axis=1) for c in range(C)]
    pm, pc = engine.moments(engine.ParticleStore.from_cells(cells, device=dev))
    src = torch.arange(C, dtype=torch.int32, device=dev)
    cr = torch.as_tensor(risk.cell_risk(risk.eps_ura([C]), [C], T_SRC), device=dev)
    ref = torch.as_tensor((np.array([170.0, 5.0]) + np.arange(1, T + 1)[:, None] * [4.0, 0.5])
                          [None], device=dev)
    ws = engine.Workspace(dev)
    mean, cov, status, rec, _ = engine.ideal_minkowski_cycle(pm, pc, src, T, n, ref, cr, seed=3,
                                                             workspace=ws)
    plan = (mean + torch.tensor([risk.R_COLLISION, 0.0], dtype=torch.float64,
                                device=dev)).contiguous()
    cell_plan = torch.arange(C, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * C
    return pm, pc, src, rec, plan, cell_plan, ws


def time_shape(name, dev, rounds, per_graph):
    C, n, T = SHAPES[name]
    pm, pc, src, rec, plan, cell_plan, ws = build(C, n, T, dev)
    lib = _lib.load()
    p = engine._p
    kind, R, seed = _lib.REC_KIND_HALFSPACE, risk.R_COLLISION, 3
    mean, cov, st = engine.ideal_moments(pm, pc, src, T, n, seed=seed, workspace=ws)
    store, st_r = engine.ideal_rollout(pm, pc, src, T, n, seed=seed)
    out_m = engine.risk_audit(store, plan=plan, cell_plan=cell_plan, rec=rec, rec_kind=kind, R=R)
    out_p = engine.ideal_risk_audit(pm, pc, src, T, n, plan=plan, cell_plan=cell_plan, R=R,
                                    seed=seed)
    out_pr = engine.ideal_risk_audit(pm, pc, src, T, n, plan=plan, cell_plan=cell_plan, rec=rec,
                                     rec_kind=kind, R=R, seed=seed)
    torch.cuda.synchronize()
    for k in ("hit", "hit_any", "rec_open", "open"):          # the two paths agree before timing
        assert torch.equal(getattr(out_m, k), getattr(out_pr[0], k)), k
    assert torch.equal(out_m.min_d2.view(torch.int64), out_pr[0].min_d2.view(torch.int64))
    assert torch.equal(out_p[0].hit, out_m.hit)

    def moments():
        engine.ideal_moments(pm, pc, src, T, n, seed=seed, workspace=ws, out_mean=mean,
                             out_cov=cov, out_status=st)

    def materialised():       # the rollout into the store held above (nothing allocated)
        _lib.check(lib.ccmpc_ideal_rollout(p(pm), p(pc), T_SRC, p(src), C, T, n, None, None, seed,
                                           None, p(store.pos), store.ld, p(st_r),
                                           engine._stream()), "ccmpc_ideal_rollout")
        engine.risk_audit(store, plan=plan, cell_plan=cell_plan, rec=rec, rec_kind=kind, R=R,
                          out=out_m)

    series = {
        "moments_a": moments,
        "materialised": materialised,
        "ideal_plan": lambda: engine.ideal_risk_audit(
            pm, pc, src, T, n, plan=plan, cell_plan=cell_plan, R=R, seed=seed, out=out_p),
        "moments_b": moments,
        "ideal_plan_rec": lambda: engine.ideal_risk_audit(
            pm, pc, src, T, n, plan=plan, cell_plan=cell_plan, rec=rec, rec_kind=kind, R=R,
            seed=seed, out=out_pr),
    }
    graphs = {k: graph_of(f, per_graph, dev) for k, f in series.items()}
    for g in graphs.values():                           # warm-up of every graph
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / per_graph)      # us per call
    res = dict(shape=name, cells=C, samples=n, T=T, T_src=T_SRC,
               materialised_store_bytes=16 * T * C * n,
               timed_calls_per_series=rounds * per_graph, series={})
    for k, v in times.items():
        v = np.asarray(v)
        res["series"][k] = dict(median_us=float(np.median(v)), min_us=float(v.min()),
                                max_us=float(v.max()))
    med = {k: v["median_us"] for k, v in res["series"].items()}
    res["moments_spread_us"] = abs(med["moments_a"] - med["moments_b"])
    res["ideal_plan_rec_minus_materialised_us"] = med["ideal_plan_rec"] - med["materialised"]
    res["not_slower_than_materialised_by_3_spreads"] = bool(
        res["ideal_plan_rec_minus_materialised_us"] <= 3 * res["moments_spread_us"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="ideal_audit_time.json")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--per-graph", type=int, default=10)
    args = ap.parse_args()
    _lib.load()
    dev = engine.require_device("cuda:0")
    results = []
    for name in SHAPES:
        r = time_shape(name, dev, args.rounds, args.per_graph)
        results.append(r)
        print(name + ": " + ", ".join(
            f"{k} {v['median_us']:.1f} [{v['min_us']:.1f}, {v['max_us']:.1f}]"
            for k, v in r["series"].items()) + " us per call; fused plan + records "
            f"{'is not' if r['not_slower_than_materialised_by_3_spreads'] else 'IS'} slower than "
            f"the materialised path by more than 3 x {r['moments_spread_us']:.1f} us", flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
