"""Time ccmpc_risk_audit beside ccmpc_moments on the same particle store.

    python tools/time_audit.py [--out audit_time.json] [--rounds 25] [--per-graph 10]
    rocprofv3 --kernel-trace --stats ... -- python tools/time_audit.py --loop 200 --store "C4/8 f64"
        (no timing: 200 eager calls of each series on one store, for a profiler run of its own)

Stores: C2 (4 OVs x 5 000, T = 8, f64) and the per-GPU C4 batch (8 scenes x 4 OVs x 20 000,
T = 12) as f64 and as f32.  On each store four series alternate in one process -- moments,
audit (plan only), moments again, audit (plan + half-space records) -- every series a captured
graph of `per-graph` calls timed with device events, `rounds` replays each after a warm-up of
every graph (rounds x per-graph >= 200 timed calls per series).  The two moments series give
the spread the comparison has to clear.  Algorithmic bytes are the store planes read once:
16 T sum(N) (f64) or 8 T sum(N) (f32); the fraction is of the 8 TB/s HBM peak.  An audit call is
two launches (initial values, then the pass) and is timed as the call."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cc-mpc_amd")]

import torch  # noqa: E402

from ccmpc import _lib, cycle, engine, synthetic  # noqa: E402

STORES = {"C2": (4, 5000, 8, 1, False), "C4/8 f64": (4, 20000, 12, 8, False),
          "C4/8 f32": (4, 20000, 12, 8, True)}
HBM_PEAK = 8e12


def build(name, dev):
    O, N, T, scenes, f32 = STORES[name]
    cells, K, scene_K, refs = [], [], [], []
    for sc in range(scenes):
        ovs, ref, _ = synthetic.scene(1000 + sc, O=O, N=N, T=T)
        cells += [c for o in ovs for c in o]
        scene_K.append([len(o) for o in ovs])
        K += scene_K[-1]
        refs.append(ref)
    if f32:
        origin = np.tile(np.array([150.0, -120.0]), (len(cells), 1))
        store = engine.ParticleStore.from_cells(cells, device=dev, dtype=torch.float32,
                                                origin=origin)
    else:
        store = engine.ParticleStore.from_cells(cells, device=dev)
    cyc = cycle.MinkowskiCycle(store, K, np.stack(refs), scene_K=scene_K)
    cyc.run()
    torch.cuda.synchronize()
    return store, cyc, T


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


def time_store(name, dev, rounds, per_graph):
    store, cyc, T = build(name, dev)
    plan = cyc.ref                                      # one reference trajectory per scene
    cell_plan = cyc.cell_ref
    out_p = engine.risk_audit(store, plan=plan, cell_plan=cell_plan, R=cyc.R)
    out_pr = cyc.audit(plan, cell_plan=cell_plan)
    mean, cov = torch.empty_like(cyc.mean), torch.empty_like(cyc.cov)
    series = {
        "moments_a": lambda: engine.moments(store, mean, cov, cyc.ws),
        "audit_plan": lambda: engine.risk_audit(store, plan=plan, cell_plan=cell_plan, R=cyc.R,
                                                out=out_p),
        "moments_b": lambda: engine.moments(store, mean, cov, cyc.ws),
        "audit_plan_rec": lambda: cyc.audit(plan, cell_plan=cell_plan, out=out_pr),
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
    n = int(sum(store.counts))
    nbytes = (8 if store.dtype == torch.float32 else 16) * T * n
    res = dict(store=name, particles=n, cells=store.n_cells, T=T,
               dtype="f32" if store.dtype == torch.float32 else "f64", algorithmic_bytes=nbytes,
               timed_calls_per_series=rounds * per_graph, series={})
    for k, v in times.items():
        v = np.asarray(v)
        med = float(np.median(v))
        res["series"][k] = dict(median_us=med, min_us=float(v.min()), max_us=float(v.max()),
                                fraction_of_8TBps=nbytes / (med * 1e-6) / HBM_PEAK)
    a, b = res["series"]["moments_a"]["median_us"], res["series"]["moments_b"]["median_us"]
    res["moments_spread_us"] = abs(a - b)
    res["audit_plan_minus_moments_us"] = res["series"]["audit_plan"]["median_us"] - 0.5 * (a + b)
    return res


def loop_store(name, dev, n):
    """n eager calls of each series on one store (kernel times come from the profiler)."""
    store, cyc, T = build(name, dev)
    plan, cell_plan = cyc.ref, cyc.cell_ref
    out_p = engine.risk_audit(store, plan=plan, cell_plan=cell_plan, R=cyc.R)
    out_pr = cyc.audit(plan, cell_plan=cell_plan)
    for _ in range(n):
        engine.moments(store, cyc.mean, cyc.cov, cyc.ws)
        engine.risk_audit(store, plan=plan, cell_plan=cell_plan, R=cyc.R, out=out_p)
        cyc.audit(plan, cell_plan=cell_plan, out=out_pr)
    torch.cuda.synchronize()
    print(f"{name}: {n} calls of moments, audit (plan), audit (plan + records)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", type=int, default=0, help="profiler mode: eager calls, no timing")
    ap.add_argument("--store", default="C4/8 f64", choices=sorted(STORES))
    ap.add_argument("--out", default="audit_time.json")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--per-graph", type=int, default=10)
    args = ap.parse_args()
    if args.rounds * args.per_graph < 200:
        raise SystemExit("at least 200 timed calls per series")
    _lib.load()
    dev = engine.require_device("cuda:0")
    if args.loop:
        loop_store(args.store, dev, args.loop)
        return
    results = []
    for name in STORES:
        r = time_store(name, dev, args.rounds, args.per_graph)
        results.append(r)
        s = r["series"]
        print(f"{name}: moments {s['moments_a']['median_us']:.2f} / "
              f"{s['moments_b']['median_us']:.2f} us, audit plan "
              f"{s['audit_plan']['median_us']:.2f} us ({s['audit_plan']['fraction_of_8TBps']:.2f} "
              f"of 8 TB/s), plan + records {s['audit_plan_rec']['median_us']:.2f} us", flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
