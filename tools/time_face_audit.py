"""Time ccmpc_face_audit beside ccmpc_risk_audit (plan only) and ccmpc_face_constraints (robust)
on the same particle store.

    python tools/time_face_audit.py [--out profiles/r20/face_audit_time.json] [--rounds 25]
                                    [--per-graph 10]

Stores: C2 (4 OVs x 5 000, T = 8, f64) and the per-GPU C4 batch (8 scenes x 4 OVs x 20 000,
T = 12) as f64 and as f32 (tools/time_audit.py's).  On each store five series alternate in one
process -- risk audit (plan only), face audit without face_sel and without out_worst, risk audit
again, face audit with everything, face constraints (robust) -- every series a captured graph
of `per-graph` calls timed with device events, `rounds` replays each after a warm-up of every
graph.  The two risk-audit series give the spread a difference has to clear three times over.
Algorithmic bytes are the store planes read once: 16 T sum(N) (f64) or 8 T sum(N) (f32); the
fraction is of the 8 TB/s HBM peak (the face constraints read (2T - 1) / T times as much).
Every call is two launches and is timed as the call."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cc-mpc_amd")]

import torch  # noqa: E402

from ccmpc import _lib, engine, synthetic  # noqa: E402

STORES = {"C2": (4, 5000, 8, 1, False), "C4/8 f64": (4, 20000, 12, 8, False),
          "C4/8 f32": (4, 20000, 12, 8, True)}
HBM_PEAK = 8e12
R = 3.4


def build(name, dev):
    O, N, T, scenes, f32 = STORES[name]
    cells, refs, cell_plan = [], [], []
    for sc in range(scenes):
        ovs, ref, _ = synthetic.scene(1000 + sc, O=O, N=N, T=T)
        for o in ovs:
            cells += list(o)
            cell_plan += [sc] * len(o)
        refs.append(np.asarray(ref, np.float64)[:T, :2])
    if f32:
        origin = np.tile(np.array([150.0, -120.0]), (len(cells), 1))
        store = engine.ParticleStore.from_cells(cells, device=dev, dtype=torch.float32,
                                                origin=origin)
    else:
        store = engine.ParticleStore.from_cells(cells, device=dev)
    past = np.array([c[:, 0].mean(0) - np.array([3.0, 0.7]) for c in cells])
    f64 = dict(dtype=torch.float64, device=dev)
    C = len(cells)
    rng = np.random.default_rng(5)
    return dict(store=store, T=T,
                plan=torch.as_tensor(np.stack(refs), **f64).contiguous(),
                cell_plan=torch.as_tensor(np.asarray(cell_plan, np.int32), device=dev),
                past=torch.as_tensor(past, **f64).contiguous(),
                extent=torch.as_tensor(np.array([3.7, 1.79]), **f64),
                gamma=torch.full((C,), 2.0, **f64),
                face_sel=torch.as_tensor(rng.integers(0, 4, (C, T)).astype(np.int32), device=dev))


def face_constraints_call(w, dev):
    """ccmpc_face_constraints (robust) on device-resident inputs: capturable."""
    lib = _lib.load()
    store, T = w["store"], w["T"]
    C = store.n_cells
    need = lib.ccmpc_face_workspace_bytes(T, C, store.n_bound)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rec = torch.empty((C, T, 4, 128), dtype=torch.uint8, device=dev)
    p = engine._p

    def call():
        _lib.check(lib.ccmpc_face_constraints(
            p(store.pos), store.ccmpc_dtype, store.ld, T, p(store.origin), p(store.cell_off),
            p(store.cell_cnt), C, store.n_bound, p(w["past"]), p(w["extent"]), p(w["gamma"]),
            p(w["plan"]), p(w["cell_plan"]), _lib.FACE_ROBUST, 4.47213, p(ws), ws.numel(), p(rec),
            engine._stream()), "ccmpc_face_constraints")
    call.keep = (ws, rec)
    return call


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
    w = build(name, dev)
    store, T = w["store"], w["T"]
    kw = dict(cell_plan=w["cell_plan"], extent=w["extent"])
    out_p = engine.risk_audit(store, plan=w["plan"], cell_plan=w["cell_plan"], R=R)
    out_lean = engine.face_audit(store, w["past"], w["plan"], worst=False, **kw)
    out_full = engine.face_audit(store, w["past"], w["plan"], face_sel=w["face_sel"], **kw)
    torch.cuda.synchronize()

    def risk():
        engine.risk_audit(store, plan=w["plan"], cell_plan=w["cell_plan"], R=R, out=out_p)
    series = {
        "risk_audit_plan_a": risk,
        "face_audit_lean": lambda: engine.face_audit(store, w["past"], w["plan"], worst=False,
                                                     out=out_lean, **kw),
        "risk_audit_plan_b": risk,
        "face_audit_full": lambda: engine.face_audit(store, w["past"], w["plan"],
                                                     face_sel=w["face_sel"], out=out_full, **kw),
        "face_constraints_robust": face_constraints_call(w, dev),
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
    s = res["series"]
    a, b = s["risk_audit_plan_a"]["median_us"], s["risk_audit_plan_b"]["median_us"]
    res["parent_spread_us"] = abs(a - b)
    res["face_audit_full_minus_parent_us"] = s["face_audit_full"]["median_us"] - 0.5 * (a + b)
    res["face_audit_full_minus_face_constraints_us"] = (
        s["face_audit_full"]["median_us"] - s["face_constraints_robust"]["median_us"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r20", "face_audit_time.json"))
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--per-graph", type=int, default=10)
    args = ap.parse_args()
    _lib.load()
    dev = engine.require_device("cuda:0")
    results = []
    for name in STORES:
        r = time_store(name, dev, args.rounds, args.per_graph)
        results.append(r)
        s = r["series"]
        print(f"{name}: risk audit (plan) {s['risk_audit_plan_a']['median_us']:.2f} / "
              f"{s['risk_audit_plan_b']['median_us']:.2f} us, face audit lean "
              f"{s['face_audit_lean']['median_us']:.2f} us, full "
              f"{s['face_audit_full']['median_us']:.2f} us "
              f"({s['face_audit_full']['fraction_of_8TBps']:.2f} of 8 TB/s), face constraints "
              f"robust {s['face_constraints_robust']['median_us']:.2f} us", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
