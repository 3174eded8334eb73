"""Time ccmpc_face_quantile beside its two parents on the same particle store: the full
ccmpc_face_audit call (whose arithmetic every counting pass repeats) and ccmpc_risk_quantile
(whose radix select it reuses).

    python tools/time_face_quantile.py [--out profiles/r21/face_quantile_time.json]
                                       [--rounds 25] [--per-graph 10]
    python tools/time_face_quantile.py --loop 5 --store "C4/8 f64"     # under a kernel trace
    python tools/time_face_quantile.py --planner [--frames 10]

Stores: C2 (4 OVs x 5 000, T = 8, f64) and the per-GPU C4 batch (8 scenes x 4 OVs x 20 000,
T = 12) as f64 and as f32 (tools/time_audit.py's, with its Minkowski records for
ccmpc_risk_quantile).  On each store four series alternate in one process -- face audit (out_worst
on, no face_sel), risk quantile, face quantile, face audit again -- every series a captured graph
of `per-graph` calls timed with device events, `rounds` replays each after a warm-up of every
graph; median [min, max] per call.  The two face-audit series give the spread a difference has
to clear.  allow is risk.allow_counts per scene, as tools/time_quantile.py's.
--loop: eager calls of the face quantile only, for a kernel trace (the per-pass times).
--planner: the host clock of MidlevelAgent.solve_planning_socp and tighten_face_plan, frame by
frame, on the golden scene faces_o2_t8 with its reference shifted 10 m."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cc-mpc_amd"), os.path.join(ROOT, "tools")]

STORE_NAMES = ["C2", "C4/8 f64", "C4/8 f32"]
PASSES = 8


def setup(name, dev):
    import torch

    import time_audit
    from ccmpc import engine, risk
    store, cyc, T = time_audit.build(name, dev)
    O = time_audit.STORES[name][0]                      # every scene allocates its own risk
    parts, c0 = [], 0
    for o0 in range(0, len(cyc.K), O):
        K_s = cyc.K[o0:o0 + O]
        parts.append(risk.allow_counts(store.counts[c0:c0 + sum(K_s)], K_s, T))
        c0 += sum(K_s)
    allow = torch.as_tensor(np.concatenate(parts), device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    past = np.array([store.cell_positions(j)[:, 0].mean(0) - np.array([3.0, 0.7])
                     for j in range(store.n_cells)])
    w = dict(store=store, cyc=cyc, T=T, allow=allow, plan=cyc.ref.contiguous(),
             cell_plan=cyc.cell_ref, past=torch.as_tensor(past, **f64).contiguous(),
             extent=torch.as_tensor(np.array([3.7, 1.79]), **f64))
    kw = dict(cell_plan=w["cell_plan"], extent=w["extent"])
    w["audit"] = engine.face_audit(store, w["past"], w["plan"], **kw)
    w["rq"] = cyc.calibrate(allow)
    need = int(engine._lib.load().ccmpc_face_quantile_workspace_bytes(T, store.n_cells))
    w["ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
    w["fq"] = engine.face_quantile(store, w["past"], w["plan"], allow=allow, workspace=w["ws"],
                                   **kw)
    torch.cuda.synchronize()
    return w


def series_of(w):
    from ccmpc import engine
    store = w["store"]
    kw = dict(cell_plan=w["cell_plan"], extent=w["extent"])

    def audit():
        engine.face_audit(store, w["past"], w["plan"], out=w["audit"], **kw)
    return {
        "face_audit_a": audit,
        "risk_quantile": lambda: w["cyc"].calibrate(w["allow"], out=w["rq"]),
        "face_quantile": lambda: engine.face_quantile(store, w["past"], w["plan"],
                                                      allow=w["allow"], out=w["fq"],
                                                      workspace=w["ws"], **kw),
        "face_audit_b": audit,
    }


def time_store(name, dev, rounds, per_graph):
    import torch

    import time_audit
    w = setup(name, dev)
    store, T = w["store"], w["T"]
    graphs = {k: time_audit.graph_of(f, per_graph, dev) for k, f in series_of(w).items()}
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
    status = w["fq"].status.cpu().numpy()
    q = w["fq"].q.cpu().numpy()
    res = dict(store=name, particles=n, cells=store.n_cells, T=T,
               dtype="f32" if store.dtype == torch.float32 else "f64",
               rows=int(status.size * 4), selected_rows=int((status == 0).sum() * 4),
               rows_within_budget=int(np.sum(q[status == 0] <= 0)),
               workspace_bytes=int(w["ws"].numel()),
               risk_quantile_records_per_cell=int(w["rq"].status.shape[1]),
               timed_calls_per_series=rounds * per_graph, series={})
    for k, v in times.items():
        v = np.asarray(v)
        res["series"][k] = dict(median_us=float(np.median(v)), min_us=float(v.min()),
                                max_us=float(v.max()))
    s = res["series"]
    a, b = s["face_audit_a"]["median_us"], s["face_audit_b"]["median_us"]
    fq = s["face_quantile"]["median_us"]
    res["parent_spread_us"] = abs(a - b)
    res["face_quantile_over_face_audit"] = fq / (0.5 * (a + b))
    res["face_quantile_over_risk_quantile"] = fq / s["risk_quantile"]["median_us"]
    return res


def loop_store(name, dev, n):
    """n eager face quantile calls on one store (kernel times come from the profiler)."""
    import torch
    w = setup(name, dev)
    fn = series_of(w)["face_quantile"]
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    print(f"{name}: {n} calls of the face quantile")


def planner_frames(dev, frames):
    """Host-clock time of solve_planning_socp and of tighten_face_plan (which contains it)."""
    import torch

    from ccmpc import ovehicle, planner
    g = np.load(os.path.join(ROOT, "tests", "golden", "faces_o2_t8.npz"), allow_pickle=False)
    T, K = int(g["T"]), [int(k) for k in g["K"]]
    flat = iter(np.split(g["positions"], np.cumsum(g["counts"])[:-1]))
    cells = [[next(flat) for _ in range(k)] for k in K]
    ref = g["ref_traj"][:T] + 10.0 * np.array([np.cos(np.radians(45.0)), np.sin(np.radians(45.0))])
    step = ref[1] - ref[0]
    x_init = np.array([*(ref[0] - step), np.arctan2(step[1], step[0]), 6.0])
    goal = ref[-1].copy()
    ovs = ovehicle.scene_from_positions(cells, g["past"], device=dev)
    agent = planner.MidlevelAgent(prediction_horizon=T, device=dev)

    class Params:
        O, frame = len(K), 100
    Params.K = np.asarray(K)
    agent.compute_obstacle_constraints_GMM_approx(Params, ovs, None, None, None, g["eps_ura"],
                                                  None, T, ref)
    out = dict(scene="faces_o2_t8 + 10 m", frames=frames, series={})

    def socp():
        return agent.solve_planning_socp(x_init, goal, ref, T, tol_g=1e-6)

    def tighten():
        try:
            r = agent.tighten_face_plan(x_init, goal, ref, T, tol_g=1e-6)
            return dict(status=0, tighten_rounds=r["tighten_rounds"], socp_rounds=r["rounds"])
        except planner.InSimulationException as e:
            return dict(status=int(getattr(e, "status", -1)),
                        tighten_rounds=int(getattr(e, "tighten_rounds", -1)))
    for name, fn in (("solve_planning_socp", socp), ("tighten_face_plan", tighten)):
        fn()                                            # warm-up: buffers, workspaces
        torch.cuda.synchronize()
        ts = []
        for _ in range(frames):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = np.asarray(ts)
        out["series"][name] = dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()),
                                   max_ms=float(ts.max()))
        if name == "tighten_face_plan":
            out["tighten_outcome"] = r
        else:
            out["socp_rounds"] = int(r["rounds"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--per-graph", type=int, default=10)
    ap.add_argument("--loop", type=int, default=0, help="profiler mode: eager calls, no timing")
    ap.add_argument("--store", default=None, choices=STORE_NAMES)
    ap.add_argument("--planner", action="store_true")
    ap.add_argument("--frames", type=int, default=10)
    args = ap.parse_args()
    import torch

    from ccmpc import _lib, engine
    _lib.load()
    dev = engine.require_device("cuda:0")
    names = [args.store] if args.store else STORE_NAMES
    if args.loop:
        for name in names:
            loop_store(name, dev, args.loop)
        return
    if args.planner:
        payload = planner_frames(dev, args.frames)
        print(json.dumps(payload), flush=True)
        default = os.path.join("profiles", "r21", "face_quantile_planner_time.json")
    else:
        results = []
        for name in names:
            r = time_store(name, dev, args.rounds, args.per_graph)
            results.append(r)
            s = r["series"]
            print(f"{name}: face audit {s['face_audit_a']['median_us']:.1f} / "
                  f"{s['face_audit_b']['median_us']:.1f} us, risk quantile "
                  f"{s['risk_quantile']['median_us']:.1f} us, face quantile "
                  f"{s['face_quantile']['median_us']:.1f} us "
                  f"[{s['face_quantile']['min_us']:.1f}, {s['face_quantile']['max_us']:.1f}] = "
                  f"{r['face_quantile_over_face_audit']:.2f} face audits", flush=True)
        payload = dict(results=results)
        default = os.path.join("profiles", "r21", "face_quantile_time.json")
    out = args.out or default
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), **payload), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
