"""Time mpc.PlanningSOCP (outer approximation over the planning QP) for one scene and for 64.

    python tools/time_socp.py [--out profiles/r18/socp_time.json] [--frames 50] [--rounds 25]
                              [--per-graph 10]

The scene is tests/_socp_ref.instance(6.0): the golden two-OV scene with its reference shifted
6 m, T = 8, two gated cells, one cone row active at the optimum, 4 rounds at tol_g = 1e-6.  The
batch is 64 copies of it with shifts spread over 6 .. 15 m.  Two measurements:

 * solved frames: PlanningSOCP.solve end to end on the host clock (round-0 cuts, then per round
   the QP launch, the cuts launch and the read-back), `frames` times after a warm-up; reported
   per frame and per round (frame time / rounds of the slowest scene).
 * one round on the device: a captured graph of `per-graph` x (PlanningQP.solve on the final
   pool, ccmpc_face_cuts at its X) alternated with a graph of `per-graph` x the same
   PlanningQP.solve alone -- the parent: the QP on a pool of the same row count -- timed with
   device events, `rounds` replays each.  The difference is what the cuts launch adds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cc-mpc_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import _socp_ref as sr  # noqa: E402
from ccmpc import _lib, engine, mpc  # noqa: E402


def graph_of(fn, n, dev):
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    return g


def time_batch(shifts, dev, frames, rounds, per_graph):
    probs = [sr.instance(float(m)) for m in shifts]
    T, S = probs[0]["T"], len(probs)
    f64 = dict(dtype=torch.float64, device=dev)
    rec = np.concatenate([sr.pack_face_records(p["cells_out"], T) for p in probs])
    rec = torch.as_tensor(np.ascontiguousarray(rec).view(np.uint8).reshape(-1), device=dev)
    cells = [len(p["cells_out"]) for p in probs]
    run = mpc.PlanningSOCP(cells, T, device=dev)
    xbar, gamma = mpc.ltv(np.array([p["x_init"] for p in probs]), T, Ts=sr.TS, lon=sr.LON)
    ref = torch.as_tensor(np.array([p["ref"] for p in probs]), **f64)
    goal = torch.as_tensor(np.array([p["goal"] for p in probs]), **f64)
    cg = torch.as_tensor(np.concatenate([p["cell_gamma"] for p in probs]), **f64)

    def frame():
        return run.solve(gamma, xbar, goal, ref, rec, cg, ref)

    for _ in range(3):
        res = frame()
    torch.cuda.synchronize()
    wall = []
    for _ in range(frames):
        t0 = time.perf_counter()
        res = frame()
        wall.append((time.perf_counter() - t0) * 1e6)
    n_rounds = int(res.rounds.max())

    # one round on the device, on the pool the last frame left (every region it used filled)
    def qp_only():
        run.qp.solve(gamma, xbar, goal, ref, run.pool)

    # the timed cuts go to a pool of their own, so the QP reads the same problem in every replay,
    # with a tolerance nothing meets and a state that says "cutting": every row is cut and stored
    pool2, g2, viol2 = torch.empty_like(run.pool), torch.empty_like(run.g), torch.empty_like(
        run.viol)
    state2 = torch.full_like(run.state, _lib.SOCP_CUT)

    def qp_and_cuts():
        _, X, _, _, _ = run.qp.solve(gamma, xbar, goal, ref, run.pool)
        engine.face_cuts(rec, T, run.scene_cell, run.n_cells, cg, X, pool2, run.pool_cell, g2,
                         viol2, state2, run.max_rounds, run.max_rounds, -1e300)

    graphs = {"qp_a": graph_of(qp_only, per_graph, dev),
              "qp_cuts": graph_of(qp_and_cuts, per_graph, dev),
              "qp_b": graph_of(qp_only, per_graph, dev)}
    for g in graphs.values():
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
            times[k].append(e0.elapsed_time(e1) * 1e3 / per_graph)
    med = {k: float(np.median(v)) for k, v in times.items()}
    wall = np.asarray(wall)
    return dict(scenes=S, T=T, cells=int(sum(cells)), pool_rows_per_scene=(run.max_rounds + 1)
                * max(cells) * T, status=[int(s) for s in np.unique(res.status)],
                rounds_max=n_rounds, rounds_mean=float(res.rounds.mean()),
                frame_us_median=float(np.median(wall)), frame_us_min=float(wall.min()),
                round_us=float(np.median(wall)) / n_rounds,
                device_round_us=med, device_qp_spread_us=abs(med["qp_a"] - med["qp_b"]),
                device_cuts_added_us=med["qp_cuts"] - 0.5 * (med["qp_a"] + med["qp_b"]),
                timed_calls_per_series=rounds * per_graph)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r18", "socp_time.json"))
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--per-graph", type=int, default=10)
    args = ap.parse_args()
    _lib.load()
    dev = engine.require_device("cuda:0")
    results = []
    for shifts in ([6.0], list(np.linspace(6.0, 15.0, 64))):
        r = time_batch(shifts, dev, args.frames, args.rounds, args.per_graph)
        results.append(r)
        d = r["device_round_us"]
        print(f"S = {r['scenes']}: status {r['status']}, rounds max {r['rounds_max']} mean "
              f"{r['rounds_mean']:.2f}; frame {r['frame_us_median']:.1f} us (min "
              f"{r['frame_us_min']:.1f}), {r['round_us']:.1f} us per round on the host clock; "
              f"device: QP alone {d['qp_a']:.2f} / {d['qp_b']:.2f} us, QP + cuts "
              f"{d['qp_cuts']:.2f} us (+{r['device_cuts_added_us']:.2f})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
