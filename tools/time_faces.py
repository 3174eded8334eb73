"""Time ccmpc_face_constraints beside ccmpc_moments on the same particle store.

    python tools/time_faces.py [--out faces_time.json] [--rounds 25] [--per-graph 10]

Stores: C2 (4 OVs x 5 000, T = 8, f64) and the per-GPU C4 batch (8 scenes x 4 OVs x 20 000,
T = 12) as f64 and as f32 (tools/time_audit.py's stores).  On each store five series alternate
in one process -- moments, faces nominal (with a reference trajectory: the approx choice too),
moments again, faces robust, faces nominal without a reference -- every series a captured graph
of `per-graph` calls timed with device events, `rounds` replays each after a warm-up of every
graph (rounds x per-graph >= 200 timed calls per series).  The two moments series give the
spread a comparison has to clear.  The bytes reported are the store planes once, 16 T sum(N)
(f64) or 8 T sum(N) (f32), the figure tools/time_audit.py reports (the (chunk, t) grid of
face_moments_kernel reads every plane but the last pair twice); the fraction is of the 8 TB/s
HBM peak.  A faces call is two launches (chunk moments, then one wave per (cell, t)) and is
timed as the call."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cc-mpc_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from ccmpc import _lib, engine  # noqa: E402
from time_audit import HBM_PEAK, STORES, build, graph_of  # noqa: E402


def time_store(name, dev, rounds, per_graph):
    store, cyc, T = build(name, dev)
    C = store.n_cells
    mean, cov = torch.empty_like(cyc.mean), torch.empty_like(cyc.cov)
    past = cyc.mean[:, 0, :].cpu().numpy() - np.array([3.0, 0.7])
    gamma = np.full(C, 2.7)
    ws = engine.Workspace(dev)
    rec = torch.empty((C, T, 4, 128), dtype=torch.uint8, device=dev)
    # the small inputs are uploaded once, outside the graphs: the calls below are the two
    # launches only
    first = engine.face_constraints(store, past, gamma, "nominal", ref_traj=cyc.ref,
                                    cell_ref=cyc.cell_ref, workspace=ws, out_rec=rec)
    small, ref, cell_ref, wbuf = first._keepalive
    pl, gm, ex = small[:2 * C], small[2 * C:3 * C], small[3 * C:]
    lib = _lib.load()
    p = engine._p

    def faces(kind, with_ref):
        def call():
            _lib.check(lib.ccmpc_face_constraints(
                p(store.pos), store.ccmpc_dtype, store.ld, T, p(store.origin), p(store.cell_off),
                p(store.cell_cnt), C, store.n_bound, p(pl), p(ex), p(gm),
                p(ref if with_ref else None), p(cell_ref if with_ref else None), kind, 4.47213,
                p(wbuf), wbuf.numel(), p(rec), engine._stream()), "ccmpc_face_constraints")
        return call

    series = {
        "moments_a": lambda: engine.moments(store, mean, cov, cyc.ws),
        "faces_nominal_ref": faces(_lib.FACE_NOMINAL, True),
        "moments_b": lambda: engine.moments(store, mean, cov, cyc.ws),
        "faces_robust": faces(_lib.FACE_ROBUST, False),
        "faces_nominal": faces(_lib.FACE_NOMINAL, False),
    }
    graphs = {k: graph_of(f, per_graph, dev) for k, f in series.items()}
    for g in graphs.values():
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    status = engine.face_records(rec)["status"]
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
    res = dict(store=name, particles=n, cells=C, T=T,
               dtype="f32" if store.dtype == torch.float32 else "f64", algorithmic_bytes=nbytes,
               timed_calls_per_series=rounds * per_graph, failed_records=int((status != 0).sum()),
               series={})
    for k, v in times.items():
        v = np.asarray(v)
        med = float(np.median(v))
        res["series"][k] = dict(median_us=med, min_us=float(v.min()), max_us=float(v.max()),
                                fraction_of_8TBps=nbytes / (med * 1e-6) / HBM_PEAK)
    a, b = res["series"]["moments_a"]["median_us"], res["series"]["moments_b"]["median_us"]
    res["moments_spread_us"] = abs(a - b)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="faces_time.json")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--per-graph", type=int, default=10)
    args = ap.parse_args()
    if args.rounds * args.per_graph < 200:
        raise SystemExit("at least 200 timed calls per series")
    _lib.load()
    dev = engine.require_device("cuda:0")
    results = []
    for name in STORES:
        r = time_store(name, dev, args.rounds, args.per_graph)
        results.append(r)
        s = r["series"]
        print(f"{name}: moments {s['moments_a']['median_us']:.2f} / "
              f"{s['moments_b']['median_us']:.2f} us, faces nominal + ref "
              f"{s['faces_nominal_ref']['median_us']:.2f} us "
              f"({s['faces_nominal_ref']['fraction_of_8TBps']:.2f} of 8 TB/s), robust "
              f"{s['faces_robust']['median_us']:.2f} us, nominal "
              f"{s['faces_nominal']['median_us']:.2f} us; failed records "
              f"{r['failed_records']}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
