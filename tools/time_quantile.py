"""Time ccmpc_risk_quantile beside ccmpc_risk_audit (records only) and ccmpc_moments on the same
particle store.

    python tools/time_quantile.py [--out quantile_time.json] [--rounds 25] [--per-graph 10]
    CCMPC_LIB=cc-mpc_amd/csrc/build_noagg/libccmpc.so python tools/time_quantile.py --out ...
        (the same against a variant library, e.g. tools/build_variant.sh noagg
         "-DCCMPC_QUANTILE_AGG=0": per-lane LDS adds instead of the in-wave aggregation)
    rocprofv3 --kernel-trace --stats ... -- python tools/time_quantile.py --loop 100 --store "C4/8 f64"
        (no timing: eager calls of each series on one store, for a profiler run of its own)

Stores: tools/time_audit.py's -- C2 (4 OVs x 5 000, T = 8, f64) and the per-GPU C4 batch
(8 scenes x 4 OVs x 20 000, T = 12) as f64 and as f32.  On each store four series alternate in
one process -- moments, audit (the store's own Minkowski half-spaces, no plan), the calibration
of those half-spaces to risk.allow_counts, moments again -- every series a captured graph of
`per-graph` calls timed with device events, `rounds` replays each after a warm-up of every graph.
The two moments series give the spread a comparison has to clear.  A calibration call is 17
launches (initial values, then 8 x counting pass + narrowing) and is timed as the call; the
per-pass figure is (call - the first launch's share) / 8 only as far as the launches are alike,
so the kernel trace gives it.  Algorithmic bytes: 8 passes x 16 T' sum(N) (f64; 8 T' sum(N) f32),
T' the steps that carry calibrated records.

Without --store every store runs in a child process of its own under a time limit; the first
failure ends the run."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cc-mpc_amd")]

HBM_PEAK = 8e12
PASSES = 8
STORE_NAMES = ["C2", "C4/8 f64", "C4/8 f32"]
CHILD_LIMIT_S = 240


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
    quant = cyc.calibrate(allow)
    audit = engine.risk_audit(store, rec=cyc.rec, rec_kind=engine._lib.REC_KIND_HALFSPACE, R=cyc.R)
    torch.cuda.synchronize()
    return store, cyc, T, allow, quant, audit


def series_of(store, cyc, allow, quant, audit):
    import torch

    from ccmpc import engine
    mean, cov = torch.empty_like(cyc.mean), torch.empty_like(cyc.cov)
    kind = engine._lib.REC_KIND_HALFSPACE
    return {
        "moments_a": lambda: engine.moments(store, mean, cov, cyc.ws),
        "audit_rec": lambda: engine.risk_audit(store, rec=cyc.rec, rec_kind=kind, R=cyc.R,
                                               out=audit),
        "quantile": lambda: cyc.calibrate(allow, out=quant),
        "moments_b": lambda: engine.moments(store, mean, cov, cyc.ws),
    }


def time_store(name, dev, rounds, per_graph):
    import torch

    import time_audit
    from ccmpc import _lib
    store, cyc, T, allow, quant, audit = setup(name, dev)
    graphs = {k: time_audit.graph_of(f, per_graph, dev)
              for k, f in series_of(store, cyc, allow, quant, audit).items()}
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
    status = quant.status.cpu().numpy()
    h = cyc.records()
    t_rec = (h["t_tau"] >> 16)[:, :status.shape[1]]
    steps = sorted(set(t_rec[status == 0].tolist()))
    plane_bytes = (8 if store.dtype == torch.float32 else 16) * n
    res = dict(store=name, particles=n, cells=store.n_cells, T=T,
               records_per_cell=int(status.shape[1]), calibrated_records=int((status == 0).sum()),
               steps_with_calibrated_records=len(steps),
               dtype="f32" if store.dtype == torch.float32 else "f64",
               audit_algorithmic_bytes=plane_bytes * T,
               quantile_algorithmic_bytes=PASSES * plane_bytes * len(steps),
               library=os.path.relpath(_lib.LIB_PATH, ROOT),
               timed_calls_per_series=rounds * per_graph, series={})
    for k, v in times.items():
        v = np.asarray(v)
        res["series"][k] = dict(median_us=float(np.median(v)), min_us=float(v.min()),
                                max_us=float(v.max()))
    s = res["series"]
    q = s["quantile"]["median_us"]
    res["moments_spread_us"] = abs(s["moments_a"]["median_us"] - s["moments_b"]["median_us"])
    res["quantile_call_over_8_us"] = q / PASSES
    res["quantile_call_over_8_vs_audit_rec"] = q / PASSES / s["audit_rec"]["median_us"]
    res["quantile_fraction_of_8TBps"] = res["quantile_algorithmic_bytes"] / (q * 1e-6) / HBM_PEAK
    return res


def loop_store(name, dev, n):
    """n eager calls of each series on one store (kernel times come from the profiler)."""
    import torch
    store, cyc, T, allow, quant, audit = setup(name, dev)
    fns = series_of(store, cyc, allow, quant, audit)
    for _ in range(n):
        for k in ("moments_a", "audit_rec", "quantile"):
            fns[k]()
    torch.cuda.synchronize()
    print(f"{name}: {n} calls of moments, audit (records), quantile")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", type=int, default=0, help="profiler mode: eager calls, no timing")
    ap.add_argument("--store", default=None, choices=STORE_NAMES,
                    help="one store in this process (default: every store, a child each)")
    ap.add_argument("--out", default="quantile_time.json")
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--per-graph", type=int, default=10)
    args = ap.parse_args()
    if args.rounds * args.per_graph < 200:
        raise SystemExit("at least 200 timed calls per series")
    if args.store is None and not args.loop:
        results, device = [], None
        for name in STORE_NAMES:
            with tempfile.TemporaryDirectory() as d:
                part = os.path.join(d, "part.json")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--store", name,
                                "--out", part, "--rounds", str(args.rounds), "--per-graph",
                                str(args.per_graph)], check=True, timeout=CHILD_LIMIT_S)
                with open(part) as f:
                    got = json.load(f)
            device = got["device"]
            results += got["results"]
        with open(args.out, "w") as f:
            json.dump(dict(device=device, results=results), f, indent=1)
            f.write("\n")
        return
    import torch

    from ccmpc import _lib, engine
    _lib.load()
    dev = engine.require_device("cuda:0")
    name = args.store or "C4/8 f64"
    if args.loop:
        loop_store(name, dev, args.loop)
        return
    r = time_store(name, dev, args.rounds, args.per_graph)
    s = r["series"]
    print(f"{name}: moments {s['moments_a']['median_us']:.2f} / {s['moments_b']['median_us']:.2f}"
          f" us, audit (records) {s['audit_rec']['median_us']:.2f} us, quantile "
          f"{s['quantile']['median_us']:.2f} us = 8 x {r['quantile_call_over_8_us']:.2f} us "
          f"({r['quantile_call_over_8_vs_audit_rec']:.2f} of the audit; "
          f"{r['quantile_fraction_of_8TBps']:.2f} of 8 TB/s)", flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=[r]), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
