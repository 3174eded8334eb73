"""Time ccmpc_ideal_risk_quantile beside its parent and beside the materialised path, with the
candidate list on and off.

    python tools/time_ideal_quantile.py [--out profiles/r27/ideal_quantile_time.json]
        [--lib-nolist PATH] [--rounds 25] [--per-graph 10]
    python tools/time_ideal_quantile.py --trace        (under rocprofv3 --kernel-trace --stats)

Shapes: 2 and 9 cells x 1e6 samples at T = 7, source moments of T_src = 8, the cycle's own 21
half-space records per cell, allow from risk.allow_counts.  On each shape the series alternate in
one process, every series a captured graph of `per-graph` calls timed with device events,
`rounds` replays each after a warm-up of every graph:
  moments_a / moments_b   ccmpc_ideal_moments, twice: the parent (one generation of the samples,
                          with the Gram); its two readings give the spread
  materialised            ccmpc_ideal_rollout + ccmpc_risk_quantile on the store
  fused_nolist            ccmpc_ideal_risk_quantile of the library at --lib-nolist, a build with
                          CCMPC_IDEAL_QUANT_LIST=0 (make OBJDIR=... OUT=...
                          EXTRA=-DCCMPC_IDEAL_QUANT_LIST=0); left out without the option
  fused                   ccmpc_ideal_risk_quantile of the package's library
The outputs of the three calibrations are compared equal before anything is timed.  The
statement under test, reported either way: the list stays if `fused` beats `fused_nolist` by
more than three times the spread (max - min) of fused_nolist's series on both shapes.  No bar is
set between fused and materialised: the fused call's purpose is the store it does not need, so
its workspace bytes are reported beside the store's.

--trace runs, eagerly on the first shape, three ccmpc_ideal_risk_audit calls (records only) and
three ccmpc_ideal_risk_quantile calls and exits: the kernel trace then holds the per-pass times
beside ideal_audit_kernel on the same shape."""
import argparse
import ctypes
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
NAMES = ("ccmpc_ideal_risk_quantile_workspace_bytes", "ccmpc_ideal_risk_quantile")


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
    """Source moments of a small random-walk store and the frame's own records."""
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
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * C
    P = T * (T - 1) // 2
    rec = engine._rec_bytes(rec, _lib.REC_KIND_HALFSPACE, C)[:, :P].contiguous()
    allow = torch.as_tensor(risk.allow_counts([n] * C, [C], T_SRC), device=dev)
    return pm, pc, src, rec, allow, ws


def other_library(path):
    """The two entry points of a second build of the library, bound as _lib binds them."""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in NAMES:
        res, args = _lib.SIGNATURES[name]
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


def same(a, b):
    return (torch.equal(a.q.view(torch.int64), b.q.view(torch.int64))
            and torch.equal(a.rhs.view(torch.int64), b.rhs.view(torch.int64))
            and torch.equal(a.status, b.status))


def time_shape(name, dev, rounds, per_graph, nolist):
    C, n, T = SHAPES[name]
    pm, pc, src, rec, allow, ws = build(C, n, T, dev)
    lib = _lib.load()
    p = engine._p
    kind, R, seed = _lib.REC_KIND_HALFSPACE, risk.R_COLLISION, 3
    mean, cov, st = engine.ideal_moments(pm, pc, src, T, n, seed=seed, workspace=ws)
    store, st_r = engine.ideal_rollout(pm, pc, src, T, n, seed=seed)
    out_m = engine.risk_quantile(store, rec, kind, allow=allow, R=R, T=T)
    out_f = engine.ideal_risk_quantile(pm, pc, src, T, n, rec, kind, allow=allow, R=R, seed=seed)
    torch.cuda.synchronize()
    assert same(out_m, out_f[0]), "fused != materialised"
    assert int((out_f[0].status == 0).sum()) > 0

    def moments():
        engine.ideal_moments(pm, pc, src, T, n, seed=seed, workspace=ws, out_mean=mean,
                             out_cov=cov, out_status=st)

    def materialised():       # the rollout into the store held above (nothing allocated)
        _lib.check(lib.ccmpc_ideal_rollout(p(pm), p(pc), T_SRC, p(src), C, T, n, None, None, seed,
                                           None, p(store.pos), store.ld, p(st_r),
                                           engine._stream()), "ccmpc_ideal_rollout")
        engine.risk_quantile(store, rec, kind, allow=allow, R=R, T=T, out=out_m)

    series = {
        "moments_a": moments,
        "materialised": materialised,
        "fused": lambda: engine.ideal_risk_quantile(pm, pc, src, T, n, rec, kind, allow=allow,
                                                    R=R, seed=seed, out=out_f),
        "moments_b": moments,
    }
    res = dict(shape=name, cells=C, samples=n, T=T, T_src=T_SRC,
               records_per_cell=int(rec.shape[1]), allow=allow.cpu().tolist(),
               materialised_store_bytes=16 * T * C * n,
               materialised_workspace_bytes=int(out_m.workspace.numel()),
               fused_workspace_bytes=int(out_f[0].workspace.numel()))
    if nolist is not None:
        need = int(nolist.ccmpc_ideal_risk_quantile_workspace_bytes(T, kind, C))
        out_n = engine.RiskQuantile(torch.empty_like(out_m.q), torch.empty_like(out_m.rhs),
                                    torch.empty_like(out_m.status),
                                    torch.empty(need, dtype=torch.uint8, device=dev))
        st_n = torch.empty_like(st_r)

        def fused_nolist():
            _lib.check(nolist.ccmpc_ideal_risk_quantile(
                p(pm), p(pc), T_SRC, p(src), C, T, n, None, seed, None, None, p(rec), kind, R,
                p(allow), p(out_n.workspace), need, p(out_n.q), p(out_n.rhs), p(out_n.status),
                p(st_n), engine._stream()), "ccmpc_ideal_risk_quantile (list off)")

        fused_nolist()
        torch.cuda.synchronize()
        assert same(out_m, out_n), "fused (list off) != materialised"
        series["fused_nolist"] = fused_nolist
        res["fused_nolist_workspace_bytes"] = need
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
    res.update(timed_calls_per_series=rounds * per_graph, series={})
    for k, v in times.items():
        v = np.asarray(v)
        res["series"][k] = dict(median_us=float(np.median(v)), min_us=float(v.min()),
                                max_us=float(v.max()))
    med = {k: v["median_us"] for k, v in res["series"].items()}
    res["moments_spread_us"] = abs(med["moments_a"] - med["moments_b"])
    res["fused_over_moments"] = med["fused"] / med["moments_a"]
    res["fused_minus_materialised_us"] = med["fused"] - med["materialised"]
    if nolist is not None:
        c = res["series"]["fused_nolist"]
        res["nolist_spread_us"] = c["max_us"] - c["min_us"]
        res["list_gain_us"] = med["fused_nolist"] - med["fused"]
        res["list_pays"] = bool(res["list_gain_us"] > 3 * res["nolist_spread_us"])
    return res


def trace(dev):
    C, n, T = next(iter(SHAPES.values()))
    pm, pc, src, rec, allow, _ = build(C, n, T, dev)
    kind, R = _lib.REC_KIND_HALFSPACE, risk.R_COLLISION
    for _ in range(3):
        engine.ideal_risk_audit(pm, pc, src, T, n, rec=rec, rec_kind=kind, R=R, seed=3)
        engine.ideal_risk_quantile(pm, pc, src, T, n, rec, kind, allow=allow, R=R, seed=3)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27",
                                                  "ideal_quantile_time.json"))
    ap.add_argument("--lib-nolist", default=None)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--per-graph", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    _lib.load()
    dev = engine.require_device("cuda:0")
    if args.trace:
        trace(dev)
        return
    nolist = other_library(args.lib_nolist) if args.lib_nolist else None
    results = []
    for name in SHAPES:
        r = time_shape(name, dev, args.rounds, args.per_graph, nolist)
        results.append(r)
        print(name + ": " + ", ".join(
            f"{k} {v['median_us']:.1f} [{v['min_us']:.1f}, {v['max_us']:.1f}]"
            for k, v in r["series"].items()) + " us per call; workspace "
            f"{r['fused_workspace_bytes']} B against a store of {r['materialised_store_bytes']} B"
            + (f"; the list {'pays' if r['list_pays'] else 'does NOT pay'}: gain "
               f"{r['list_gain_us']:.1f} us against 3 x {r['nolist_spread_us']:.1f} us"
               if nolist is not None else ""), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
