"""Bit-for-bit comparison of two libccmpc.so builds on the cycle's outputs (GPU box, repo root):

    python tools/bits_compare.py build_r0 main      ("main" = the in-tree library)
    python tools/bits_compare.py qp build_r0 main   (the planning QP's outputs instead)

Each build runs in a child process that dumps every configuration's mean, covariance,
half-space records and lower probabilities (one-launch cycle, plus the moments-only launch) to
gpurun_out/bits_<build>.npz; the parent then compares the two dumps byte for byte.  Used to
show that a change to the reduction's shape (tree levels, gathers) keeps the same bits.

The qp mode dumps out_u, out_x, out_cost, out_status and out_iter of ccmpc_mpc_qp for
T in QP_T, full and compact records, 1 scene and 8, the methods ipm and gi and gi with
CCMPC_QP_GI_MAX_STEPS=0 (every scene that needs an active-set change handed to the IPM), one
T = 8 batch whose rows go to the workspace and one fused-LTV solve.
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, O, N, T, scenes, store dtype): the C3 sweep (one cell per OV, up to 2-level trees),
# C2, Scheme4 cells (T = 9, 10: a Gram narrower than the workgroup; T = 12), the C4 batch and
# C5 (deferred root at T = 40)
CONFIGS = [("C2", 4, 5000, 8, 1, "f32"), ("C3-1e3", 1, 1000, 8, 1, "f32"),
           ("C3-2e4", 1, 20000, 8, 1, "f32"), ("C3-1e5", 1, 100000, 8, 1, "f32"),
           ("C3-2e5", 1, 200000, 8, 1, "f32"), ("C3-1e5-f64", 1, 100000, 8, 1, "f64"),
           ("T9-C2", 4, 5000, 9, 1, "f32"), ("T10-1e5", 1, 100000, 10, 1, "f32"),
           ("T12-1e5", 1, 100000, 12, 1, "f32"), ("T20-1e5", 1, 100000, 20, 1, "f32"),
           ("C4/8", 4, 20000, 12, 8, "f32"), ("C4/8-f64", 4, 20000, 12, 8, "f64"),
           ("C5", 8, 50000, 40, 1, "f32")]


def dump(out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "cc-mpc_amd")]
    import torch
    from ccmpc import cycle, engine, synthetic
    dev = torch.device("cuda", 0)
    res = {}
    for name, O, N, T, scenes, dt in CONFIGS:
        cells, K, refs = [], [], []
        for sc in range(scenes):
            ovs, ref, _ = synthetic.scene(20251015 + 1000 + sc, O=O, N=N, T=T)
            cells += [c for o in ovs for c in o]
            K.append([len(o) for o in ovs])
            refs.append(ref)
        store = engine.ParticleStore.from_cells(
            cells, device=dev, dtype=torch.float64 if dt == "f64" else torch.float32)
        cyc = cycle.MinkowskiCycle(store, [k for ks in K for k in ks], np.array(refs),
                                   scene_K=K)
        cyc.run()
        torch.cuda.synchronize()
        for k, v in (("mean", cyc.mean), ("cov", cyc.cov), ("rec", cyc.rec),
                     ("prob_lower", cyc.prob_lower)):
            res[f"{name}/{k}"] = v.cpu().numpy().copy()
        engine.moments(store, cyc.mean, cyc.cov, cyc.ws)
        torch.cuda.synchronize()
        res[f"{name}/mom_cov"] = cyc.cov.cpu().numpy().copy()
        print(f"{name}: {int(sum(store.counts))} particles, {store.n_cells} cells", flush=True)
        del store, cyc
        torch.cuda.empty_cache()
    np.savez(out, **res)


QP_T = (5, 8, 12, 16, 24, 40)
QP_RUNS = (("ipm", None), ("gi", None), ("gi", "0"))       # (CCMPC_QP_METHOD, _GI_MAX_STEPS)


def dump_qp(out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "cc-mpc_amd")]
    import torch
    from ccmpc import _lib, cycle, dist, engine, mpc, synthetic
    dev = torch.device("cuda", 0)
    res = {}

    def solve(name, cps, T, kind, inputs, ltv=None, max_cells=None):
        for method, steps in QP_RUNS:
            os.environ["CCMPC_QP_METHOD"] = method
            os.environ.pop("CCMPC_QP_GI_MAX_STEPS", None)
            if steps is not None:
                os.environ["CCMPC_QP_GI_MAX_STEPS"] = steps
            qp = mpc.PlanningQP(cps, T, kind=kind, device=dev)
            if max_cells is not None:                       # a capacity, not a count
                qp.max_cells = max_cells
                need = _lib.load().ccmpc_mpc_qp_workspace_bytes(qp.S, T, max_cells, kind)
                assert need > 16, "rows still fit LDS"      # qp_plan(...).rows_lds is false
                qp.ws = torch.zeros(int(need), dtype=torch.uint8, device=dev)
            got = qp.solve(*inputs, ltv=ltv)
            torch.cuda.synchronize()
            for k, v in zip(("u", "x", "cost", "status", "iter"), got):
                res[f"{name}/{method}{'' if steps is None else '-steps' + steps}/{k}"] = \
                    v.cpu().numpy().copy()
        return res[f"{name}/gi/status"], res[f"{name}/gi/iter"]

    for T in QP_T:
        cells, K, cps, x0s, goals, refs = [], [], [], [], [], []
        for sc in range(8):
            c, k, ref, goal, x0, _ = synthetic.crossing_scene(20251015 + 5000 + sc, O=2, N=1000,
                                                              T=T)
            cells += c
            K += k
            cps.append(len(c))
            refs.append(ref)
            goals.append(goal)
            x0s.append(x0)
        store = engine.ParticleStore.from_cells(cells, device=dev)
        cyc = cycle.MinkowskiCycle(store, K, np.array(refs), scene_K=[[2, 2]] * 8)
        cyc.run()
        xbar, gamma = mpc.ltv(np.array(x0s), T, lon=3.7)
        goal_t = torch.as_tensor(np.array(goals), device=dev)
        ref_t = torch.as_tensor(np.array(refs), device=dev)
        full = cyc.rec.contiguous()
        recs = ((mpc.REC_HALFSPACE, "full", full),
                (mpc.REC_HALFSPACE_COMPACT, "compact", dist.compact_records(full, 0)))
        for kind, kn, rec in recs:
            st, it = solve(f"T{T}/{kn}/8", cps, T, kind, (gamma, xbar, goal_t, ref_t, rec))
            # alone: the first scene that needs an active-set change (the hand-over's path)
            s = int(np.argmax((st != mpc.QP_OK) | (it > 0)))
            c0 = sum(cps[:s])
            solve(f"T{T}/{kn}/1", [cps[s]], T, kind,
                  (gamma[s:s + 1], xbar[s:s + 1], goal_t[s:s + 1], ref_t[s:s + 1],
                   rec[c0:c0 + cps[s]].contiguous()))
        if T == 8:
            solve("T8/full/8-rows-in-workspace", cps, T, mpc.REC_HALFSPACE,
                  (gamma, xbar, goal_t, ref_t, full), max_cells=80)
            x0_t = torch.as_tensor(np.array(x0s), device=dev)
            solve("T8/full/8-fused-ltv", cps, T, mpc.REC_HALFSPACE,
                  (torch.zeros_like(gamma), torch.zeros_like(xbar), goal_t, ref_t, full),
                  ltv=(x0_t, 0.5, 3.7))
        print(f"T = {T}: {len(res)} arrays so far", flush=True)
    np.savez(out, **res)


def main():
    if sys.argv[1] in ("--dump", "--dump-qp"):
        (dump if sys.argv[1] == "--dump" else dump_qp)(sys.argv[2])
        return
    qp = sys.argv[1] == "qp"
    if qp:
        del sys.argv[1]
    paths = []
    for v in sys.argv[1:3]:
        env = dict(os.environ)
        if v != "main":
            env["CCMPC_LIB"] = os.path.join(ROOT, "cc-mpc_amd", "csrc", v, "libccmpc.so")
        out = os.path.join(ROOT, "gpurun_out", f"bits_{v}.npz")
        if qp:
            out = out[:-4] + "_qp.npz"
        os.makedirs(os.path.dirname(out), exist_ok=True)
        print(f"== {v}", flush=True)
        subprocess.run([sys.executable, __file__, "--dump-qp" if qp else "--dump", out],
                       env=env, check=True, timeout=600)
        paths.append(out)
    a, b = np.load(paths[0]), np.load(paths[1])
    bad = 0
    for k in a.files:
        same = a[k].tobytes() == b[k].tobytes()
        bad += not same
        if not same:
            x, y = a[k], b[k]
            if k.endswith("/rec"):             # half-space records: decisions exact?  d, Q rel
                sys.path[:0] = [os.path.join(ROOT, "cc-mpc_amd")]
                from ccmpc import _lib
                x = x.reshape(-1, 128).view(_lib.HALFSPACE_DTYPE).reshape(-1)
                y = y.reshape(-1, 128).view(_lib.HALFSPACE_DTYPE).reshape(-1)
                dec = all(np.array_equal(x[f], y[f]) for f in ("which", "side", "status"))
                rel = max(float(np.max(np.abs(x[f] - y[f]) / (np.abs(x[f]) + 1e-300)))
                          for f in ("d", "q00", "q11", "r00", "r11"))
                print(f"DIFF {k}: which/side/status identical: {dec}; max rel d/Q/QR {rel:.2e}")
            else:
                rel = float(np.max(np.abs(x - y)) / max(np.max(np.abs(x)), 1e-300))
                print(f"DIFF {k}: {np.count_nonzero(x != y)} of {x.size} elements differ, "
                      f"max |diff| / max |a| = {rel:.2e}")
    print(f"{len(a.files) - bad} of {len(a.files)} arrays bit-identical")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
