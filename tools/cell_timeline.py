"""Per-cell timeline of the headline cycle launch (bench.py's scene: seed 20251015, 4 OVs x 5000
particles, T = 8) from the phase stamps of a PROBE=20 build (4: stamps, 16: slot 7 = the root
gather's end, slot 2 = the arrival's drain and barrier done, just before the ticket's add):

    tools/build_variant.sh ts20 "-DCCMPC_PROBE=20"
    CCMPC_LIB=cc-mpc_amd/csrc/build_ts20/libccmpc.so python tools/cell_timeline.py [REPS]

For every cell: its items, when the last item's slab was published, when its last arriver had
drained its stores and passed the barrier (drained), when it left the tree with the add's answer
(ticket), the gather's end, the finaliser's end and the half-space tail's end -- all in
us from the launch's first stamp, the median over REPS launches (each the last of 5 back to
back) -- and which cell ended the launch how often.  (A one-item cell takes no ticket: its
"drained" column is the end of its stream and its drain / add columns mean nothing.)
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cc-mpc_amd")]

import torch  # noqa: E402

from ccmpc import _lib, cycle, engine, synthetic  # noqa: E402

ITEM, WHOLE = 256, 1024


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lib.ccmpc_probe_timestamps.restype = ctypes.c_int
    lib.ccmpc_probe_timestamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
    ovs, ref, _ = synthetic.scene(20251015, O=4, N=5000, T=8)
    store = engine.ParticleStore.from_cells([c for o in ovs for c in o], device=dev)
    cyc = cycle.MinkowskiCycle(store, [len(o) for o in ovs], ref).bind()
    items = [1 if n <= WHOLE else -(-n // ITEM) for n in store.counts]
    first = np.concatenate(([0], np.cumsum(items)))
    slot_items = getattr(store, "slot_cap", 0) // ITEM   # slotted: cell c's items start at c * this
    n_wg = store.n_cells * slot_items if slot_items else first[-1]
    rows, enders, spans = [], [], []
    for _ in range(reps):
        for _ in range(3):
            cyc.launch()
        torch.cuda.synchronize()
        assert lib.ccmpc_probe_timestamps(None, 1) == 0
        for _ in range(5):
            cyc.launch()
        torch.cuda.synchronize()
        buf = np.zeros(8192 * 8, np.uint64)
        assert lib.ccmpc_probe_timestamps(buf.ctypes.data_as(ctypes.c_void_p), 0) == 0
        ts = buf.reshape(8192, 8).astype(np.int64)[:n_wg]
        rel = (ts - ts[:, 0].min()) / 100.0
        row = []
        for c in range(store.n_cells):
            r = (rel[c * slot_items:c * slot_items + items[c]] if slot_items
                 else rel[first[c]:first[c + 1]])
            last = int(np.argmax(r[:, 6]))           # the finaliser: the only one with a tail stamp
            row.append((r[:, 0].max(), r[:, 3].max(), r[last, 2], r[last, 4], r[last, 7],
                        r[last, 5], r[last, 6], r[last, 3]))
        rows.append(row)
        ends = [x[6] for x in row]
        enders.append(int(np.argmax(ends)))
        spans.append(max(ends))
    arr = np.array(rows)
    med = np.median(arr, axis=0)
    # of the cell's last arriver, per launch: its own publish -> drained, drained -> ticket
    drain = np.median(arr[:, :, 2] - arr[:, :, 7], axis=0)
    add = np.median(arr[:, :, 3] - arr[:, :, 2], axis=0)
    print(f"{reps} launches, span median {np.median(spans):.2f} us "
          f"(min {min(spans):.2f}, max {max(spans):.2f}); stamps cost time: compare spans "
          f"between probe builds only")
    print("cell particles items | last start  last publish  drained  ticket  gather end  "
          "finalise end  tail end | drain  add | ends launch")
    for c in range(store.n_cells):
        m = med[c]
        print(f"{c:4d} {store.counts[c]:9d} {items[c]:5d} | {m[0]:10.2f} {m[1]:13.2f} {m[2]:8.2f} "
              f"{m[3]:7.2f} {m[4]:11.2f} {m[5]:13.2f} {m[6]:9.2f} | {drain[c]:5.2f} {add[c]:4.2f} | "
              f"{enders.count(c):3d} / {reps}")
    d = med[:, 1:7] - med[:, :6]
    print("median phase lengths over cells (us): publish->ticket %.2f (the last arriver's own "
          "drain + barrier %.2f, its add's round trip %.2f), gather %.2f, finalise %.2f, tail %.2f"
          % (np.median(med[:, 3] - med[:, 1]), np.median(drain), np.median(add),
             *np.median(d[:, 3:], axis=0)))


if __name__ == "__main__":
    main()
