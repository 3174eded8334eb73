"""Device-side building blocks over the C ABI: particle stores, moments, half-space kernels.

PyTorch is used only for device memory, streams and graphs; every numeric step is a HIP kernel
in libccmpc.so.  All functions enqueue on torch's current stream and never synchronise, so a
whole constraint-generation cycle can be captured into a hipGraph (torch.cuda.CUDAGraph).
"""
import collections
import ctypes
import os

import numpy as np
import torch

from . import _lib, risk

F64, F32 = _lib.CCMPC_F64, _lib.CCMPC_F32


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device_index=None):
    """torch's current stream on the current (or given) device as a raw handle.  The raw
    getter skips building a torch.cuda.Stream object (~2 us of host time per call, and the
    planning step makes several)."""
    if _raw_stream is not None:
        idx = torch.cuda.current_device() if device_index is None else device_index
        return ctypes.c_void_p(_raw_stream(idx))
    s = torch.cuda.current_stream() if device_index is None else torch.cuda.current_stream(
        device_index)
    return ctypes.c_void_p(s.cuda_stream)


def require_device(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.CcmpcError("ccmpc runs on the GPU only (no CPU fallback); got device "
                              f"{device}")
    if not torch.cuda.is_available():
        raise _lib.CcmpcError("no HIP device visible: the ccmpc path needs an MI355X")
    _lib.load()
    return device


def _round4(x):
    return (int(x) + 3) // 4 * 4


# Cell offsets and ld of the stores built here, in particles: a multiple of 4 is what the
# kernels need (16-byte vector loads); 32 puts every load group of a cell on whole 128-byte
# lines (a 16-particle f64 step, a 32-particle Scheme4 / f32 step), so the waves that stream
# neighbouring groups never share a line.  Measured against 4 (profiles/r03/ab3_store_align32.log):
# C5 85.9 -> 81.1 us cold, the per-GPU C4 batch 37.4 -> 36.0 us cold, C2 / C3 unchanged.
# CCMPC_STORE_ALIGN overrides it (A/B).
STORE_ALIGN = int(os.environ.get("CCMPC_STORE_ALIGN", "32"))


def _round_to(x, a):
    return (int(x) + a - 1) // a * a


# The slotted layout (ParticleStore.slot_cap > 0): every cell owns slot_cap columns, so a cell's
# start is c * slot_cap and the cycle kernel's short-horizon instances form their first particle
# addresses from the workgroup index alone (moments.hip, SLOT).  SLOT_CHUNK is the largest item
# the non-balanced RB = 1 path cuts (4 waves of 2^6 particles: CCMPC_LG_NW1 and the wave quota
# below the balanced-mode bound); a slot is a whole number of them, and the library checks that
# against the chunk it picks.  from_cells chooses the layout by itself only where the launch stays
# small and the slots are not mostly air (slot_rule).
SLOT_CHUNK = 256
SLOT_MAX_CELLS = 64          # the straight locate's range: the launches the front was written for
SLOT_MAX_ITEMS = 256         # at most one workgroup per CU, dead ones included
SLOT_MAX_T = 8               # the RB = 1 path
SLOT_MAX_BOUND = 1 << 18     # above it the launch is in balanced mode
SLOT_MIN_FILL = 0.4          # total / (n_cells * slot_cap): see slot_rule


def _lcm(a, b):
    import math
    return a * b // math.gcd(a, b)


def slot_capacity(counts, align=None):
    """The smallest slot that holds every cell: max(count) rounded up to the store alignment and
    to SLOT_CHUNK, at least one chunk."""
    al = STORE_ALIGN if align is None else int(align)
    unit = _lcm(al, SLOT_CHUNK)
    return max(_round_to(max([int(c) for c in counts] + [0]), unit), unit)


def slot_rule(counts, T, n_bound, align=None):
    """The slot capacity from_cells picks by itself, or 0 for the packed layout.  Slots where the
    launch has at most SLOT_MAX_CELLS cells and SLOT_MAX_ITEMS workgroups (one per CU, so that
    the workgroups without particles cost no second round), takes the RB = 1 path and is not in
    balanced mode -- and where the cells fill at least SLOT_MIN_FILL of their slots: a slotted
    store is n_cells * slot_cap wide whatever the cells hold, every copy of it and every row
    stride grows with that, and every chunk of a slot past its cell's last is a workgroup
    launched to exit.  C2, the sparsest store measured (nine cells of 600 .. 5000 in slots of
    5120: 0.43), is inside; below that nothing was measured, so such stores stay packed."""
    counts = [int(c) for c in counts]
    if not counts or len(counts) > SLOT_MAX_CELLS or T > SLOT_MAX_T or n_bound > SLOT_MAX_BOUND:
        return 0
    cap = slot_capacity(counts, align)
    if len(counts) * cap // SLOT_CHUNK > SLOT_MAX_ITEMS:
        return 0
    if sum(counts) < SLOT_MIN_FILL * len(counts) * cap:
        return 0
    return cap


def store_layout(counts, capacity=None, align=None, slot_cap=0):
    """(offsets, n_bound, ld) of a ParticleStore: host arithmetic only.  n_bound is the packed
    walk's end (or the capacity) in either layout."""
    counts = [int(c) for c in counts]
    al = STORE_ALIGN if align is None else int(align)
    if al < 4 or al % 4:
        raise ValueError("store alignment must be a multiple of 4 particles")
    offs, cur = [], 0
    for c in counts:
        offs.append(cur)
        cur = _round_to(cur + max(c, 0), al)
    n_bound = cur if capacity is None else max(cur, int(capacity))
    ld = max(_round_to(n_bound, al), al)
    slot_cap = int(slot_cap)
    if slot_cap:
        if slot_cap < 0 or slot_cap % al or slot_cap % SLOT_CHUNK:
            raise ValueError(f"slot_cap must be a positive multiple of {al} and {SLOT_CHUNK}")
        if counts and max(counts) > slot_cap:
            raise ValueError(f"a cell of {max(counts)} particles in slots of {slot_cap}")
        offs = [j * slot_cap for j in range(len(counts))]
        ld = max(ld, len(counts) * slot_cap)
    return offs, n_bound, ld


def cells_image(cells, offsets, ld, dtype=torch.float64, origin=None):
    """The host image [2T, ld] of a store holding `cells` at `offsets` (zero elsewhere)."""
    T = cells[0].shape[1]
    host = np.zeros((2 * T, ld), dtype=np.float64 if dtype == torch.float64 else np.float32)
    for j, c in enumerate(cells):
        c = np.asarray(c, dtype=np.float64)
        if origin is not None:
            c = c - np.asarray(origin, dtype=np.float64).reshape(-1, 2)[j]
        n = c.shape[0]
        o = offsets[j]
        host[:, o:o + n] = c.transpose(1, 2, 0).reshape(2 * T, n)
    return host


class ParticleStore:
    """Plane-major SoA particle clouds of several cells (see include/ccmpc.h).

    pos[(2t + c), off[j] + i] = coordinate c of particle i of cell j at step t.
    Cell offsets and ld are multiples of `align` particles (STORE_ALIGN = 32 by default; the
    kernels need a multiple of 4: 16-byte vector loads).
    F64 stores hold world coordinates; F32 stores hold coordinates relative to ``origin[j]``.

    slot_cap = 0: cells packed one behind the other.  slot_cap > 0: the slotted layout, every
    cell_off[j] == j * slot_cap, slot_cap a multiple of the alignment and of SLOT_CHUNK and at
    least max(counts), ld >= n_cells * slot_cap.  n_bound is the same in both (the particle total
    or capacity): it picks the kernels' item size, so both layouts cut the same items.
    """

    def __init__(self, T, counts, dtype=torch.float64, device="cuda", origin=None,
                 capacity=None, align=None, slot_cap=0):
        self.device = require_device(device)
        self.T = int(T)
        counts = [int(c) for c in counts]
        offs, self.n_bound, self.ld = store_layout(counts, capacity, align, slot_cap)
        self.slot_cap = int(slot_cap)
        self.dtype = dtype
        self.pos = torch.zeros((2 * self.T, self.ld), dtype=dtype, device=self.device)
        self.counts = counts
        self.cell_off = torch.tensor(offs, dtype=torch.int64, device=self.device)
        self.cell_cnt = torch.tensor(counts, dtype=torch.int64, device=self.device)
        self.offsets = offs
        if origin is None:
            self.origin = None
        else:
            self.origin = torch.as_tensor(np.asarray(origin, dtype=np.float64).reshape(-1, 2),
                                          device=self.device)

    @property
    def n_cells(self):
        return int(self.cell_cnt.shape[0])

    @property
    def ccmpc_dtype(self):
        return F64 if self.dtype == torch.float64 else F32

    @property
    def ws_bound(self):
        """The particle bound to size a moments workspace with: a slotted launch keeps one slab
        per chunk of every slot (ccmpc_cycle_args in include/ccmpc.h)."""
        return max(self.n_bound, self.n_cells * self.slot_cap)

    @classmethod
    def from_cells(cls, cells, device="cuda", dtype=torch.float64, origin=None, capacity=None,
                   slots=None):
        """cells: list of (N_j, T, 2) arrays (the reference's pred_positions[k] layout).
        For a float32 store, ``origin`` (n_cells, 2) is subtracted in float64 before the cast.
        ``capacity`` raises the particle bound the kernels are sized for (n_particles_bound).
        ``slots``: None picks the layout by slot_rule, True forces the slotted layout (at
        slot_capacity), False the packed one."""
        T = cells[0].shape[1]
        counts = [c.shape[0] for c in cells]
        if slots is None:
            cap = slot_rule(counts, T, store_layout(counts, capacity)[1])
        else:
            cap = slot_capacity(counts) if slots else 0
        store = cls(T, counts, dtype=dtype, device=device, origin=origin, capacity=capacity,
                    slot_cap=cap)
        store.pos.copy_(torch.from_numpy(cells_image(cells, store.offsets, store.ld, dtype,
                                                     origin)))
        return store

    def sync_counts(self):
        """Fetch device-side cell offsets/counts (after ccmpc_bucket); synchronises."""
        self.counts = [int(c) for c in self.cell_cnt.cpu().tolist()]
        self.offsets = [int(c) for c in self.cell_off.cpu().tolist()]
        return self.counts

    def cell_positions(self, j):
        """(N_j, T, 2) float64 host copy of one cell (world frame)."""
        if self.counts is None:
            self.sync_counts()
        n, o = self.counts[j], self.offsets[j]
        x = self.pos[:, o:o + n].double().cpu().numpy().reshape(self.T, 2, n).transpose(2, 0, 1)
        if self.origin is not None:
            x = x + self.origin[j].cpu().numpy()
        return x


class Workspace:
    """Grow-only device scratch buffer (pre-size it before graph capture).

    Allocated zero-filled: its head holds the per-cell arrival counters of the one-launch
    reductions, which must start at zero and which every call leaves at zero (ccmpc.h).
    One Workspace per stream."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.buf = torch.zeros(0, dtype=torch.uint8, device=self.device)

    def get(self, nbytes):
        nbytes = max(int(nbytes), 16)
        if self.buf.numel() < nbytes:
            self.buf = torch.zeros(nbytes + 4096, dtype=torch.uint8, device=self.device)
        return self.buf


def moments(store, out_mean=None, out_cov=None, workspace=None):
    """Per-cell mean [C, T, 2] and covariance [C, 2T, 2T] (ddof = 1) of a ParticleStore."""
    lib = _lib.load()
    C, T = store.n_cells, store.T
    if out_mean is None:
        out_mean = torch.empty((C, T, 2), dtype=torch.float64, device=store.device)
    if out_cov is None:
        out_cov = torch.empty((C, 2 * T, 2 * T), dtype=torch.float64, device=store.device)
    need = lib.ccmpc_moments_workspace_bytes(T, C, store.n_bound)
    ws = (workspace or Workspace(store.device)).get(need)
    _lib.check(lib.ccmpc_moments(_p(store.pos), store.ccmpc_dtype, store.ld, T, _p(store.origin),
                                 _p(store.cell_off), _p(store.cell_cnt), C, store.n_bound,
                                 _p(ws), ws.numel(), _p(out_mean), _p(out_cov), _stream()),
               "ccmpc_moments")
    return out_mean, out_cov


def minkowski(mean, cov, ref_traj, cell_risk, cell_ref=None, R=3.4, tol=1e-8, maxiter=1000,
              out_rec=None, out_prob_lower=None):
    """Half-space records [C, T(T-1)/2] (raw bytes, see records.halfspaces) + prob_lower [C, T]."""
    lib = _lib.load()
    C, T = mean.shape[0], mean.shape[1]
    P = T * (T - 1) // 2
    if out_rec is None:
        out_rec = torch.empty((C, max(P, 1), 128), dtype=torch.uint8, device=mean.device)
    if out_prob_lower is None:
        out_prob_lower = torch.empty((C, T), dtype=torch.float64, device=mean.device)
    _lib.check(lib.ccmpc_minkowski(_p(mean), _p(cov), T, C, _p(ref_traj), _p(cell_ref),
                                   _p(cell_risk), float(R), float(tol), int(maxiter),
                                   _p(out_rec), _p(out_prob_lower), _stream()),
               "ccmpc_minkowski")
    return out_rec, out_prob_lower


def minkowski_cycle(store, ref_traj, cell_risk, cell_ref=None, R=3.4, tol=1e-8, maxiter=1000,
                    workspace=None, out_mean=None, out_cov=None, out_rec=None,
                    out_prob_lower=None):
    """moments + Minkowski half-spaces in ONE launch (ccmpc_minkowski_cycle)."""
    lib = _lib.load()
    C, T = store.n_cells, store.T
    dev = store.device
    P = max(T * (T - 1) // 2, 1)
    out_mean = out_mean if out_mean is not None else torch.empty((C, T, 2), dtype=torch.float64,
                                                                 device=dev)
    out_cov = out_cov if out_cov is not None else torch.empty((C, 2 * T, 2 * T),
                                                              dtype=torch.float64, device=dev)
    out_rec = out_rec if out_rec is not None else torch.empty((C, P, 128), dtype=torch.uint8,
                                                              device=dev)
    out_prob_lower = (out_prob_lower if out_prob_lower is not None
                      else torch.empty((C, T), dtype=torch.float64, device=dev))
    need = lib.ccmpc_moments_workspace_bytes(T, C, store.n_bound)
    ws = (workspace or Workspace(dev)).get(need)
    _lib.check(lib.ccmpc_minkowski_cycle(
        _p(store.pos), store.ccmpc_dtype, store.ld, T, _p(store.origin), _p(store.cell_off),
        _p(store.cell_cnt), C, store.n_bound, _p(ws), ws.numel(), _p(ref_traj), _p(cell_ref),
        _p(cell_risk), float(R), float(tol), int(maxiter), _p(out_mean), _p(out_cov),
        _p(out_rec), _p(out_prob_lower), _stream()), "ccmpc_minkowski_cycle")
    return out_mean, out_cov, out_rec, out_prob_lower


def ideal_minkowski_cycle(prev_mean, prev_cov, src_cell, T, n_samples, ref_traj, cell_risk,
                          x0=None, seed=0, rng_cell=None, cell_ref=None, R=3.4, tol=1e-8,
                          maxiter=1000, workspace=None):
    """Shrinking-horizon step in one launch: predict_ideal -> moments -> half-spaces."""
    lib = _lib.load()
    C = src_cell.shape[0]
    T_src = prev_mean.shape[1]
    dev = prev_mean.device
    P = max(T * (T - 1) // 2, 1)
    out_mean = torch.empty((C, T, 2), dtype=torch.float64, device=dev)
    out_cov = torch.empty((C, 2 * T, 2 * T), dtype=torch.float64, device=dev)
    status = torch.empty(C, dtype=torch.int32, device=dev)
    rec = torch.empty((C, P, 128), dtype=torch.uint8, device=dev)
    pl = torch.empty((C, T), dtype=torch.float64, device=dev)
    need = lib.ccmpc_ideal_moments_workspace_bytes(T, C, n_samples)
    ws = (workspace or Workspace(dev)).get(need)
    _lib.check(lib.ccmpc_ideal_minkowski_cycle(
        _p(prev_mean), _p(prev_cov), T_src, _p(src_cell), C, T, n_samples, _p(x0),
        int(seed) & (2**64 - 1), _p(rng_cell), _p(ws), ws.numel(), _p(ref_traj), _p(cell_ref),
        _p(cell_risk), float(R), float(tol), int(maxiter), _p(out_mean), _p(out_cov), _p(status),
        _p(rec), _p(pl), _stream()), "ccmpc_ideal_minkowski_cycle")
    return out_mean, out_cov, status, rec, pl


# L4 in one workgroup per (cell, t) (ccmpc_l4, one launch) while the average cell holds at most
# this many particles; the split form (ccmpc_l4_split, two launches) above it.  The two sum the
# headings in different orders (same result to rounding), so the step graph and the eager calls
# choose by this one rule.
_L4_ONE_WG_MAX = int(os.environ.get("CCMPC_L4_ONE_WG_MAX", "8192"))


def l4_one_workgroup(n_cells, n_bound):
    return n_bound <= _L4_ONE_WG_MAX * max(int(n_cells), 1)


def l4(store, past_last, bbox, with_yaw=False, with_vertices=False, split=None,
       workspace=None):
    """Headings, L4 outer approximation and t=0 yaw stats per (cell, t): ccmpc_l4_split (every
    (cell, t) over several workgroups, two launches) or, split=False, ccmpc_l4 (one workgroup
    per (cell, t)); split=None chooses by l4_one_workgroup.  Returns dict(A [C,T,4,2], b [C,T,4],
    yaw_mean [C,T], yaw0_var [C], yaw?, vertices?)."""
    lib = _lib.load()
    C, T, dev = store.n_cells, store.T, store.device
    if split is None:
        split = not l4_one_workgroup(C, store.n_bound)
    out = dict(A=torch.empty((C, T, 4, 2), dtype=torch.float64, device=dev),
               b=torch.empty((C, T, 4), dtype=torch.float64, device=dev),
               yaw_mean=torch.empty((C, T), dtype=torch.float64, device=dev),
               yaw0_var=torch.empty((C,), dtype=torch.float64, device=dev))
    out["yaw"] = (torch.empty((T, store.ld), dtype=torch.float64, device=dev) if with_yaw
                  else None)
    out["vertices"] = (torch.empty((T * 8, store.ld), dtype=torch.float64, device=dev)
                       if with_vertices else None)
    # both small host inputs in one host-to-device copy
    pb = torch.as_tensor(np.stack([np.asarray(past_last, np.float64).reshape(C, 2),
                                   np.asarray(bbox, np.float64).reshape(C, 2)]), device=dev)
    past_last, bbox = pb[0], pb[1]
    if split:
        need = lib.ccmpc_l4_workspace_bytes(T, C, store.n_bound)
        ws = (workspace or Workspace(dev)).get(need)
        _lib.check(lib.ccmpc_l4_split(
            _p(store.pos), store.ccmpc_dtype, store.ld, T, _p(store.origin), _p(store.cell_off),
            _p(store.cell_cnt), C, store.n_bound, _p(past_last), _p(bbox), _p(ws), ws.numel(),
            _p(out["A"]), _p(out["b"]), _p(out["yaw_mean"]), _p(out["yaw0_var"]),
            _p(out["yaw"]), _p(out["vertices"]), _stream()), "ccmpc_l4_split")
        out["_keepalive"] = (past_last, bbox, ws)
        return out
    _lib.check(lib.ccmpc_l4(_p(store.pos), store.ccmpc_dtype, store.ld, T, _p(store.origin),
                            _p(store.cell_off), _p(store.cell_cnt), C, _p(past_last), _p(bbox),
                            _p(out["A"]), _p(out["b"]), _p(out["yaw_mean"]), _p(out["yaw0_var"]),
                            _p(out["yaw"]), _p(out["vertices"]), _stream()), "ccmpc_l4")
    out["_keepalive"] = (past_last, bbox)
    return out


def sample_unicycle(init_state, latent_pmf, gmm, N, T, dt=0.5, seed=0, device="cuda", ov_base=0,
                    z=None, eps=None, per_particle=False):
    """GMM-latent particle sampler (ccmpc_sample_unicycle_ex).

    init_state (O, 4); latent_pmf (O, L) p(z|x) (only used when z is drawn here; may be None
    when z is given).  gmm: per (OV, latent, step) parameters (O, L, T, 5), or with
    per_particle=True every sample's own parameters as p_y_xz's autoregressive decoder emits
    them, (O, N, T, 5) -- host array or device tensor; (O, T, 5, N) device layout is built here.
    z: injected latent ids (O, N) (torch's one-hot z argmax, prediction.py:103) or None for the
    Philox draw; eps: injected standard-normal noise (O, N, T, 2) float32 or None for Philox.
    ov_base = global id of the first OV (keys the Philox streams; see ccmpc.dist).
    Returns (z [O,N] int32, F32 ParticleStore in sample order: one cell per OV)."""
    lib = _lib.load()
    dev = require_device(device)
    O, L, t_init, t_cdf, t_gmm, layout, t_z, t_eps = _sampler_inputs(
        init_state, latent_pmf, gmm, N, T, dev, z, eps, per_particle)
    # the sampler writes OV o at o * round4(N): the kernel's own layout (align 4)
    store = ParticleStore(T, [N] * O, dtype=torch.float32, device=dev, origin=np.zeros((O, 2)),
                          align=4)
    out_z = torch.empty((O, N), dtype=torch.int32, device=dev)
    _lib.check(lib.ccmpc_sample_unicycle_ex(
        _p(t_init), _p(t_cdf), L, _p(t_gmm), layout, _p(t_z), _p(t_eps), O, N, T, float(dt),
        int(seed) & (2**64 - 1), None, int(ov_base), _p(out_z), _p(store.pos), store.ld,
        _stream()),
        "ccmpc_sample_unicycle_ex")
    store._keepalive = (t_init, t_cdf, t_gmm, t_z, t_eps)
    return out_z, store


def load_predictions(predictions, z, n_latent, rows=None, device="cuda"):
    """generate_vehicle_latents' predictions (nodes, N, T, 2) float32 scene-relative and z
    (nodes, N) int64 / int32 (prediction.py:93-105; host arrays or device tensors) -> the
    sample-order F32 store + int32 z that ccmpc_bucket reads (ccmpc_load_predictions), OV o
    = node rows[o] (default: every node).  Returns (z [O, N] int32, ParticleStore)."""
    lib = _lib.load()
    dev = require_device(device)
    pred = torch.as_tensor(predictions, device=dev)
    if pred.dtype != torch.float32 or pred.dim() != 4 or pred.shape[3] != 2:
        raise ValueError("predictions must be (nodes, N, T, 2) float32")
    pred = pred.contiguous()
    zt = torch.as_tensor(z, device=dev).contiguous()
    if zt.dtype not in (torch.int64, torch.int32) or tuple(zt.shape) != tuple(pred.shape[:2]):
        raise ValueError("z must be (nodes, N) int64 or int32")
    n_nodes, N, T = int(pred.shape[0]), int(pred.shape[1]), int(pred.shape[2])
    rows = list(range(n_nodes)) if rows is None else [int(r) for r in rows]
    if any(r < 0 or r >= n_nodes for r in rows):
        raise ValueError(f"rows outside [0, {n_nodes})")
    O = len(rows)
    t_rows = torch.as_tensor(np.asarray(rows, np.int32), device=dev)
    store = ParticleStore(T, [N] * O, dtype=torch.float32, device=dev, origin=np.zeros((O, 2)),
                          align=4)
    out_z = torch.empty((O, N), dtype=torch.int32, device=dev)
    stride = store.offsets[1] if O > 1 else N
    z_bad = torch.zeros(O, dtype=torch.int32, device=dev)
    _lib.check(lib.ccmpc_load_predictions(
        _p(pred), _p(zt), zt.element_size(), _p(t_rows), O, N, T, int(n_latent), _p(store.pos),
        store.ld, stride, _p(out_z), _p(z_bad), _stream()), "ccmpc_load_predictions")
    raise_bad_latents(z_bad.cpu().numpy(), n_latent)
    store._keepalive = (pred, zt, t_rows)
    return out_z, store


def raise_bad_latents(z_bad, n_latent):
    """IndexError where make_ovehicles' `veh_latent_predictions[zn[jdx]]` (v8ideal/__init__.py:
    488-491, a list of n_latent entries) raises it: z_bad[o] = OV o's ids outside
    [-n_latent, n_latent), counted on the device."""
    bad = [int(b) for b in np.asarray(z_bad).reshape(-1)]
    if any(bad):
        o = next(j for j, b in enumerate(bad) if b)
        raise IndexError(f"list index out of range: {bad[o]} latent id(s) of OV {o} outside "
                         f"[-{n_latent}, {n_latent}) (make_ovehicles' per-latent list)")


def _sampler_inputs(init_state, latent_pmf, gmm, N, T, dev, z, eps, per_particle):
    """Device copies of a sampler call's inputs (ccmpc_sample_unicycle_ex's layouts)."""
    init_state = np.asarray(init_state, np.float64).reshape(-1, 4)
    O = init_state.shape[0]
    t_z = t_eps = t_cdf = None
    if z is not None:
        t_z = torch.as_tensor(z, device=dev).to(torch.int32).reshape(O, N).contiguous()
    if latent_pmf is not None:
        pmf = np.asarray(latent_pmf, np.float64).reshape(O, -1)
        L = pmf.shape[1]
        t_cdf = torch.as_tensor(np.cumsum(pmf, axis=1), device=dev)
    elif t_z is not None:
        # the latent count: the per-latent table's, else any id below 64 (the kernel's bound)
        L = (int(gmm.shape[1]) if hasattr(gmm, "shape") else len(gmm[0])) if not per_particle else 64
    else:
        raise ValueError("latent_pmf is needed when z is drawn by the sampler")
    if t_z is not None and t_z.numel():
        lo, hi = int(t_z.min().item()), int(t_z.max().item())
        if lo < 0 or hi >= L:
            raise ValueError(f"injected z outside [0, {L}): [{lo}, {hi}]")
    if per_particle:
        if t_z is None:
            raise ValueError("per-particle GMM parameters need the injected z")
        g = torch.as_tensor(gmm, device=dev).to(torch.float32).reshape(O, N, T, 5)
        t_gmm = g.permute(0, 2, 3, 1).contiguous()           # (O, T, 5, N): particle-minor
        layout = _lib.GMM_PER_PARTICLE
    else:
        t_gmm = torch.as_tensor(np.ascontiguousarray(np.asarray(
            gmm.cpu() if torch.is_tensor(gmm) else gmm, np.float32).reshape(O, L, T, 5)),
            device=dev)
        layout = _lib.GMM_PER_LATENT
    if eps is not None:
        e = torch.as_tensor(eps, device=dev).to(torch.float32).reshape(O, N, T, 2)
        t_eps = e.permute(0, 2, 3, 1).contiguous()           # (O, T, 2, N)
    t_init = torch.as_tensor(init_state, device=dev)
    return O, L, t_init, t_cdf, t_gmm, layout, t_z, t_eps


def _bucket_plan(pmf, filter_pmf, max_k):
    """Kept modes of every OV (p(z|x) > filter, host data as in prediction.py:77-79): K per
    OV, max_k, keep_map [O, L] (kept index or -1), cell_base [O]."""
    O, L = pmf.shape
    keep = [np.argwhere(pmf[o] > filter_pmf).ravel() for o in range(O)]
    K = [int(k.size) for k in keep]
    if min(K) == 0:
        raise ValueError("attempt to get argmin of an empty sequence: an OV has no latent mode "
                         f"with p(z|x) > {filter_pmf} (ovehicle.py:96-97 fails the same way)")
    max_k = max(K) if max_k is None else max_k
    keep_map = -np.ones((O, L), np.int32)
    for o in range(O):
        keep_map[o, keep[o]] = np.arange(K[o], dtype=np.int32)
    cell_base = np.concatenate([[0], np.cumsum(K)[:-1]]).astype(np.int32)
    return K, max_k, keep_map, cell_base


FUSED_MAX_N = 1 << 18          # ccmpc_sample_bucket / ccmpc_bucket_predictions


def sample_bucket(init_state, latent_pmf, gmm, N, T, minpos, dt=0.5, seed=0, device="cuda",
                  ov_base=0, z=None, eps=None, per_particle=False, filter_pmf=0.1, max_k=None,
                  with_z=False, workspace=None):
    """Sampler + bucketing as one placement pass (ccmpc_sample_bucket, N <= 262144): the draws of
    sample_unicycle with the same arguments, bucketed as bucket() buckets them (each cell the
    same particles in the same order, the same pmf / init_center bits; only the cell offsets
    differ).  latent_pmf (O, L) is required (it decides the kept modes).

    Returns (bucketed F32 ParticleStore, K per OV, cell_pmf [n_cells] device, init_center
    [n_cells, 2] device), and the sample-order z [O, N] first when with_z.  workspace: an
    optional uint8 device tensor, zero-filled once by the caller and reused across calls."""
    lib = _lib.load()
    dev = require_device(device)
    if latent_pmf is None:
        raise ValueError("latent_pmf decides the kept modes: it is required")
    if not 1 <= int(N) <= FUSED_MAX_N:
        raise ValueError(f"sample_bucket takes N in [1, {FUSED_MAX_N}]: use sample_unicycle + "
                         "bucket beyond")
    O, L, t_init, t_cdf, t_gmm, layout, t_z, t_eps = _sampler_inputs(
        init_state, latent_pmf, gmm, N, T, dev, z, eps, per_particle)
    pmf = np.asarray(latent_pmf, np.float64).reshape(O, L)
    K, max_k, keep_map, cell_base = _bucket_plan(pmf, filter_pmf, max_k)
    region, cur, n_bound = [], 0, 0
    for o in range(O):
        region.append(cur)
        cur = _round4(cur + K[o] * (N + 4))          # room for every cell's worst case
        n_bound = _round4(n_bound + N + 4 * K[o])    # the particles themselves (+ alignment)
    n_cells = int(sum(K))
    origin = np.repeat(np.asarray(minpos, np.float64).reshape(-1, 2), K, axis=0)
    out = ParticleStore(T, [0] * n_cells, dtype=torch.float32, device=dev, origin=origin,
                        capacity=cur)
    out.counts = None                                   # device-side until sync_counts()
    out.n_bound = n_bound
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    t_keep, t_nk, t_base = t(keep_map), t(np.asarray(K, np.int32)), t(cell_base)
    t_min = t(np.asarray(minpos, np.float64).reshape(-1, 2))
    t_reg = t(np.asarray(region, np.int64))
    pmf_out = torch.empty(n_cells, dtype=torch.float64, device=dev)
    centre = torch.empty((n_cells, 2), dtype=torch.float64, device=dev)
    out_z = torch.empty((O, N), dtype=torch.int32, device=dev) if with_z else None
    need = lib.ccmpc_sample_bucket_workspace_bytes(O, N, T, max_k)
    if need == 0:
        raise ValueError("shape not supported by ccmpc_sample_bucket")
    ws = workspace if workspace is not None else torch.zeros(need, dtype=torch.uint8, device=dev)
    _lib.check(lib.ccmpc_sample_bucket(
        _p(t_init), _p(t_cdf), L, _p(t_gmm), layout, _p(t_z), _p(t_eps), O, N, T, float(dt),
        int(seed) & (2**64 - 1), None, int(ov_base), _p(t_keep), _p(t_nk), _p(t_base), max_k,
        _p(t_min), _p(t_reg), _p(ws), ws.numel(), _p(out_z), _p(out.pos), out.ld,
        _p(out.cell_off), _p(out.cell_cnt), _p(pmf_out), _p(centre), _stream()),
        "ccmpc_sample_bucket")
    out._keepalive = (t_init, t_cdf, t_gmm, t_z, t_eps, t_keep, t_nk, t_base, t_min, t_reg, ws)
    if with_z:
        return out_z, out, K, pmf_out, centre
    return out, K, pmf_out, centre


def bucket_predictions(predictions, z, latent_pmf, minpos, rows=None, filter_pmf=0.1,
                       max_k=None, device="cuda", workspace=None):
    """make_ovehicles on generate_vehicle_latents' predictions (nodes, N, T, 2) float32 and z
    (nodes, N) int64 / int32 (prediction.py:93-105; host arrays or device tensors) in one
    placement pass (ccmpc_bucket_predictions): the cells load_predictions + bucket give, bit
    for bit (only the cell offsets differ).  OV o = node rows[o] (default: every node);
    latent_pmf (O, L).  Raises IndexError where the reference's list index does (an id outside
    [-L, L)).  Returns (bucketed F32 ParticleStore, K per OV, cell_pmf, init_center)."""
    lib = _lib.load()
    dev = require_device(device)
    pred = torch.as_tensor(predictions, device=dev)
    if pred.dtype != torch.float32 or pred.dim() != 4 or pred.shape[3] != 2:
        raise ValueError("predictions must be (nodes, N, T, 2) float32")
    pred = pred.contiguous()
    zt = torch.as_tensor(z, device=dev).contiguous()
    if zt.dtype not in (torch.int64, torch.int32) or tuple(zt.shape) != tuple(pred.shape[:2]):
        raise ValueError("z must be (nodes, N) int64 or int32")
    n_nodes, N, T = int(pred.shape[0]), int(pred.shape[1]), int(pred.shape[2])
    rows = list(range(n_nodes)) if rows is None else [int(r) for r in rows]
    if any(r < 0 or r >= n_nodes for r in rows):
        raise ValueError(f"rows outside [0, {n_nodes})")
    pmf = np.asarray(latent_pmf, np.float64)
    O, L = pmf.shape
    if O != len(rows):
        raise ValueError(f"latent_pmf has {O} rows for {len(rows)} OVs")
    if not 1 <= N <= FUSED_MAX_N:
        raise ValueError(f"bucket_predictions takes N in [1, {FUSED_MAX_N}]: use "
                         "load_predictions + bucket beyond")
    K, max_k, keep_map, cell_base = _bucket_plan(pmf, filter_pmf, max_k)
    region, cur, n_bound = [], 0, 0
    for o in range(O):
        region.append(cur)
        cur = _round4(cur + K[o] * (N + 4))
        n_bound = _round4(n_bound + N + 4 * K[o])
    n_cells = int(sum(K))
    mp = np.asarray(minpos, np.float64).reshape(-1, 2)
    mp = np.tile(mp, (O, 1)) if mp.shape[0] == 1 else mp
    origin = np.repeat(mp, K, axis=0)
    out = ParticleStore(T, [0] * n_cells, dtype=torch.float32, device=dev, origin=origin,
                        capacity=cur)
    out.counts = None
    out.n_bound = n_bound
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    t_keep, t_nk, t_base = t(keep_map), t(np.asarray(K, np.int32)), t(cell_base)
    t_min, t_reg = t(mp), t(np.asarray(region, np.int64))
    t_rows = t(np.asarray(rows, np.int32))
    pmf_out = torch.empty(n_cells, dtype=torch.float64, device=dev)
    centre = torch.empty((n_cells, 2), dtype=torch.float64, device=dev)
    z_bad = torch.empty(O, dtype=torch.int32, device=dev)
    need = lib.ccmpc_sample_bucket_workspace_bytes(O, N, T, max_k)
    if need == 0:
        raise ValueError("shape not supported by ccmpc_bucket_predictions")
    ws = workspace if workspace is not None else torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.check(lib.ccmpc_bucket_predictions(
        _p(pred), _p(zt), zt.element_size(), _p(t_rows), O, N, T, L, _p(t_keep), _p(t_nk),
        _p(t_base), max_k, _p(t_min), _p(t_reg), _p(ws), ws.numel(), _p(out.pos), out.ld,
        _p(out.cell_off), _p(out.cell_cnt), _p(pmf_out), _p(centre), _p(z_bad), _stream()),
        "ccmpc_bucket_predictions")
    raise_bad_latents(z_bad.cpu().numpy(), L)
    out._keepalive = (pred, zt, t_rows, t_keep, t_nk, t_base, t_min, t_reg, ws)
    return out, K, pmf_out, centre


def affine(mean, cov, ref_traj, cell_gamma, cell_ref=None, R=3.4, out_rec=None):
    lib = _lib.load()
    C, T = mean.shape[0], mean.shape[1]
    if out_rec is None:
        out_rec = torch.empty((C, T, 128), dtype=torch.uint8, device=mean.device)
    _lib.check(lib.ccmpc_affine(_p(mean), _p(cov), T, C, _p(ref_traj), _p(cell_ref),
                                _p(cell_gamma), float(R), _p(out_rec), _stream()),
               "ccmpc_affine")
    return out_rec


TANGENT_CHOOSE = -2  # CCMPC_TANGENT_CHOOSE: the reference's const_idx = None


def affine_scale(mean, cov, ref_traj, cell_risk, tangent=None, const_idx=None, cell_ref=None,
                 R=3.4, out_rec=None, scaled=True):
    """GMM-affine half-spaces with the recursive-feasibility covariance scale
    (ccmpc_affine_scale; v8ideal/__init__.py:2074-2456).  tangent [C, T] float64 and
    const_idx [C, T] int32 carry the previous frame's slopes / tangent indices (T < ph);
    None -> slopes from ref_traj and the closest tangent (T == ph).  scaled=False is
    compute_obstacle_constraints_GMM_affine_robust (:1541-1878): scale = 1."""
    lib = _lib.load()
    C, T = mean.shape[0], mean.shape[1]
    dev = mean.device
    if out_rec is None:
        out_rec = torch.empty((C, T, 128), dtype=torch.uint8, device=dev)
    tg = ci = None
    if tangent is not None:
        tg = torch.as_tensor(np.asarray(tangent, np.float64).reshape(C, T), device=dev)
        ci = torch.as_tensor(np.asarray(const_idx, np.int32).reshape(C, T), device=dev)
    _lib.check(lib.ccmpc_affine_scale(_p(mean), _p(cov), T, C, _p(ref_traj), _p(cell_ref),
                                      _p(cell_risk), float(R), int(bool(scaled)), _p(tg),
                                      _p(ci), _p(out_rec),
                                      _stream()), "ccmpc_affine_scale")
    out_rec._keepalive = (tg, ci)
    return out_rec


def ideal_rollout(prev_mean, prev_cov, src_cell, T, n_samples, x0=None, Z=None, seed=0,
                  rng_cell=None):
    """Materialised predict_ideal trajectories as an F64 ParticleStore + per-cell status."""
    lib = _lib.load()
    C = src_cell.shape[0]
    T_src = prev_mean.shape[1]
    store = ParticleStore(T, [n_samples] * C, dtype=torch.float64, device=prev_mean.device, align=4,
                          capacity=C * n_samples)
    status = torch.empty(C, dtype=torch.int32, device=prev_mean.device)
    _lib.check(lib.ccmpc_ideal_rollout(_p(prev_mean), _p(prev_cov), T_src, _p(src_cell), C, T,
                                       n_samples, _p(x0), _p(Z), int(seed) & (2**64 - 1),
                                       _p(rng_cell), _p(store.pos), store.ld, _p(status),
                                       _stream()),
               "ccmpc_ideal_rollout")
    return store, status


def ideal_moments(prev_mean, prev_cov, src_cell, T, n_samples, x0=None, seed=0, rng_cell=None,
                  workspace=None, out_mean=None, out_cov=None, out_status=None):
    """predict_ideal fused with the moment reduction: mean [C,T,2], cov [C,2T,2T], status [C]."""
    lib = _lib.load()
    C = src_cell.shape[0]
    T_src = prev_mean.shape[1]
    dev = prev_mean.device
    if out_mean is None:
        out_mean = torch.empty((C, T, 2), dtype=torch.float64, device=dev)
    if out_cov is None:
        out_cov = torch.empty((C, 2 * T, 2 * T), dtype=torch.float64, device=dev)
    if out_status is None:
        out_status = torch.empty(C, dtype=torch.int32, device=dev)
    need = lib.ccmpc_ideal_moments_workspace_bytes(T, C, n_samples)
    ws = (workspace or Workspace(dev)).get(need)
    _lib.check(lib.ccmpc_ideal_moments(_p(prev_mean), _p(prev_cov), T_src, _p(src_cell), C, T,
                                       n_samples, _p(x0), int(seed) & (2**64 - 1), _p(rng_cell),
                                       _p(ws), ws.numel(), _p(out_mean), _p(out_cov),
                                       _p(out_status), _stream()),
               "ccmpc_ideal_moments")
    return out_mean, out_cov, out_status


def halfspaces(rec_bytes):
    """Device record bytes -> numpy structured array (HALFSPACE_DTYPE); synchronises."""
    return rec_bytes.cpu().numpy().reshape(-1).view(_lib.HALFSPACE_DTYPE).reshape(
        rec_bytes.shape[:-1])


def affine_records(rec_bytes):
    return rec_bytes.cpu().numpy().reshape(-1).view(_lib.AFFINE_DTYPE).reshape(
        rec_bytes.shape[:-1])


FACE_KINDS = {"nominal": _lib.FACE_NOMINAL, "robust": _lib.FACE_ROBUST}


def face_constraints(store, past_last, cell_gamma, kind="nominal", ref_traj=None, cell_ref=None,
                     extent=(3.7, 1.79), car_r=4.47213, workspace=None, out_rec=None):
    """Box-face chance-constraint records [C, T, 4] (raw bytes, see face_records) of a
    ParticleStore: ccmpc_face_constraints (v8ideal/__init__.py:966-1376).  kind "nominal"
    (root = sqrtm(C_f); with ref_traj [r, T, 2] it also marks the approx variant's face) or
    "robust" (root = sqrt(|C_f|_F) I).  extent = (lon, lat), the reference's truck_d.
    `workspace` must not be one the counter-bearing calls (moments, cycles, L4 split) share:
    this call overwrites its head, which they need zero."""
    lib = _lib.load()
    if kind not in FACE_KINDS:
        raise ValueError(f"kind must be one of {sorted(FACE_KINDS)}, got {kind!r}")
    C, T, dev = store.n_cells, store.T, store.device
    if out_rec is None:
        out_rec = torch.empty((C, T, 4, 128), dtype=torch.uint8, device=dev)
    # the small host inputs in one host-to-device copy: past_last [C, 2], gamma [C], extent [2]
    host = np.concatenate([np.asarray(past_last, np.float64).reshape(C * 2),
                           np.asarray(cell_gamma, np.float64).reshape(C),
                           np.asarray(extent, np.float64).reshape(2)])
    small = torch.as_tensor(host, device=dev)
    pl, gm, ex = small[:2 * C], small[2 * C:3 * C], small[3 * C:]
    if ref_traj is not None and not torch.is_tensor(ref_traj):
        ref_traj = torch.as_tensor(np.asarray(ref_traj, np.float64).reshape(-1, T, 2), device=dev)
    if cell_ref is not None and not torch.is_tensor(cell_ref):
        cell_ref = torch.as_tensor(np.asarray(cell_ref, np.int32).reshape(C), device=dev)
    need = lib.ccmpc_face_workspace_bytes(T, C, store.n_bound)
    ws = (workspace or Workspace(dev)).get(need)
    _lib.check(lib.ccmpc_face_constraints(
        _p(store.pos), store.ccmpc_dtype, store.ld, T, _p(store.origin), _p(store.cell_off),
        _p(store.cell_cnt), C, store.n_bound, _p(pl), _p(ex), _p(gm), _p(ref_traj), _p(cell_ref),
        FACE_KINDS[kind], float(car_r), _p(ws), ws.numel(), _p(out_rec), _stream()),
        "ccmpc_face_constraints")
    out_rec._keepalive = (small, ref_traj, cell_ref, ws)
    return out_rec


def face_records(rec):
    """Device (or host) face record bytes -> numpy structured array (FACE_DTYPE) of the same
    leading shape, with the packed word split into t / face / chosen; synchronises."""
    raw = rec.cpu().numpy() if torch.is_tensor(rec) else np.asarray(rec)
    r = raw.reshape(-1).view(_lib.FACE_DTYPE).reshape(raw.shape[:-1])
    out = np.empty(r.shape, dtype=np.dtype(_lib.FACE_DTYPE.descr[:-1] + [
        ("t", "<i4"), ("face", "<i4"), ("chosen", "<i4")]))
    for name in ("mean", "root", "C", "status"):
        out[name] = r[name]
    w = r["t_face_chosen"]
    out["t"] = w >> 16
    out["face"] = (w >> 8) & 0xff
    out["chosen"] = w & 0xff
    return out


def face_cuts(rec, T, scene_cell, n_cells, cell_gamma, plan, pool, pool_cell, out_g, out_viol,
              out_state, round, max_rounds, tol_g=1e-6, face_sel=None, car_r=4.47213,
              only_violated=False):
    """One round of outer-approximation cuts of the face rows (ccmpc_face_cuts): every selected
    (cell, t) row of `rec` [n_cells, T, 4, 128] linearised at `plan` [S, T, ld >= 2] (the QP's
    X [S, T, 4] is read in place) into region `round` of `pool` [(max_rounds + 1) n_cells, T, 32],
    which PlanningQP reads with kind REC_AFFINE_COMPACT and scene_cell = pool_cell.  scene_cell /
    pool_cell: int64 [S + 1] device tensors; face_sel: int32 [n_cells, T] or None (the records'
    own choice); out_g [n_cells, T], out_viol [S] float64 and out_state [S] int32 are written in
    full.  Every tensor is a contiguous device tensor; the sizes are checked here because the
    kernel reads raw pointers.  Enqueues one launch on the current stream, never synchronises."""
    lib = _lib.load()
    T, C, S = int(T), int(n_cells), int(scene_cell.numel()) - 1
    regions = int(max_rounds) + 1

    def need(t, name, dtype, numel):
        if (not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != dtype
                or not t.is_contiguous() or t.numel() < numel):
            raise ValueError(f"{name}: contiguous {dtype} device tensor of >= {numel} elements "
                             "required")
    if S < 0 or pool_cell.numel() != S + 1:
        raise ValueError("scene_cell and pool_cell must both hold S + 1 offsets")
    if plan.dim() != 3 or plan.shape[0] != S or plan.shape[1] != T or plan.shape[2] < 2:
        raise ValueError(f"plan must be [{S}, {T}, >= 2]")
    need(rec, "rec", torch.uint8, C * T * 4 * 128)
    need(scene_cell, "scene_cell", torch.int64, S + 1)
    need(pool_cell, "pool_cell", torch.int64, S + 1)
    need(cell_gamma, "cell_gamma", torch.float64, C)
    need(plan, "plan", torch.float64, 0)
    need(pool, "pool", torch.uint8, regions * C * T * 32)
    need(out_g, "out_g", torch.float64, C * T)
    need(out_viol, "out_viol", torch.float64, S)
    need(out_state, "out_state", torch.int32, S)
    if face_sel is not None:
        need(face_sel, "face_sel", torch.int32, C * T)
    _lib.check(lib.ccmpc_face_cuts(
        _p(rec), T, S, _p(scene_cell), _p(face_sel), _p(cell_gamma), float(car_r), _p(plan),
        int(plan.shape[2]), int(round), int(max_rounds), float(tol_g), int(bool(only_violated)),
        _p(pool), _p(pool_cell), _p(out_g), _p(out_viol), _p(out_state), _stream()),
        "ccmpc_face_cuts")
    return out_g, out_viol, out_state


RiskAudit = collections.namedtuple("RiskAudit", "hit hit_any min_d2 rec_open open")
RiskAudit.__doc__ = """risk_audit's device tensors: hit [C, T] int64, hit_any [C] int64, min_d2
[C, T] float64 (None without a plan); rec_open [C, P] int64, open [C, T] int64 (None without
records).  See ccmpc_risk_audit in include/ccmpc.h for what each counts."""


def _audit_rows(rec_kind, T):
    half = rec_kind in (_lib.REC_KIND_HALFSPACE, _lib.REC_KIND_HALFSPACE_COMPACT)
    return T * (T - 1) // 2 if half else T


def _audit_plan_arg(plan, cell_plan, C, T, dev):
    """risk_audit's checks of plan / cell_plan: (plan as a contiguous (n, T, 2) float64 device
    tensor, cell_plan as an int32 device tensor or None)."""
    t_plan = torch.as_tensor(plan, device=dev)
    if t_plan.dim() == 2:
        t_plan = t_plan.unsqueeze(0)
    if t_plan.dim() != 3 or t_plan.shape[1] < T or t_plan.shape[2] < 2:
        raise ValueError(f"plan must be (T, >= 2) or (n_plans, T, >= 2) with T >= {T}")
    if (t_plan.dtype != torch.float64 or tuple(t_plan.shape[1:]) != (T, 2)
            or not t_plan.is_contiguous()):
        t_plan = t_plan[:, :T, :2].to(torch.float64).contiguous()
    n_plans = int(t_plan.shape[0])
    if cell_plan is None:
        if n_plans != 1:
            raise ValueError(f"{n_plans} plans need cell_plan")
    elif torch.is_tensor(cell_plan):    # device-resident: its range is the caller's contract
        if (cell_plan.dtype != torch.int32 or tuple(cell_plan.shape) != (C,)
                or cell_plan.device != dev or not cell_plan.is_contiguous()):
            raise ValueError(f"cell_plan must be a contiguous int32 [{C}] tensor on {dev}")
    else:
        host = np.asarray(cell_plan, np.int64).reshape(-1)
        if host.shape[0] != C or (C and (host.min() < 0 or host.max() >= n_plans)):
            raise ValueError(f"cell_plan must hold {C} indices in [0, {n_plans})")
        cell_plan = torch.as_tensor(host.astype(np.int32), device=dev)
    return t_plan, cell_plan


def _audit_rec_arg(rec, rec_kind, C, T):
    """risk_audit's checks of rec / rec_kind: (rows per cell P, rec as contiguous (C, P, width)
    bytes)."""
    if rec_kind not in (_lib.REC_KIND_HALFSPACE, _lib.REC_KIND_AFFINE,
                        _lib.REC_KIND_HALFSPACE_COMPACT, _lib.REC_KIND_AFFINE_COMPACT):
        raise ValueError(f"unknown rec_kind {rec_kind!r}")
    P = _audit_rows(rec_kind, T)
    width = 32 if rec_kind >= _lib.REC_KIND_HALFSPACE_COMPACT else 128
    if rec.dtype != torch.uint8:
        rec = rec.view(torch.uint8)
    rec = rec.reshape(C, -1, width) if rec.dim() != 3 else rec
    if rec.shape[0] != C or rec.shape[2] != width or rec.shape[1] < P:
        raise ValueError(f"rec must be ({C}, >= {P}, {width}) bytes for rec_kind {rec_kind}")
    if P == 0:
        pass                        # T = 1 half-space kinds: no rows, only out_open
    elif rec.shape[1] != P:         # rows of a longer horizon's buffer
        rec = rec[:, :P].contiguous()
    elif not rec.is_contiguous():
        rec = rec.contiguous()
    return P, rec


def _audit_out(out, on_p, on_r, C, T, P, dev):
    """A fresh RiskAudit, or `out` with the shapes of its enabled halves checked."""
    if out is None:
        i64 = dict(dtype=torch.int64, device=dev)
        return RiskAudit(
            torch.empty((C, T), **i64) if on_p else None,
            torch.empty((C,), **i64) if on_p else None,
            torch.empty((C, T), dtype=torch.float64, device=dev) if on_p else None,
            torch.empty((C, P), **i64) if on_r else None,
            torch.empty((C, T), **i64) if on_r else None)
    want = dict(hit=(C, T), hit_any=(C,), min_d2=(C, T), rec_open=(C, P), open=(C, T))
    for name, shape in want.items():
        t = getattr(out, name)
        on = on_p if name in ("hit", "hit_any", "min_d2") else on_r
        if on and (t is None or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"out.{name} must be a contiguous {shape} tensor")
    return out


def ideal_risk_audit(prev_mean, prev_cov, src_cell, T, n_samples, plan=None, rec=None,
                     rec_kind=None, R=risk.R_COLLISION, cell_plan=None, x0=None, seed=0,
                     seed_dev=None, rng_cell=None, out=None):
    """risk_audit on the samples of the ideal rollout, which are never materialised
    (ccmpc_ideal_risk_audit): the outputs equal ideal_rollout(prev_mean, prev_cov, src_cell, T,
    n_samples, x0=x0, seed=seed, rng_cell=rng_cell) followed by risk_audit on that store, count
    for count and min_d2 bit for bit, at no HBM traffic for the samples.

    Rollout arguments as ideal_minkowski_cycle (src_cell / rng_cell int32 device tensors [C],
    x0 [C, 2] float64 or None); seed_dev: a uint64-sized device tensor that overrides seed, so
    a captured call audits a fresh seed per replay.  plan / cell_plan / rec / rec_kind / R / out
    as risk_audit, with n_samples particles in every cell.
    Returns (RiskAudit, status): status [C] int32 is the rollout's.  out: a previous call's
    (RiskAudit, status) pair, or a bare RiskAudit (the status is then not written and returned
    as None); nothing is allocated then, so the call can be captured.  Enqueues two launches on
    the current stream, never synchronises."""
    lib = _lib.load()
    dev = prev_mean.device
    C = int(src_cell.shape[0])
    T_src = int(prev_mean.shape[1])
    T, n_samples = int(T), int(n_samples)
    if plan is None and rec is None:
        raise ValueError("ideal_risk_audit needs a plan, records, or both")
    if not 1 <= T <= T_src - 1:
        raise ValueError(f"T = {T} outside [1, {T_src - 1}] (the source horizon less one)")
    t_plan = None
    if plan is not None:
        t_plan, cell_plan = _audit_plan_arg(plan, cell_plan, C, T, dev)
    else:
        cell_plan = None
    P = 0
    if rec is not None:
        P, rec = _audit_rec_arg(rec, rec_kind, C, T)
    status = None
    if out is None:
        status = torch.empty(C, dtype=torch.int32, device=dev)
    elif not isinstance(out, RiskAudit):
        out, status = out
        if (status.dtype != torch.int32 or tuple(status.shape) != (C,)
                or not status.is_contiguous()):
            raise ValueError(f"status must be a contiguous int32 [{C}] tensor")
    on_p, on_r = plan is not None, rec is not None
    out = _audit_out(out, on_p, on_r, C, T, P, dev)
    if C == 0:
        return out, status
    _lib.check(lib.ccmpc_ideal_risk_audit(
        _p(prev_mean), _p(prev_cov), T_src, _p(src_cell), C, T, n_samples, _p(x0),
        int(seed) & (2**64 - 1), _p(seed_dev), _p(rng_cell), _p(t_plan), _p(cell_plan),
        # no rows (T = 1 half-space kinds): any non-null address switches the record half on
        (_p(rec) if P else _p(prev_mean)) if on_r else None, int(rec_kind) if on_r else 0,
        float(R),
        _p(out.hit if on_p else None), _p(out.hit_any if on_p else None),
        _p(out.min_d2 if on_p else None), _p(out.rec_open if on_r else None),
        _p(out.open if on_r else None), _p(status), _stream()), "ccmpc_ideal_risk_audit")
    return out, status


def risk_audit(store, plan=None, rec=None, rec_kind=None, R=risk.R_COLLISION, cell_plan=None,
               T=None, out=None):
    """Monte-Carlo audit of a plan and / or constraint records on a ParticleStore
    (ccmpc_risk_audit): per cell, the particles the plan passes within R of, and the particles
    each record (and all records of a step together) leave unprotected.

    plan: device float64 tensor (T, >= 2) or (n_plans, T, >= 2) -- ego positions in the first
    two columns, e.g. the QP's X_star / out_x; cell_plan: each cell's plan row (None: row 0) as
    a host sequence (range-checked here) or an int32 device tensor [C] (read unchecked).
    rec: the (C, P, 128) uint8 records a cycle holds (rec_kind REC_KIND_HALFSPACE / _AFFINE) or
    their (C, P, 32) compact packing (the _COMPACT kinds).  T: the audited horizon (default
    store.T; fewer steps read only the first planes).
    out: a previous RiskAudit whose buffers are written again (nothing is allocated then, so the
    call can be captured).  A plan that is not already a contiguous (n, T, 2) float64 device
    tensor is copied first; a captured call that is to follow in-place updates of the plan must
    be given that form, so that the kernel reads the caller's tensor.
    Returns RiskAudit; enqueues two launches on the current stream, never synchronises."""
    lib = _lib.load()
    dev = store.device
    C = store.n_cells
    T = store.T if T is None else int(T)
    if not 1 <= T <= store.T:
        raise ValueError(f"T = {T} outside [1, {store.T}] (the store's horizon)")
    if plan is None and rec is None:
        raise ValueError("risk_audit needs a plan, records, or both")
    if getattr(store, "offsets", None) and any(int(o) % 4 for o in store.offsets):
        raise ValueError("cell offsets must be multiples of 4 particles")
    t_plan = None
    if plan is not None:
        t_plan, cell_plan = _audit_plan_arg(plan, cell_plan, C, T, dev)
    else:
        cell_plan = None
    P = 0
    if rec is not None:
        P, rec = _audit_rec_arg(rec, rec_kind, C, T)
    out = _audit_out(out, plan is not None, rec is not None, C, T, P, dev)
    on_p, on_r = plan is not None, rec is not None
    if C == 0:
        return out
    _lib.check(lib.ccmpc_risk_audit(
        _p(store.pos), store.ccmpc_dtype, store.ld, T, _p(store.origin), _p(store.cell_off),
        _p(store.cell_cnt), C, store.n_bound, _p(t_plan), _p(cell_plan),
        # no rows (T = 1 half-space kinds): any non-null address switches the record half on
        (_p(rec) if P else _p(store.pos)) if on_r else None, int(rec_kind) if on_r else 0,
        float(R),
        _p(out.hit if on_p else None), _p(out.hit_any if on_p else None),
        _p(out.min_d2 if on_p else None), _p(out.rec_open if on_r else None),
        _p(out.open if on_r else None), _stream()), "ccmpc_risk_audit")
    return out


def _face_plan_inputs(store, past_last, plan, cell_plan, extent, T, ld_plan):
    """The checked device inputs face_audit and face_quantile share (see face_audit):
    (T, past_last, extent, plan, ld_plan, cell_plan)."""
    dev = store.device
    C = store.n_cells
    T = store.T if T is None else int(T)
    if not 1 <= T <= store.T:
        raise ValueError(f"T = {T} outside [1, {store.T}] (the store's horizon)")
    if getattr(store, "offsets", None) and any(int(o) % 4 for o in store.offsets):
        raise ValueError("cell offsets must be multiples of 4 particles")
    f64 = dict(dtype=torch.float64, device=dev)

    def small(x, shape, name):
        if torch.is_tensor(x):
            if (x.dtype != torch.float64 or x.device != dev or not x.is_contiguous()
                    or x.numel() != int(np.prod(shape))):
                raise ValueError(f"{name} must be a contiguous float64 {shape} tensor on {dev}")
            return x
        return torch.as_tensor(np.ascontiguousarray(x, np.float64).reshape(shape), **f64)
    pl = small(past_last, (C, 2), "past_last")
    ex = small(extent, (2,), "extent")
    if torch.is_tensor(plan) and plan.device == dev:
        t_plan = plan
        if t_plan.dtype != torch.float64 or not t_plan.is_contiguous():
            raise ValueError("a device plan must be a contiguous float64 tensor")
        if ld_plan is None:
            if t_plan.dim() == 2:
                t_plan = t_plan.unsqueeze(0)
            if t_plan.dim() != 3 or t_plan.shape[1] != T or t_plan.shape[2] < 2:
                raise ValueError(f"plan must be ({T}, >= 2) or (n_plans, {T}, >= 2)")
            ld_plan = int(t_plan.shape[2])
        ld_plan = int(ld_plan)
        if ld_plan < 2 or t_plan.numel() % (T * ld_plan):
            raise ValueError(f"plan holds no whole number of [{T}, {ld_plan}] rows")
        n_plans = t_plan.numel() // (T * ld_plan)
    else:
        host = np.asarray(plan.cpu() if torch.is_tensor(plan) else plan, np.float64)
        if host.ndim == 2:
            host = host[None]
        if host.ndim != 3 or host.shape[1] < T or host.shape[2] < 2:
            raise ValueError(f"plan must be (T, >= 2) or (n_plans, T, >= 2) with T >= {T}")
        if ld_plan is not None and int(ld_plan) != 2:
            raise ValueError("ld_plan applies to a device plan; a host plan is copied as [n, T, 2]")
        t_plan = torch.as_tensor(np.ascontiguousarray(host[:, :T, :2]), **f64)
        ld_plan, n_plans = 2, int(host.shape[0])
    if cell_plan is None:
        if n_plans != 1:
            raise ValueError(f"{n_plans} plans need cell_plan")
    elif torch.is_tensor(cell_plan):        # device-resident: its range is the caller's contract
        if (cell_plan.dtype != torch.int32 or tuple(cell_plan.shape) != (C,)
                or cell_plan.device != dev or not cell_plan.is_contiguous()):
            raise ValueError(f"cell_plan must be a contiguous int32 [{C}] tensor on {dev}")
    else:
        host = np.asarray(cell_plan, np.int64).reshape(-1)
        if host.shape[0] != C or (C and (host.min() < 0 or host.max() >= n_plans)):
            raise ValueError(f"cell_plan must hold {C} indices in [0, {n_plans})")
        cell_plan = torch.as_tensor(host.astype(np.int32), device=dev)
    return T, pl, ex, t_plan, ld_plan, cell_plan


FaceAudit = collections.namedtuple(
    "FaceAudit", "face_open in_box in_box_any sel_open sel_open_any worst")
FaceAudit.__doc__ = """face_audit's device tensors: face_open [C, T, 4], in_box [C, T], in_box_any
[C] int64; sel_open [C, T], sel_open_any [C] int64 (None without face_sel); worst [C, T, 4]
float64 (None with worst=False).  See ccmpc_face_audit in include/ccmpc.h for what each counts."""


def face_audit(store, past_last, plan, face_sel=None, cell_plan=None, extent=(3.7, 1.79),
               car_r=4.47213, T=None, ld_plan=None, worst=True, out=None):
    """Monte-Carlo audit of the box-face rows on a ParticleStore (ccmpc_face_audit): per
    (cell, t) the particles each face's inequality leaves open at `plan`, those inside whose
    inflated box the plan lies, the count under the selected face and the largest violation.

    past_last [C, 2] and extent = (lon, lat) as face_constraints (host arrays, or contiguous
    float64 device tensors, which are read in place).  plan: ego positions in the first two
    columns -- a host array (T, >= 2) / (n_plans, T, >= 2), copied as [n, T, 2], or a contiguous
    float64 device tensor [n_plans, T, ld_plan >= 2] read in place (PlanningSOCP's X [S, T, 4]);
    ld_plan overrides the step stride of a flat device tensor.  cell_plan: each cell's plan row
    (None: row 0), a host sequence (range-checked here) or an int32 device tensor [C].
    face_sel [C, T]: 0..3 the face that is the row of (c, t), -1 no row; a host array
    (range-checked here: ValueError outside [-1, 3]) or a contiguous int32 device tensor; None
    skips the two sel outputs.  T: the audited horizon (default store.T).  worst=False skips the
    maxima.  out: a previous FaceAudit whose buffers are written again (with device-resident
    inputs nothing is allocated then, so the call can be captured).
    Returns FaceAudit; enqueues two launches on the current stream, never synchronises."""
    lib = _lib.load()
    dev = store.device
    C = store.n_cells
    T, pl, ex, t_plan, ld_plan, cell_plan = _face_plan_inputs(store, past_last, plan, cell_plan,
                                                              extent, T, ld_plan)
    if face_sel is not None:
        if torch.is_tensor(face_sel) and face_sel.device == dev:
            if (face_sel.dtype != torch.int32 or face_sel.numel() != C * T
                    or not face_sel.is_contiguous()):
                raise ValueError(f"face_sel must be a contiguous int32 [{C}, {T}] tensor")
        else:
            host = np.asarray(face_sel.cpu() if torch.is_tensor(face_sel) else face_sel, np.int64)
            if host.shape != (C, T):
                raise ValueError(f"face_sel must be ({C}, {T})")
            if host.size and (host.min() < -1 or host.max() > 3):
                raise ValueError("face_sel must be in [-1, 3]: a face 0..3, or -1 for no row")
            face_sel = torch.as_tensor(np.ascontiguousarray(host.astype(np.int32)), device=dev)
    on_s = face_sel is not None
    want = dict(face_open=((C, T, 4), torch.int64, True), in_box=((C, T), torch.int64, True),
                in_box_any=((C,), torch.int64, True), sel_open=((C, T), torch.int64, on_s),
                sel_open_any=((C,), torch.int64, on_s),
                worst=((C, T, 4), torch.float64, bool(worst)))
    if out is None:
        out = FaceAudit(*(torch.empty(shape, dtype=dt, device=dev) if on else None
                          for shape, dt, on in want.values()))
    else:
        for name, (shape, dt, on) in want.items():
            t = getattr(out, name)
            if on and (t is None or tuple(t.shape) != shape or t.dtype != dt
                       or not t.is_contiguous()):
                raise ValueError(f"out.{name} must be a contiguous {dt} {shape} tensor")
    if C == 0:
        return out
    _lib.check(lib.ccmpc_face_audit(
        _p(store.pos), store.ccmpc_dtype, store.ld, T, _p(store.origin), _p(store.cell_off),
        _p(store.cell_cnt), C, store.n_bound, _p(pl), _p(ex), float(car_r), _p(t_plan), ld_plan,
        _p(cell_plan), _p(face_sel), _p(out.face_open), _p(out.in_box), _p(out.in_box_any),
        _p(out.sel_open if on_s else None), _p(out.sel_open_any if on_s else None),
        _p(out.worst if worst else None), _stream()), "ccmpc_face_audit")
    out.face_open._keepalive = (pl, ex, t_plan, cell_plan, face_sel)
    return out


FaceQuantile = collections.namedtuple("FaceQuantile", "q arg cut status")
FaceQuantile.__doc__ = """face_quantile's device tensors: q [C, T, 4] float64 (the (m+1)-th largest
face value), arg [C, T, 4] int64 (the particle that attains it, -1 for none), cut [C, T, 4, 32]
uint8 (ccmpc_gather_rec: that particle's half-space shifted to the budget, or an empty record),
status [C, T] int32 (0, or _lib.CAL_VACUOUS / CAL_SKIPPED).  See ccmpc_face_quantile in
include/ccmpc.h."""

_face_quantile_ws = {}      # (device, stream) -> the call's workspace, grown on demand


def face_quantile(store, past_last, plan, allow=None, cell_plan=None, extent=(3.7, 1.79),
                  car_r=4.47213, margin=0.0, T=None, ld_plan=None, out=None, workspace=None):
    """Monte-Carlo calibration of the box-face rows on a ParticleStore (ccmpc_face_quantile):
    per (cell, t, face) the (allow[c] + 1)-th largest face value v_f of the cell's particles at
    `plan` -- the distance by which the row misses (> 0) or clears (<= 0) a budget of allow[c]
    open particles --, the particle that attains it, and that particle's own half-space shifted
    to the budget and by `margin`, as a record the planning QP reads.

    store, past_last, plan, cell_plan, extent, car_r, T and ld_plan as face_audit.  allow as
    risk_quantile: None (zeros), a host sequence (checked to be >= 0 here) or an int64 device
    tensor [C] (read unchecked; a negative entry marks the cell SKIPPED), e.g.
    risk.allow_counts.  margin >= 0.  out: a previous FaceQuantile whose buffers are written
    again.  workspace: a uint8 device tensor of ccmpc_face_quantile_workspace_bytes(T, C) bytes;
    None takes one cached per (device, stream), as PlanningQP keeps its own (with `out`, a given
    workspace and device-resident inputs nothing is allocated, so the call can be captured).
    Returns FaceQuantile; enqueues 19 launches on the current stream, never synchronises."""
    lib = _lib.load()
    dev = store.device
    C = store.n_cells
    T, pl, ex, t_plan, ld_plan, cell_plan = _face_plan_inputs(store, past_last, plan, cell_plan,
                                                              extent, T, ld_plan)
    margin = float(margin)
    if not (np.isfinite(margin) and margin >= 0.0):
        raise ValueError("margin must be finite and >= 0")
    if allow is None:
        pass
    elif torch.is_tensor(allow):
        if (allow.dtype != torch.int64 or tuple(allow.shape) != (C,) or allow.device != dev
                or not allow.is_contiguous()):
            raise ValueError(f"allow must be a contiguous int64 [{C}] tensor on {dev}")
    else:
        host = np.asarray(allow, np.int64).reshape(-1)
        if host.shape[0] != C or (C and host.min() < 0):
            raise ValueError(f"allow must hold {C} counts >= 0")
        allow = torch.as_tensor(host, device=dev)
    need = int(lib.ccmpc_face_quantile_workspace_bytes(T, C))
    if need == 0:
        raise ValueError(f"ccmpc_face_quantile rejects T = {T}, n_cells = {C}")
    want = dict(q=((C, T, 4), torch.float64), arg=((C, T, 4), torch.int64),
                cut=((C, T, 4, 32), torch.uint8), status=((C, T), torch.int32))
    if out is None:
        out = FaceQuantile(*(torch.empty(shape, dtype=dt, device=dev)
                             for shape, dt in want.values()))
    else:
        for name, (shape, dt) in want.items():
            t = getattr(out, name)
            if t is None or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"out.{name} must be a contiguous {dt} {shape} tensor")
    if workspace is None:
        stream = _stream()
        key = (dev, int(getattr(stream, "value", stream) or 0))
        workspace = _face_quantile_ws.get(key)
        if workspace is None or workspace.numel() < need:
            workspace = _face_quantile_ws[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    elif (workspace.dtype != torch.uint8 or workspace.device != dev
          or not workspace.is_contiguous() or workspace.numel() < need):
        raise ValueError(f"workspace must be a contiguous uint8 tensor of {need} bytes on {dev}")
    if C == 0:
        return out
    _lib.check(lib.ccmpc_face_quantile(
        _p(store.pos), store.ccmpc_dtype, store.ld, T, _p(store.origin), _p(store.cell_off),
        _p(store.cell_cnt), C, store.n_bound, _p(pl), _p(ex), float(car_r), _p(t_plan), ld_plan,
        _p(cell_plan), _p(allow), margin, _p(workspace), workspace.numel(), _p(out.q),
        _p(out.arg), _p(out.cut), _p(out.status), _stream()), "ccmpc_face_quantile")
    out.q._keepalive = (pl, ex, t_plan, cell_plan, allow, workspace)
    return out


def face_quantile_cuts(quant):
    """Host view of a FaceQuantile's cut records: a structured array [C, T, 4] of
    _lib.GATHER_DTYPE (n0, n1, rhs, side, status, t_tau)."""
    b = quant.cut.detach().cpu().numpy() if torch.is_tensor(quant.cut) else np.asarray(quant.cut)
    return np.ascontiguousarray(b).view(_lib.GATHER_DTYPE)[..., 0]


RiskQuantile = collections.namedtuple("RiskQuantile", "q rhs status workspace")
RiskQuantile.__doc__ = """risk_quantile's device tensors: q [C, P] float64 (the (m+1)-th largest
projection), rhs [C, P] float64 (the offset that protects it), status [C, P] int32 (0, or
_lib.CAL_VACUOUS / CAL_SKIPPED), and the workspace buffer the call owns.  See
ccmpc_risk_quantile in include/ccmpc.h."""

_REC_KINDS = (_lib.REC_KIND_HALFSPACE, _lib.REC_KIND_AFFINE, _lib.REC_KIND_HALFSPACE_COMPACT,
              _lib.REC_KIND_AFFINE_COMPACT)


def _rec_layout(rec_kind):
    """(record bytes, byte offset of the rhs field, byte offset and width of side)."""
    if rec_kind == _lib.REC_KIND_HALFSPACE:
        f = _lib.HALFSPACE_DTYPE.fields
        return 128, f["d"][1], f["side"][1], 4
    if rec_kind == _lib.REC_KIND_AFFINE:
        f = _lib.AFFINE_DTYPE.fields
        return 128, f["rhs"][1], f["side"][1], 4
    f = _lib.GATHER_DTYPE.fields
    return _lib.GATHER_DTYPE.itemsize, f["rhs"][1], f["side"][1], 2


def _rec_bytes(rec, rec_kind, C):
    if rec_kind not in _REC_KINDS:
        raise ValueError(f"unknown rec_kind {rec_kind!r}")
    width = _rec_layout(rec_kind)[0]
    if rec.dtype != torch.uint8:
        rec = rec.view(torch.uint8)
    rec = rec.reshape(C, -1, width) if rec.dim() != 3 else rec
    if rec.shape[0] != C or rec.shape[2] != width:
        raise ValueError(f"rec must be ({C}, P, {width}) bytes for rec_kind {rec_kind}")
    return rec


def record_fields(rec, rec_kind):
    """Host (n0, n1, rhs, side, status, t) arrays [C, P] of device (or host) record bytes of
    any of the four kinds: the fields ccmpc_risk_audit / ccmpc_risk_quantile read."""
    b = rec.detach().cpu().numpy() if torch.is_tensor(rec) else np.asarray(rec)
    b = np.ascontiguousarray(b).view(np.uint8)
    half = rec_kind in (_lib.REC_KIND_HALFSPACE, _lib.REC_KIND_HALFSPACE_COMPACT)
    if rec_kind == _lib.REC_KIND_HALFSPACE:
        h = b.view(_lib.HALFSPACE_DTYPE)[..., 0]
        rhs, t = h["d"], h["t_tau"]
    elif rec_kind == _lib.REC_KIND_AFFINE:
        h = b.view(_lib.AFFINE_DTYPE)[..., 0]
        rhs, t = h["rhs"], h["t"]
    else:
        h = b.view(_lib.GATHER_DTYPE)[..., 0]
        rhs, t = h["rhs"], h["t_tau"]
    t = t.astype(np.int64) >> 16 if half else t.astype(np.int64)
    return (h["n0"].copy(), h["n1"].copy(), rhs.copy(), h["side"].astype(np.float64),
            h["status"].astype(np.int64), t)


def risk_quantile(store, rec, rec_kind, allow=None, R=risk.R_COLLISION, T=None, out=None):
    """Monte-Carlo calibration of record offsets on a ParticleStore (ccmpc_risk_quantile): per
    record, the (allow[c] + 1)-th largest projection side * (n . p) of the cell's particles at
    the record's step, and the smallest offset for which the audit's predicate protects it --
    the offset that leaves at most allow[c] particles of the cell open.

    rec / rec_kind / R / T as risk_audit.  allow: particles a record may leave open, per cell:
    None (zeros), a host sequence (checked to be >= 0 here) or an int64 device tensor [C] (read
    unchecked; a negative entry marks the cell's records SKIPPED), e.g. risk.allow_counts.
    out: a previous RiskQuantile whose buffers and workspace are used again (nothing is allocated
    then, so the call can be captured).  Returns RiskQuantile; enqueues 17 launches on the
    current stream, never synchronises."""
    lib = _lib.load()
    dev = store.device
    C = store.n_cells
    T = store.T if T is None else int(T)
    if not 1 <= T <= store.T:
        raise ValueError(f"T = {T} outside [1, {store.T}] (the store's horizon)")
    if getattr(store, "offsets", None) and any(int(o) % 4 for o in store.offsets):
        raise ValueError("cell offsets must be multiples of 4 particles")
    if rec is None:
        raise ValueError("risk_quantile needs records")
    rec = _rec_bytes(rec, rec_kind, C)
    P = _audit_rows(rec_kind, T)
    if rec.shape[1] < P:
        raise ValueError(f"rec holds {rec.shape[1]} rows per cell, T = {T} needs {P}")
    if P and (rec.shape[1] != P or not rec.is_contiguous()):
        rec = rec[:, :P].contiguous()       # rows of a longer horizon's buffer
    if allow is None:
        pass
    elif torch.is_tensor(allow):
        if (allow.dtype != torch.int64 or tuple(allow.shape) != (C,) or allow.device != dev
                or not allow.is_contiguous()):
            raise ValueError(f"allow must be a contiguous int64 [{C}] tensor on {dev}")
    else:
        host = np.asarray(allow, np.int64).reshape(-1)
        if host.shape[0] != C or (C and host.min() < 0):
            raise ValueError(f"allow must hold {C} counts >= 0")
        allow = torch.as_tensor(host, device=dev)
    need = int(lib.ccmpc_risk_quantile_workspace_bytes(T, int(rec_kind), C))
    if need == 0:
        raise ValueError(f"ccmpc_risk_quantile rejects T = {T}, rec_kind = {rec_kind}")
    if out is None:
        out = RiskQuantile(torch.empty((C, P), dtype=torch.float64, device=dev),
                           torch.empty((C, P), dtype=torch.float64, device=dev),
                           torch.empty((C, P), dtype=torch.int32, device=dev),
                           torch.empty(need, dtype=torch.uint8, device=dev))
    else:
        for name in ("q", "rhs", "status"):
            t = getattr(out, name)
            if t is None or tuple(t.shape) != (C, P) or not t.is_contiguous():
                raise ValueError(f"out.{name} must be a contiguous {(C, P)} tensor")
        if out.workspace is None or out.workspace.numel() < need:
            raise ValueError(f"out.workspace must hold {need} bytes")
    if C == 0:
        return out
    _lib.check(lib.ccmpc_risk_quantile(
        _p(store.pos), store.ccmpc_dtype, store.ld, T, _p(store.origin), _p(store.cell_off),
        _p(store.cell_cnt), C, store.n_bound, _p(rec), int(rec_kind), float(R), _p(allow),
        _p(out.workspace), out.workspace.numel(), _p(out.q), _p(out.rhs), _p(out.status),
        _stream()), "ccmpc_risk_quantile")
    return out


def ideal_risk_quantile(prev_mean, prev_cov, src_cell, T, n_samples, rec, rec_kind, allow=None,
                        R=risk.R_COLLISION, x0=None, seed=0, seed_dev=None, rng_cell=None,
                        out=None):
    """risk_quantile on the samples of the ideal rollout, which are never materialised
    (ccmpc_ideal_risk_quantile): q, rhs and status equal, bit for bit, ideal_rollout(prev_mean,
    prev_cov, src_cell, T, n_samples, x0=x0, seed=seed, rng_cell=rng_cell) followed by
    risk_quantile on that store; every counting pass generates the samples again in registers.
    Records of a failed cell from its first failed step on are SKIPPED.

    Rollout arguments (src_cell, x0, seed, seed_dev, rng_cell) as ideal_risk_audit; rec /
    rec_kind / allow / R as risk_quantile, with n_samples particles in every cell.
    Returns (RiskQuantile, cell_status): cell_status [C] int32 is the rollout's.  out: a
    previous call's (RiskQuantile, cell_status) pair, or a bare RiskQuantile (the status is then
    not written and returned as None); nothing is allocated then, so the call can be captured.
    Enqueues 17 launches on the current stream, never synchronises."""
    lib = _lib.load()
    dev = prev_mean.device
    C = int(src_cell.shape[0])
    T_src = int(prev_mean.shape[1])
    T, n_samples = int(T), int(n_samples)
    if not 1 <= T <= T_src - 1:
        raise ValueError(f"T = {T} outside [1, {T_src - 1}] (the source horizon less one)")
    if rec is None:
        raise ValueError("ideal_risk_quantile needs records")
    rec = _rec_bytes(rec, rec_kind, C)
    P = _audit_rows(rec_kind, T)
    if rec.shape[1] < P:
        raise ValueError(f"rec holds {rec.shape[1]} rows per cell, T = {T} needs {P}")
    if P and (rec.shape[1] != P or not rec.is_contiguous()):
        rec = rec[:, :P].contiguous()       # rows of a longer horizon's buffer
    if allow is None:
        pass
    elif torch.is_tensor(allow):
        if (allow.dtype != torch.int64 or tuple(allow.shape) != (C,) or allow.device != dev
                or not allow.is_contiguous()):
            raise ValueError(f"allow must be a contiguous int64 [{C}] tensor on {dev}")
    else:
        host = np.asarray(allow, np.int64).reshape(-1)
        if host.shape[0] != C or (C and host.min() < 0):
            raise ValueError(f"allow must hold {C} counts >= 0")
        allow = torch.as_tensor(host, device=dev)
    need = int(lib.ccmpc_ideal_risk_quantile_workspace_bytes(T, int(rec_kind), C))
    if need == 0:
        raise ValueError(f"ccmpc_ideal_risk_quantile rejects T = {T}, rec_kind = {rec_kind}, "
                         f"n_cells = {C}")
    status = None
    if out is None:
        status = torch.empty(C, dtype=torch.int32, device=dev)
        out = RiskQuantile(torch.empty((C, P), dtype=torch.float64, device=dev),
                           torch.empty((C, P), dtype=torch.float64, device=dev),
                           torch.empty((C, P), dtype=torch.int32, device=dev),
                           torch.empty(need, dtype=torch.uint8, device=dev))
    else:
        if not isinstance(out, RiskQuantile):
            out, status = out
            if (status.dtype != torch.int32 or tuple(status.shape) != (C,)
                    or not status.is_contiguous()):
                raise ValueError(f"status must be a contiguous int32 [{C}] tensor")
        for name in ("q", "rhs", "status"):
            t = getattr(out, name)
            if t is None or tuple(t.shape) != (C, P) or not t.is_contiguous():
                raise ValueError(f"out.{name} must be a contiguous {(C, P)} tensor")
        if out.workspace is None or out.workspace.numel() < need:
            raise ValueError(f"out.workspace must hold {need} bytes")
    if C == 0:
        return out, status
    _lib.check(lib.ccmpc_ideal_risk_quantile(
        _p(prev_mean), _p(prev_cov), T_src, _p(src_cell), C, T, n_samples, _p(x0),
        int(seed) & (2**64 - 1), _p(seed_dev), _p(rng_cell),
        # no rows (T = 1 half-space kinds): rec is only checked to be non-null
        _p(rec) if P else _p(prev_mean), int(rec_kind), float(R), _p(allow),
        _p(out.workspace), out.workspace.numel(), _p(out.q), _p(out.rhs), _p(out.status),
        _p(status), _stream()), "ccmpc_ideal_risk_quantile")
    return out, status


def calibrated_records(rec, rec_kind, quant, mode="replace"):
    """A new uint8 tensor of `rec`'s layout whose rhs field (d of the half-space record, rhs of
    the affine record and of the compact packing) carries risk_quantile's offsets; `rec` itself
    is never written.  Device tensor ops only, no host round trip.
      "replace"  rhs <- quant.rhs
      "tighten"  whichever has the larger side*rhs: never less constrained than the analytic one
      "relax"    whichever has the smaller side*rhs
    Records that are VACUOUS or SKIPPED keep their rhs in every mode, as do rows past quant's."""
    if mode not in ("replace", "tighten", "relax"):
        raise ValueError(f"mode must be 'replace', 'tighten' or 'relax', not {mode!r}")
    C = int(quant.rhs.shape[0])
    out = _rec_bytes(rec, rec_kind, C).clone(memory_format=torch.contiguous_format)
    P = int(quant.rhs.shape[1])
    if out.shape[1] < P:
        raise ValueError(f"rec holds {out.shape[1]} rows per cell, the calibration {P}")
    if P == 0:
        return out
    _, o_rhs, o_side, w_side = _rec_layout(rec_kind)
    field = out[:, :P, o_rhs:o_rhs + 8].view(torch.float64)[..., 0]
    side = out[:, :P, o_side:o_side + w_side].view(
        torch.int32 if w_side == 4 else torch.int16)[..., 0].to(torch.float64)
    sel = quant.status == 0
    if mode == "tighten":
        sel = sel & (side * quant.rhs > side * field)
    elif mode == "relax":
        sel = sel & (side * quant.rhs < side * field)
    field.copy_(torch.where(sel, quant.rhs, field))
    return out


def bucket(z, sample_store, latent_pmf, minpos, filter_pmf=0.1, max_k=None):
    """GPU bucketing (ccmpc_bucket) of a sampler output (z [O,N], sample-order F32 store with
    one cell per OV) into kept-mode cells.  latent_pmf (O, L) is host data, as in the reference
    (latent_probs come back to the host in prediction.py:77-79).

    Returns (bucketed F32 ParticleStore with origin = minpos per cell, K per OV, cell_pmf
    [n_cells] device, init_center [n_cells, 2] device).  Device-side counts: store.counts holds
    capacity bounds until ``store.sync_counts()``.
    """
    lib = _lib.load()
    dev = sample_store.device
    pmf = np.asarray(latent_pmf, np.float64)
    O, L = pmf.shape
    N = int(z.shape[1])
    T = sample_store.T
    K, max_k, keep_map, cell_base = _bucket_plan(pmf, filter_pmf, max_k)
    region, cur = [], 0
    for o in range(O):
        region.append(cur)
        cur = _round4(cur + N + 4 * K[o])
    n_cells = int(sum(K))
    origin = np.repeat(np.asarray(minpos, np.float64).reshape(-1, 2), K, axis=0)
    out = ParticleStore(T, [0] * n_cells, dtype=torch.float32, device=dev, origin=origin,
                        capacity=cur)
    out.counts = None                                   # device-side until sync_counts()
    out.n_bound = cur
    t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    t_keep, t_nk, t_base = t(keep_map), t(np.asarray(K, np.int32)), t(cell_base)
    t_min = t(np.asarray(minpos, np.float64).reshape(-1, 2))
    t_reg = t(np.asarray(region, np.int64))
    pmf_out = torch.empty(n_cells, dtype=torch.float64, device=dev)
    centre = torch.empty((n_cells, 2), dtype=torch.float64, device=dev)
    need = lib.ccmpc_bucket_workspace_bytes(O, N, L, max_k)
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device=dev)   # zero-filled head: counters
    _lib.check(lib.ccmpc_bucket(_p(z), _p(sample_store.pos), sample_store.ld, T, O, N, L,
                                _p(t_keep), _p(t_nk), _p(t_base), max_k, _p(t_min), _p(t_reg),
                                _p(ws), ws.numel(), _p(out.pos), out.ld, _p(out.cell_off),
                                _p(out.cell_cnt), _p(pmf_out), _p(centre), _stream()),
               "ccmpc_bucket")
    out._keepalive = (t_keep, t_nk, t_base, t_min, t_reg, ws)
    return out, K, pmf_out, centre
