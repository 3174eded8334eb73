"""Host-side risk allocation constants (v8ideal/__init__.py:2920-2926, :910-913, :1481-1482).

These are per-cell scalars computed once per planning step with the same scipy calls the
reference makes inside its inner loop; the kernels receive them as data.
"""
import functools

import numpy as np
import scipy.stats

EPS_TOTAL = 0.05      # v8ideal/__init__.py:2920
TARGET_P = 0.9999     # v8ideal/__init__.py:912
R_COLLISION = 3.4     # v8ideal/__init__.py:795


def eps_ura(K, eps=EPS_TOTAL):
    """eps_ura[i, k] = eps / O for every mode of every OV (not divided by K)."""
    K = [int(k) for k in K]
    O = len(K)
    out = np.zeros((O, max(K) if O else 0))
    for i, k in enumerate(K):
        out[i, :k] = eps / O
    return out


@functools.lru_cache(maxsize=4096)
def _chi2_ppf2(p):
    """scipy.stats.chi2.ppf(p, df=2), memoised: the reference's value, computed once per
    distinct probability (a planning episode reuses a handful)."""
    return float(scipy.stats.chi2.ppf(p, df=2))


@functools.lru_cache(maxsize=4096)
def _norm_ppf(p):
    return float(scipy.stats.norm.ppf(p))


def cell_risk(eps_ura_mat, K, ph, target_p=TARGET_P):
    """(n_cells, 3) = chi2.ppf(1-eps_ijt, 2), chi2.ppf(target_p, 2), norm.ppf(1-eps_ijt) with
    eps_ijt = eps_ura[ov, k] / ph, cells in (ov, k) order."""
    chi_p = _chi2_ppf2(float(target_p))
    rows = []
    for o, k_o in enumerate(K):
        for k in range(int(k_o)):
            e = float(eps_ura_mat[o, k]) / ph
            rows.append((_chi2_ppf2(1 - e), chi_p, _norm_ppf(1 - e)))
    return np.asarray(rows, dtype=np.float64).reshape(-1, 3)


def scenes_cell_risk(scene_K, ph, target_p=TARGET_P):
    """cell_risk of several independent planning steps batched into one cycle: each scene
    allocates its own risk, eps_ura = 0.05 / O_scene (v8ideal/__init__.py:2920-2926)."""
    parts = [cell_risk(eps_ura(K), K, ph, target_p) for K in scene_K]
    return np.concatenate(parts, 0) if parts else np.zeros((0, 3))


def cell_gamma(eps_ura_mat, K, ph):
    """(n_cells,) = norm.ppf(1 - eps_ura[ov, k] / ph) for the GMM-affine generator."""
    return cell_risk(eps_ura_mat, K, ph)[:, 2].copy()


def _np(x):
    if x is None:
        return None
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _cell_budgets(K, ph, eps):
    """(budget_traj [C], budget_step [C]) = eps_ura[o, k] and eps_ura[o, k] / ph, cells in
    (ov, k) order."""
    K = [int(k) for k in K]
    e = eps_ura(K, eps)
    traj = np.array([e[o, k] for o, k_o in enumerate(K) for k in range(k_o)], np.float64)
    return traj, traj / ph


def audit_report(audit, counts, K, ph, eps=EPS_TOTAL):
    """Host-side report of an engine.RiskAudit (device tensors or arrays) against the risk
    budget: counts [n_cells] particles per cell, K modes per OV (cells in (ov, k) order), ph the
    horizon the per-step budget is split over.  Reports only: raises nothing about the risk and
    changes no planner decision.  Returns a dict of NumPy arrays --
      p_hit [C, T], p_hit_any [C], p_open [C, T]  counts over N_c (nan for an empty cell; None
                                                  for a half the audit did not run)
      min_dist [C, T]                             sqrt(min_d2)
      hit, hit_any, open, min_d2, rec_open        the audit's own arrays (rec_open -1: record
                                                  not audited), counts [C] = N_c
      budget_traj [C] = eps_ura[o, k], budget_step [C] = eps_ura[o, k] / ph
      traj_within_budget [C]    p_hit_any <= budget_traj   (False for an empty cell's nan)
      step_within_budget [C, T] p_hit <= budget_step
      worst (cell, t)           the step with the largest p_hit (None without a plan or
                                without particles), worst_p_hit its value."""
    K = [int(k) for k in K]
    n = np.asarray(counts, np.float64).reshape(-1)
    if n.shape[0] != sum(K):
        raise ValueError(f"{n.shape[0]} cell counts for {sum(K)} cells")
    budget_traj, budget_step = _cell_budgets(K, ph, eps)
    hit, hit_any, min_d2 = _np(audit.hit), _np(audit.hit_any), _np(audit.min_d2)
    rec_open, opn = _np(audit.rec_open), _np(audit.open)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.where(n > 0, n, np.nan)
        p_hit = None if hit is None else hit / den[:, None]
        p_hit_any = None if hit_any is None else hit_any / den
        p_open = None if opn is None else opn / den[:, None]
        min_dist = None if min_d2 is None else np.sqrt(min_d2)
    out = dict(p_hit=p_hit, p_hit_any=p_hit_any, p_open=p_open, min_dist=min_dist,
               hit=hit, hit_any=hit_any, open=opn, min_d2=min_d2, counts=n.astype(np.int64),
               rec_open=rec_open, budget_traj=budget_traj, budget_step=budget_step,
               traj_within_budget=None, step_within_budget=None, worst=None, worst_p_hit=None)
    if p_hit is not None:
        with np.errstate(invalid="ignore"):
            out["traj_within_budget"] = p_hit_any <= budget_traj
            out["step_within_budget"] = p_hit <= budget_step[:, None]
        if p_hit.size and not np.all(np.isnan(p_hit)):
            c, t = np.unravel_index(int(np.nanargmax(p_hit)), p_hit.shape)
            out["worst"] = (int(c), int(t))
            out["worst_p_hit"] = float(p_hit[c, t])
    return out


def face_audit_report(audit, counts, K, ph, eps=EPS_TOTAL):
    """Host-side report of an engine.FaceAudit (device tensors or arrays) against the risk
    budget the face rows' Gamma was sized for: counts [n_cells] particles per cell, K modes per
    OV (cells in (ov, k) order), ph the horizon the per-step budget is split over.  Reports
    only: it judges nothing beyond the within_budget booleans and changes no planner decision.
    Returns a dict of NumPy arrays --
      face_open [C, T, 4], in_box [C, T], in_box_any [C], sel_open [C, T] (-1: no row),
      sel_open_any [C], worst [C, T, 4]   the audit's own arrays (None for a part not run)
      p_face_open [C, T, 4], p_in_box [C, T], p_in_box_any [C]   counts over N_c (nan for an
                                          empty cell)
      p_sel_open [C, T]                   sel_open / N_c, nan where (c, t) has no row
      p_sel_open_any [C]                  sel_open_any / N_c
      has_row [C, T]                      sel_open >= 0 (None without face_sel)
      counts [C] = N_c, budget_traj [C] = eps_ura[o, k], budget_step [C] = eps_ura[o, k] / ph
      step_within_budget [C, T]  p_sel_open <= budget_step   (False where there is no row or no
                                 particle; None without face_sel)
      traj_within_budget [C]     p_sel_open_any <= budget_traj (False for an empty cell)
      row_holds [C, T, 4]        worst <= 0: row f holds for every particle (None without worst)
      worst_row (cell, t)        the row with the largest p_sel_open (None without one),
      worst_p_sel_open           its value."""
    K = [int(k) for k in K]
    n = np.asarray(counts, np.float64).reshape(-1)
    if n.shape[0] != sum(K):
        raise ValueError(f"{n.shape[0]} cell counts for {sum(K)} cells")
    budget_traj, budget_step = _cell_budgets(K, ph, eps)
    face_open, in_box, in_box_any = _np(audit.face_open), _np(audit.in_box), _np(audit.in_box_any)
    sel_open, sel_open_any, worst = _np(audit.sel_open), _np(audit.sel_open_any), _np(audit.worst)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.where(n > 0, n, np.nan)
        out = dict(face_open=face_open, in_box=in_box, in_box_any=in_box_any, sel_open=sel_open,
                   sel_open_any=sel_open_any, worst=worst,
                   p_face_open=face_open / den[:, None, None], p_in_box=in_box / den[:, None],
                   p_in_box_any=in_box_any / den, p_sel_open=None, p_sel_open_any=None,
                   has_row=None, counts=n.astype(np.int64), budget_traj=budget_traj,
                   budget_step=budget_step, step_within_budget=None, traj_within_budget=None,
                   row_holds=None if worst is None else worst <= 0.0, worst_row=None,
                   worst_p_sel_open=None)
        if sel_open is not None:
            has_row = sel_open >= 0
            p_sel = np.where(has_row, sel_open / den[:, None], np.nan)
            p_any = sel_open_any / den
            out.update(has_row=has_row, p_sel_open=p_sel, p_sel_open_any=p_any,
                       step_within_budget=p_sel <= budget_step[:, None],
                       traj_within_budget=p_any <= budget_traj)
            if p_sel.size and not np.all(np.isnan(p_sel)):
                c, t = np.unravel_index(int(np.nanargmax(p_sel)), p_sel.shape)
                out["worst_row"] = (int(c), int(t))
                out["worst_p_sel_open"] = float(p_sel[c, t])
    return out


def allow_counts(counts, K, ph, eps=EPS_TOTAL):
    """(n_cells,) int64 = floor(eps_ura[o, k] / ph * N_c): the particles of cell c a record may
    leave open without exceeding the per-step budget audit_report sets its counts beside
    (engine.risk_quantile's `allow`).  0 for an empty cell."""
    n = np.asarray(counts, np.float64).reshape(-1)
    if n.shape[0] != sum(int(k) for k in K):
        raise ValueError(f"{n.shape[0]} cell counts for {sum(int(k) for k in K)} cells")
    return np.floor(_cell_budgets(K, ph, eps)[1] * n).astype(np.int64)


def face_calibration_report(quant, counts, K, ph, face_sel=None, eps=EPS_TOTAL):
    """Host-side report of an engine.FaceQuantile (device tensors or arrays) computed with
    allow = allow_counts(counts, K, ph, eps): counts [n_cells], K and ph as face_audit_report;
    face_sel [C, T]: 0..3 the face that is the row of (c, t), anything else no row (None: no
    selected-row entries).  Reports only.  Returns a dict of NumPy arrays --
      q [C, T, 4], arg [C, T, 4], status [C, T]   the call's own arrays (status 0 selected,
                                1 vacuous: allow >= N_c, 2 skipped)
      counts [C], budget_step [C] = eps_ura[o, k] / ph, allow [C] = allow_counts(...)
      meets_budget [C, T, 4]    q <= 0: face f's row leaves at most allow particles open
      margin_sel [C, T]         q at the selected face, in metres: by how far the row misses
                                (> 0) or clears (<= 0) the budget; -inf for a vacuous row, nan
                                without a row, for a skipped one and for an empty cell (None
                                without face_sel)
      step_meets_budget [C, T]  margin_sel <= 0 (False where it is nan)
      worst_row (cell, t)       the row with the largest margin_sel (None without one),
      worst_margin              its value."""
    n = np.asarray(counts, np.float64).reshape(-1)
    q, arg = _np(quant.q), _np(quant.arg)
    status = _np(quant.status).astype(np.int64)
    C, T = status.shape
    if n.shape[0] != C:
        raise ValueError(f"{n.shape[0]} cell counts for {C} cells")
    with np.errstate(invalid="ignore"):
        out = dict(q=q, arg=arg, status=status, counts=n.astype(np.int64),
                   budget_step=_cell_budgets(K, ph, eps)[1], allow=allow_counts(n, K, ph, eps),
                   meets_budget=q <= 0.0, margin_sel=None, step_meets_budget=None,
                   worst_row=None, worst_margin=None)
        if face_sel is not None:
            sel = np.asarray(_np(face_sel), np.int64)
            if sel.shape != (C, T):
                raise ValueError(f"face_sel must be ({C}, {T})")
            # a vacuous row of a cell with particles clears any budget (q = -inf); an empty cell
            # has no fraction to meet one with, as in face_audit_report
            has = (sel >= 0) & (sel <= 3) & (status != 2) & (n > 0)[:, None]
            qs = np.take_along_axis(q, np.clip(sel, 0, 3)[..., None], -1)[..., 0]
            m = np.where(has, qs, np.nan)
            out.update(margin_sel=m, step_meets_budget=m <= 0.0)
            if m.size and not np.all(np.isnan(m)):
                c, t = np.unravel_index(int(np.nanargmax(m)), m.shape)
                out["worst_row"] = (int(c), int(t))
                out["worst_margin"] = float(m[c, t])
    return out


def calibration_report(quant, fields, counts, K, ph, eps=EPS_TOTAL):
    """Host-side report of an engine.RiskQuantile (device tensors or arrays) beside the analytic
    records it calibrated.  fields: the records' (n0, n1, rhs, side, ...) arrays [C, P]
    (engine.record_fields); counts [n_cells], K and ph as audit_report.  Reports only.  Returns
    a dict of NumPy arrays --
      status [C, P]        0 calibrated, 1 vacuous (allow >= N_c), 2 skipped
      q, rhs_cal [C, P]    the selected projection and the calibrated offset; rhs the analytic one
      slack [C, P]         side*rhs - side*rhs_cal: how far the analytic record stands beyond the
                           empirical one (positive) or short of it (negative); nan where the
                           record is not calibrated
      slack_m [C, P]       slack / |n|, in metres
      counts [C], budget_step [C] = eps_ura[o, k] / ph, allow [C] = allow_counts(...)
      worst_rec [C]        the calibrated record with the smallest slack_m (-1: none),
      worst_slack_m [C]    its slack_m (nan: none)."""
    n = np.asarray(counts, np.float64).reshape(-1)
    status = _np(quant.status).astype(np.int64)
    q, rhs_cal = _np(quant.q), _np(quant.rhs)
    C, P = status.shape
    if n.shape[0] != C:
        raise ValueError(f"{n.shape[0]} cell counts for {C} cells")
    n0, n1, rhs, side = (np.asarray(f, np.float64)[:, :P] for f in tuple(fields)[:4])
    cal = status == 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        slack = np.where(cal, side * rhs - side * rhs_cal, np.nan)
        slack_m = slack / np.sqrt(n0 * n0 + n1 * n1)
    worst_rec = np.full(C, -1, np.int64)
    worst = np.full(C, np.nan)
    for c in range(C):
        ok = cal[c] & ~np.isnan(slack_m[c])
        if ok.any():
            p = int(np.argmin(np.where(ok, slack_m[c], np.inf)))
            worst_rec[c], worst[c] = p, slack_m[c, p]
    return dict(status=status, q=q, rhs_cal=rhs_cal, rhs=rhs, slack=slack, slack_m=slack_m,
                counts=n.astype(np.int64), budget_step=_cell_budgets(K, ph, eps)[1],
                allow=allow_counts(n, K, ph, eps), worst_rec=worst_rec, worst_slack_m=worst)
