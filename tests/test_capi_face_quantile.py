"""ccmpc_face_quantile exists at every layer (header, library, ctypes binding, Python callers)
and rejects bad arguments before it touches a device (host only; no device work)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ccmpc.h")
LIB = os.path.join(ROOT, "cc-mpc_amd", "ccmpc", "libccmpc.so")
NAME = "ccmpc_face_quantile"
SIZE = "ccmpc_face_quantile_workspace_bytes"


def test_symbols_declared_exported_and_bound():
    from ccmpc import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    for name, nargs in ((NAME, 24), (SIZE, 2)):
        assert re.search(r"\b" + name + r"\s*\(", text)
        assert re.search(r"\bT " + name + r"\b", nm)
        assert hasattr(ctypes.CDLL(LIB), name)
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len(decl.split(",")) == nargs
    assert re.search(r"#define CCMPC_ABI_VERSION 2\b", text)


def _call(**over):
    """ccmpc_face_quantile on host addresses it must never read: every case fails its checks
    (or has no cells)."""
    from ccmpc import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float64)
    addr = buf.ctypes.data - buf.ctypes.data % 32 + 32
    a = dict(positions=addr, dtype=_lib.CCMPC_F64, ld=64, T=8, origin=None, cell_off=addr,
             cell_cnt=addr, n_cells=1, n_bound=64, past_last=addr, extent=addr, car_r=4.47213,
             plan=addr, ld_plan=2, cell_plan=None, allow=None, margin=0.0, ws=addr, ws_bytes=None,
             q=addr, arg=addr, cut=addr, status=addr)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = int(lib.ccmpc_face_quantile_workspace_bytes(8, max(a["n_cells"], 0)))
    return lib.ccmpc_face_quantile(
        a["positions"], a["dtype"], a["ld"], a["T"], a["origin"], a["cell_off"], a["cell_cnt"],
        a["n_cells"], a["n_bound"], a["past_last"], a["extent"], a["car_r"], a["plan"],
        a["ld_plan"], a["cell_plan"], a["allow"], a["margin"], a["ws"], a["ws_bytes"], a["q"],
        a["arg"], a["cut"], a["status"], None)


@pytest.mark.parametrize("over", [
    # ccmpc_face_audit's cases
    dict(T=0), dict(T=41), dict(ld=62), dict(ld=0), dict(ld_plan=1), dict(ld_plan=0),
    dict(car_r=float("nan")), dict(car_r=float("inf")), dict(n_cells=-1), dict(dtype=2),
    dict(n_bound=-1), dict(positions=None), dict(cell_off=None), dict(cell_cnt=None),
    dict(past_last=None), dict(extent=None), dict(plan=None),
    dict(q=None), dict(arg=None), dict(cut=None), dict(status=None),
    # its own
    dict(margin=-1e-9), dict(margin=float("nan")), dict(margin=float("inf")),
    dict(ws_bytes=0), dict(ws_bytes=8 * 4 * 1048 + 63), dict(ws=None), dict(n_bound=1 << 32),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_argument_errors(over):
    from ccmpc import _lib
    lib = _lib.load()
    assert _call(**over) == -1                                   # CCMPC_ERR_ARG
    assert b"ccmpc_face_quantile" in lib.ccmpc_last_error()


def test_misaligned_workspace_is_rejected():
    buf = np.zeros(64, np.float64)
    addr = buf.ctypes.data - buf.ctypes.data % 32 + 32
    assert _call(ws=addr + 8) == -1
    assert _call(cut=addr + 8) == -1


def test_no_cells_is_a_no_op():
    assert _call(n_cells=0) == 0
    assert _call(n_cells=0, ws=None, ws_bytes=64) == 0


def test_workspace_size():
    from ccmpc import _lib
    lib = _lib.load()
    size = lib.ccmpc_face_quantile_workspace_bytes
    for T, C in ((0, 1), (41, 1), (8, -1), (8, 1 << 30)):
        assert size(T, C) == 0
    assert size(8, 0) > 0
    # O(cells T): 1 KiB of bins and 24 bytes of state per (cell, t, face), whatever the store
    assert size(8, 3) == 3 * 8 * 4 * 1048 + 64
    assert size(40, 67) == 67 * 40 * 4 * 1048 + 64


def test_python_callers_exist():
    from ccmpc import engine, mpc, planner, risk
    assert callable(engine.face_quantile) and callable(risk.face_calibration_report)
    assert callable(planner.MidlevelAgent.calibrate_face_rows)
    assert callable(planner.MidlevelAgent.tighten_face_plan)
    assert engine.FaceQuantile._fields == ("q", "arg", "cut", "status")
    assert (mpc.TIGHTEN_OK, mpc.TIGHTEN_INFEASIBLE, mpc.TIGHTEN_MAXROUNDS) == (0, 1, 8)
    assert callable(mpc.PlanningTighten)


def test_report_on_fabricated_arrays():
    from ccmpc import engine, risk
    inf, nan = np.inf, np.nan
    q = np.array([[[0.5, -1.0, 0.0, 0.2], [-0.1, -0.2, 0.3, 0.4]],
                  [[-inf] * 4, [-inf] * 4],
                  [[nan] * 4, [nan] * 4]])
    quant = engine.FaceQuantile(q=q, arg=np.zeros((3, 2, 4), np.int64), cut=None,
                                status=np.array([[0, 0], [1, 1], [2, 2]]))
    sel = np.array([[0, 1], [2, -1], [3, 3]])
    rep = risk.face_calibration_report(quant, [640, 2, 5], [3], 2, face_sel=sel, eps=0.01)
    assert np.allclose(rep["budget_step"], 0.005) and np.array_equal(rep["allow"], [3, 0, 0])
    assert np.array_equal(rep["margin_sel"][0], [0.5, -0.2])
    assert rep["margin_sel"][1, 0] == -inf and np.isnan(rep["margin_sel"][1, 1])
    assert np.all(np.isnan(rep["margin_sel"][2]))
    assert np.array_equal(rep["step_meets_budget"], [[False, True], [True, False], [False, False]])
    assert np.array_equal(rep["meets_budget"][0, 0], [False, True, True, False])
    assert rep["worst_row"] == (0, 0) and rep["worst_margin"] == 0.5
    bare = risk.face_calibration_report(quant, [640, 2, 5], [3], 2, eps=0.01)
    assert bare["margin_sel"] is None and bare["worst_row"] is None
    empty = risk.face_calibration_report(
        engine.FaceQuantile(q=np.full((1, 1, 4), -inf), arg=np.full((1, 1, 4), -1), cut=None,
                            status=np.array([[1]])), [0], [1], 1, face_sel=np.array([[0]]))
    assert np.isnan(empty["margin_sel"][0, 0]) and not empty["step_meets_budget"][0, 0]
