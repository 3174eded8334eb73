"""ccmpc_face_audit exists at every layer (header, library, ctypes binding, Python callers) and
rejects bad arguments before it touches a device (host only; no device work)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ccmpc.h")
LIB = os.path.join(ROOT, "cc-mpc_amd", "ccmpc", "libccmpc.so")
NAME = "ccmpc_face_audit"


def test_symbol_declared_exported_and_bound():
    from ccmpc import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    assert re.search(r"\b" + NAME + r"\s*\(", text)
    assert re.search(r"\bT " + NAME + r"\b", nm)
    assert hasattr(ctypes.CDLL(LIB), NAME)
    decl = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(_lib.SIGNATURES[NAME][1]) == len(decl.split(",")) == 23
    assert re.search(r"#define CCMPC_ABI_VERSION 2\b", text)


def _call(**over):
    """ccmpc_face_audit on host addresses it must never read: every case fails its checks."""
    from ccmpc import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float64)
    addr = buf.ctypes.data - buf.ctypes.data % 32 + 32
    a = dict(positions=addr, dtype=_lib.CCMPC_F64, ld=64, T=8, origin=None, cell_off=addr,
             cell_cnt=addr, n_cells=1, n_bound=64, past_last=addr, extent=addr, car_r=4.47213,
             plan=addr, ld_plan=2, cell_plan=None, face_sel=addr, face_open=addr, in_box=addr,
             in_box_any=addr, sel_open=addr, sel_open_any=addr, worst=addr)
    a.update(over)
    return lib.ccmpc_face_audit(
        a["positions"], a["dtype"], a["ld"], a["T"], a["origin"], a["cell_off"], a["cell_cnt"],
        a["n_cells"], a["n_bound"], a["past_last"], a["extent"], a["car_r"], a["plan"],
        a["ld_plan"], a["cell_plan"], a["face_sel"], a["face_open"], a["in_box"],
        a["in_box_any"], a["sel_open"], a["sel_open_any"], a["worst"], None)


@pytest.mark.parametrize("over", [
    dict(T=0), dict(T=41), dict(ld=62), dict(ld=0), dict(ld_plan=1), dict(ld_plan=0),
    dict(car_r=float("nan")), dict(car_r=float("inf")), dict(n_cells=-1),
    dict(positions=None), dict(cell_off=None), dict(cell_cnt=None), dict(past_last=None),
    dict(extent=None), dict(plan=None), dict(face_open=None), dict(in_box=None),
    dict(in_box_any=None), dict(sel_open=None), dict(sel_open_any=None),
    dict(sel_open=None, sel_open_any=None, worst=None),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_argument_errors(over):
    from ccmpc import _lib
    lib = _lib.load()
    assert _call(**over) == -1                                   # CCMPC_ERR_ARG
    assert b"ccmpc_face_audit" in lib.ccmpc_last_error()


def test_no_cells_is_a_no_op():
    assert _call(n_cells=0) == 0
    # without face_sel the sel outputs may be NULL, and out_worst is always optional
    assert _call(n_cells=0, face_sel=None, sel_open=None, sel_open_any=None, worst=None) == 0


def test_python_callers_exist():
    from ccmpc import engine, planner, risk
    assert callable(engine.face_audit) and callable(risk.face_audit_report)
    assert callable(planner.MidlevelAgent.audit_face_rows)
    assert engine.FaceAudit._fields == ("face_open", "in_box", "in_box_any", "sel_open",
                                        "sel_open_any", "worst")


def test_report_sets_fractions_beside_budgets():
    from ccmpc import engine, risk
    a = engine.FaceAudit(
        face_open=np.array([[[4, 0, 1, 2]], [[0, 0, 0, 0]]]), in_box=np.array([[0], [0]]),
        in_box_any=np.array([0, 0]), sel_open=np.array([[1], [-1]]),
        sel_open_any=np.array([1, 0]), worst=np.array([[[0.5, -1.0, 0.1, 0.2]],
                                                       [[-np.inf] * 4]]))
    rep = risk.face_audit_report(a, [4, 0], [2], 1, eps=0.5)
    assert np.array_equal(rep["p_face_open"][0, 0], [1.0, 0.0, 0.25, 0.5])
    assert np.all(np.isnan(rep["p_face_open"][1]))
    assert rep["p_sel_open"][0, 0] == 0.25 and np.isnan(rep["p_sel_open"][1, 0])
    assert np.array_equal(rep["has_row"], [[True], [False]])
    assert np.array_equal(rep["budget_step"], [0.5, 0.5])
    assert np.array_equal(rep["step_within_budget"], [[True], [False]])
    assert np.array_equal(rep["traj_within_budget"], [True, False])
    assert np.array_equal(rep["row_holds"][0, 0], [False, True, False, False])
    assert rep["worst_row"] == (0, 0) and rep["worst_p_sel_open"] == 0.25
