"""ccmpc_face_cuts exists at every layer (header, library, ctypes binding, Python callers) and
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
NAME = "ccmpc_face_cuts"


def test_symbol_declared_exported_and_bound():
    from ccmpc import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    assert re.search(r"\b" + NAME + r"\s*\(", text)
    assert re.search(r"\bT " + NAME + r"\b", nm)
    assert hasattr(ctypes.CDLL(LIB), NAME)
    decl = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(_lib.SIGNATURES[NAME][1]) == len(decl.split(",")) == 19
    assert re.search(r"#define CCMPC_ABI_VERSION 2\b", text)
    for name, val in (("CCMPC_SOCP_OK", _lib.SOCP_OK), ("CCMPC_SOCP_CUT", _lib.SOCP_CUT),
                      ("CCMPC_SOCP_BAD_ROW", _lib.SOCP_BAD_ROW),
                      ("CCMPC_SOCP_BAD_LAYOUT", _lib.SOCP_BAD_LAYOUT),
                      ("CCMPC_CUT_EMPTY", _lib.CUT_EMPTY)):
        assert re.search(rf"#define {name} {val}\b", text), name


def _call(**over):
    """ccmpc_face_cuts on host addresses it must never read: every case fails its checks."""
    from ccmpc import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.float64)           # 16-byte aligned or better
    addr = buf.ctypes.data - buf.ctypes.data % 32 + 32
    a = dict(rec=addr, T=8, S=1, scene_cell=addr, face_sel=None, gamma=addr, car_r=4.47213,
             plan=addr, ld_plan=4, round=0, max_rounds=12, tol_g=1e-6, only_violated=0,
             pool=addr, pool_cell=addr, out_g=addr, out_viol=addr, out_state=addr)
    a.update(over)
    return lib.ccmpc_face_cuts(a["rec"], a["T"], a["S"], a["scene_cell"], a["face_sel"],
                               a["gamma"], a["car_r"], a["plan"], a["ld_plan"], a["round"],
                               a["max_rounds"], a["tol_g"], a["only_violated"], a["pool"],
                               a["pool_cell"], a["out_g"], a["out_viol"], a["out_state"], None)


@pytest.mark.parametrize("over", [
    dict(T=0), dict(T=41), dict(tol_g=float("nan")), dict(tol_g=float("inf")),
    dict(car_r=float("inf")), dict(car_r=float("nan")), dict(round=-1), dict(round=13),
    dict(max_rounds=-1), dict(round=1, max_rounds=0), dict(ld_plan=1), dict(S=-1),
    dict(pool=None), dict(out_g=None), dict(out_viol=None), dict(out_state=None),
    dict(rec=None), dict(scene_cell=None), dict(gamma=None), dict(plan=None),
    dict(pool_cell=None),
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_argument_errors(over):
    from ccmpc import _lib
    lib = _lib.load()
    assert _call(**over) == -1                                   # CCMPC_ERR_ARG
    assert b"ccmpc_face_cuts" in lib.ccmpc_last_error()


def test_no_scenes_is_a_no_op():
    assert _call(S=0) == 0


def test_python_callers_exist():
    from ccmpc import engine, mpc, planner
    assert callable(engine.face_cuts)
    assert callable(mpc.PlanningSOCP) and callable(mpc.PlanningSOCP.solve)
    assert callable(planner.MidlevelAgent.solve_planning_socp)
    assert callable(planner.MidlevelAgent.audit_face_plan)
    codes = (mpc.SOCP_OK, mpc.SOCP_INFEASIBLE, mpc.SOCP_NUMERIC, mpc.SOCP_MAXROUNDS,
             mpc.SOCP_BAD_ROW)
    assert len(set(codes)) == 5
    assert mpc.SOCP_INFEASIBLE == mpc.QP_MAXITER and mpc.SOCP_NUMERIC == mpc.QP_NUMERIC
