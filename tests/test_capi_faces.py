"""The box-face chance-constraint entry points exist at every layer: header, library, ctypes
binding, planner mirror (host only; no device work)."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ccmpc.h")
LIB = os.path.join(ROOT, "cc-mpc_amd", "ccmpc", "libccmpc.so")
NAMES = ("ccmpc_face_workspace_bytes", "ccmpc_face_constraints")


def test_face_record_is_128_bytes():
    from ccmpc import _lib
    assert _lib.FACE_DTYPE.itemsize == 128
    assert _lib.FACE_DTYPE.names == ("mean", "root", "C", "status", "t_face_chosen")
    assert _lib.FACE_DTYPE.fields["status"][1] == 120


def test_symbols_declared_exported_and_bound():
    from ccmpc import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    lib = ctypes.CDLL(LIB)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert re.search(r"\bT " + name + r"\b", nm), name
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
    assert "typedef struct ccmpc_face_rec" in text
    assert len(_lib.SIGNATURES["ccmpc_face_constraints"][1]) == 20
    assert re.search(r"#define CCMPC_ABI_VERSION 2\b", text)


def test_workspace_bytes():
    from ccmpc import _lib
    lib = _lib.load()
    assert lib.ccmpc_face_workspace_bytes(8, 4, 20000) > 0
    assert lib.ccmpc_face_workspace_bytes(41, 4, 20000) == 0        # T > 40 rejected
    assert lib.ccmpc_face_workspace_bytes(0, 4, 20000) == 0
    assert lib.ccmpc_face_workspace_bytes(8, -1, 20000) == 0
    assert lib.ccmpc_face_workspace_bytes(8, 4, -1) == 0
    # one partial of 18 doubles per (item, t): at least that for the items the bound implies
    assert lib.ccmpc_face_workspace_bytes(8, 4, 20000) >= (20000 // 2048) * 8 * 18 * 8


def test_status_strings_unchanged():
    from ccmpc import _lib
    lib = _lib.load()
    assert lib.ccmpc_status_string(-12) == b"non-finite slope or moment"
    assert lib.ccmpc_status_string(-14) == (b"covariance not positive semi-definite "
                                            b"(complex sqrtm)")


def test_midlevel_agent_has_the_three_generators():
    from ccmpc import planner
    for name in ("compute_obstacle_constraints_GMM", "compute_robust_constraints_GMM",
                 "compute_obstacle_constraints_GMM_approx"):
        assert callable(getattr(planner.MidlevelAgent, name)), name
    assert hasattr(planner, "SocConstraint") and hasattr(planner, "FaceConstraintList")


def test_engine_binding():
    from ccmpc import engine
    assert callable(engine.face_constraints) and callable(engine.face_records)
