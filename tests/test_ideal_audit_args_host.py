"""ccmpc_ideal_risk_audit, host side: the binding's presence and the argument rejection, which
happens before any device call (so none of this needs a GPU).  Every rejected call is made with
n_cells = 3 and dummy host addresses: were a check missing, the call would go on to launch."""
import ctypes

import pytest

ERR_ARG = -1


def _call(lib, T_src=9, T=8, n_cells=3, n=1000, R=3.4, plan=True, rec=False, kind=0,
          plan_outs=True, rec_outs=True, rec_open=True):
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    po = p if plan_outs else null
    ro = p if rec_outs else null
    return lib.ccmpc_ideal_risk_audit(
        p, p, T_src, null, n_cells, T, n, null, 7, null, null, p if plan else null, null,
        p if rec else null, kind, R, po, po, po, ro if rec_open else null, ro, null, null)


@pytest.fixture(scope="module")
def lib():
    from ccmpc import _lib
    return _lib.load()


def test_binding_has_the_ideal_audit(lib):
    from ccmpc import _lib, engine, planner
    assert "ccmpc_ideal_risk_audit" in _lib.SIGNATURES
    assert hasattr(lib, "ccmpc_ideal_risk_audit")
    assert len(_lib.SIGNATURES["ccmpc_ideal_risk_audit"][1]) == 23
    assert callable(engine.ideal_risk_audit)
    assert callable(planner.MidlevelAgent.audit_ideal_plan)
    assert lib.ccmpc_abi_version() == 2          # an additive entry point


def test_no_cells_is_ok(lib):
    assert _call(lib, n_cells=0) == 0
    assert _call(lib, n_cells=0, rec=True, kind=3) == 0
    assert _call(lib, n_cells=0, plan=False, rec=True, kind=1) == 0
    # T = 1 of the half-space kinds has no rows: out_rec_open may be null
    assert _call(lib, n_cells=0, T_src=2, T=1, rec=True, kind=0, rec_open=False) == 0


@pytest.mark.parametrize("n_cells", [0, 3])
@pytest.mark.parametrize("kw, msg", [
    (dict(T_src=1, T=1), b"T_src must be"),
    (dict(T_src=41), b"T_src must be"),
    (dict(T=0), b"T must be"),
    (dict(T=9), b"T must be"),                         # T_src - 1 = 8 is the last
    (dict(T_src=40, T=40), b"T must be"),
    (dict(n_cells=-1), b"n_cells"),
    (dict(n_cells=65536), b"n_cells"),
    (dict(n=0), b"n_samples"),
    (dict(n=1 << 32), b"n_samples"),
    (dict(R=0.0), b"R must be"),
    (dict(R=-1.0), b"R must be"),
    (dict(R=float("inf")), b"R must be"),
    (dict(R=float("nan")), b"R must be"),
    (dict(rec=True, kind=4), b"rec_kind"),
    (dict(rec=True, kind=-1), b"rec_kind"),
    (dict(plan=False, rec=False), b"both null"),
    (dict(plan_outs=False), b"plan half needs"),
    (dict(plan=False, rec=True, rec_outs=False), b"record half needs"),
    (dict(rec=True, kind=1, rec_outs=False), b"record half needs"),
    (dict(rec=True, kind=0, rec_open=False), b"record half needs"),
])
def test_rejected_before_any_device_call(lib, n_cells, kw, msg):
    kw = dict(kw)
    kw.setdefault("n_cells", n_cells)
    assert _call(lib, **kw) == ERR_ARG
    assert msg in lib.ccmpc_last_error(), lib.ccmpc_last_error()


def test_limits_are_accepted(lib):
    # the largest legal values, with no cells so nothing is launched
    assert _call(lib, n_cells=0, T_src=40, T=39, n=(1 << 32) - 1, rec=True, kind=0) == 0
    assert _call(lib, n_cells=0, T_src=2, T=1, n=1) == 0
