"""ccmpc_ideal_risk_quantile, host side: the binding's presence, the workspace query and the
argument rejection, which happens before any device call (so none of this needs a GPU).  Every
rejected call is made with n_cells = 0 and with n_cells = 3 and dummy host addresses: were a
check missing, the latter would go on to launch."""
import ctypes

import pytest

ERR_ARG = -1


def _call(lib, T_src=9, T=8, n_cells=3, n=1000, R=3.4, rec=True, kind=0, outs=(1, 1, 1),
          ws_bytes=None, ws_shift=0):
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16                                # a 16-byte aligned dummy address
    p = ctypes.c_void_p(base)
    null = ctypes.c_void_p(0)
    if ws_bytes is None:
        ws_bytes = max(int(lib.ccmpc_ideal_risk_quantile_workspace_bytes(T, kind, n_cells)), 64)
    q, rhs, st = (p if o else null for o in outs)
    return lib.ccmpc_ideal_risk_quantile(
        p, p, T_src, null, n_cells, T, n, null, 7, null, null, p if rec else null, kind, R,
        null, ctypes.c_void_p(base + ws_shift), ws_bytes, q, rhs, st, null, null)


@pytest.fixture(scope="module")
def lib():
    from ccmpc import _lib
    return _lib.load()


def test_binding_has_the_ideal_quantile(lib):
    from ccmpc import _lib, engine, planner
    for name, nargs in (("ccmpc_ideal_risk_quantile", 22),
                        ("ccmpc_ideal_risk_quantile_workspace_bytes", 3)):
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert callable(engine.ideal_risk_quantile)
    assert callable(planner.MidlevelAgent.calibrate_ideal_constraints)
    assert lib.ccmpc_abi_version() == 2          # an additive entry point


def test_workspace_query(lib):
    ws = lib.ccmpc_ideal_risk_quantile_workspace_bytes
    for kind in range(4):
        assert ws(7, kind, 9) > 0
        assert ws(39, kind, 65535) > 0
        assert ws(1, kind, 0) > 0
        # at least ccmpc_risk_quantile's record, bins and rank per record
        assert ws(7, kind, 9) >= lib.ccmpc_risk_quantile_workspace_bytes(7, kind, 9)
    assert ws(7, 0, 2) < ws(7, 0, 3) < ws(8, 0, 3)
    for T, kind, C in ((0, 0, 3), (40, 0, 3), (7, 4, 3), (7, -1, 3), (7, 0, -1), (7, 0, 65536)):
        assert ws(T, kind, C) == 0


def test_no_cells_and_no_rows_are_ok(lib):
    for kind in range(4):
        assert _call(lib, n_cells=0, kind=kind) == 0
    # T = 1 of the half-space kinds has no rows: no output is needed, nothing is launched
    assert _call(lib, n_cells=0, T_src=2, T=1, kind=0, outs=(0, 0, 0)) == 0
    assert _call(lib, n_cells=3, T_src=2, T=1, kind=2, outs=(0, 0, 0)) == 0


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
    (dict(kind=4), b"rec_kind"),
    (dict(kind=-1), b"rec_kind"),
    (dict(rec=False), b"rec is null"),
    (dict(outs=(0, 1, 1)), b"out_q"),
    (dict(outs=(1, 0, 1)), b"out_rhs"),
    (dict(outs=(1, 1, 0)), b"out_status"),
    (dict(kind=1, outs=(0, 0, 0)), b"null output"),
    (dict(ws_bytes=0), b"workspace too small"),
    (dict(ws_bytes=63), b"workspace too small"),
    (dict(ws_shift=8), b"16-byte aligned"),
])
def test_rejected_before_any_device_call(lib, n_cells, kw, msg):
    kw = dict(kw)
    kw.setdefault("n_cells", n_cells)
    assert _call(lib, **kw) == ERR_ARG
    err = lib.ccmpc_last_error()
    assert b"ccmpc_ideal_risk_quantile" in err and msg in err, err


def test_workspace_one_byte_short_is_rejected(lib):
    need = int(lib.ccmpc_ideal_risk_quantile_workspace_bytes(8, 0, 3))
    assert _call(lib, ws_bytes=need - 1) == ERR_ARG
    assert b"workspace too small" in lib.ccmpc_last_error()


def test_limits_are_accepted(lib):
    # the largest legal values, with no cells so nothing is launched
    assert _call(lib, n_cells=0, T_src=40, T=39, n=(1 << 32) - 1, kind=0) == 0
    assert _call(lib, n_cells=0, T_src=40, T=39, n=(1 << 32) - 1, kind=3) == 0
    assert _call(lib, n_cells=0, T_src=2, T=1, n=1, kind=1) == 0
    assert _call(lib, n_cells=0, R=5e-324) == 0
