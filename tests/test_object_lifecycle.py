"""The lifecycle of the six id-addressed device objects (Count-Min tables,
heavy-hitter sets, time profiles, tallies, seen-row sets, row logs), call by
call through the C-ABI: the return code of every refusal and the text the three
busy refusals leave in ske_last_hip_error.

The expected codes are those of the six sketch_api_*.cpp units as they stood
before they shared one object table, the differences between the families
included: the heavy-hitter sets and the Count-Min tables look an id up without
range-checking it (an id at the maximum is "no such object", not EINVAL), and
their info does not refuse while a graph is being recorded (it fails on the
stream wait, SKE_EHIP)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, EINVAL, EHIP, EBUSY = 0, -1, -3, -13


def _family(pkg, name):
    L = pkg._lib
    two = lambda cap: (cap,)  # noqa: E731  init(id, capacity_log2)
    fam = {
        "cms": dict(max=L.SKE_MAX_CMS, info="ske_cms_info", struct=L.CmsInfo, nosuch=L.SKE_ECMSNOKEY,
                    exists=L.SKE_ECMSEXISTS, checked=False, info_refuses=False, reset=False,
                    args=(1, 1), noun="a Count-Min Sketch table", empty=dict(width=1, depth=1, count=0),
                    bad=[((0, 1), L.SKE_ECMSWIDTH), ((1, 0), L.SKE_ECMSDEPTH), ((1, 65), L.SKE_ECMSDEPTH),
                         ((1 << 26, 4), L.SKE_ECMSWIDTH)]),
        "hh": dict(max=L.SKE_MAX_HH, info="ske_hh_info", struct=L.HhInfo, nosuch=L.SKE_EHHNOSET,
                   exists=L.SKE_EHHEXISTS, checked=False, info_refuses=False, reset=True,
                   args=two(L.SKE_HH_MIN_LOG2), noun="a heavy-hitter set",
                   empty=dict(capacity=1 << L.SKE_HH_MIN_LOG2, used=0, overflow=0),
                   bad=[(two(L.SKE_HH_MIN_LOG2 - 1), L.SKE_EHHCAP), (two(L.SKE_HH_MAX_LOG2 + 1), L.SKE_EHHCAP)]),
        "tp": dict(max=L.SKE_MAX_TP, info="ske_tp_read", struct=None, nosuch=L.SKE_ETPNOSET,
                   exists=L.SKE_ETPEXISTS, checked=True, info_refuses=True, reset=True,
                   args=(), noun="a time profile", empty=None, bad=[]),
        "tally": dict(max=L.SKE_MAX_TALLY, info="ske_tally_info", struct=L.TallyInfo, nosuch=L.SKE_ETALLYNOSET,
                      exists=L.SKE_ETALLYEXISTS, checked=True, info_refuses=True, reset=True,
                      args=two(L.SKE_TALLY_MIN_LOG2), noun="a tally",
                      empty=dict(capacity=1 << L.SKE_TALLY_MIN_LOG2, used=0, overflow=0, taken=0, dropped_events=0,
                                 dropped_valid=0),
                      bad=[(two(L.SKE_TALLY_MIN_LOG2 - 1), L.SKE_ETALLYCAP),
                           (two(L.SKE_TALLY_MAX_LOG2 + 1), L.SKE_ETALLYCAP)]),
        "seen": dict(max=L.SKE_MAX_SEEN, info="ske_seen_info", struct=L.SeenInfo, nosuch=L.SKE_ESEENNOSET,
                     exists=L.SKE_ESEENEXISTS, checked=True, info_refuses=True, reset=True,
                     args=two(L.SKE_SEEN_MIN_LOG2), noun="a seen set",
                     empty=dict(capacity=1 << L.SKE_SEEN_MIN_LOG2, limit=(1 << L.SKE_SEEN_MIN_LOG2) // 2, used=0,
                                calls=0, looked_at=0, first=0, unplaced=0),
                     bad=[(two(L.SKE_SEEN_MIN_LOG2 - 1), L.SKE_ESEENCAP),
                          (two(L.SKE_SEEN_MAX_LOG2 + 1), L.SKE_ESEENCAP)]),
        "rows": dict(max=L.SKE_MAX_ROWS, info="ske_rows_info", struct=L.RowsInfo, nosuch=L.SKE_EROWSNOLOG,
                     exists=L.SKE_EROWSEXISTS, checked=True, info_refuses=True, reset=True,
                     args=two(L.SKE_ROWS_MIN_LOG2), noun="a row log",
                     empty=dict(capacity=1 << L.SKE_ROWS_MIN_LOG2, used=0, taken=0, refused_ids=0, dropped=0,
                                overflow=0),
                     bad=[(two(L.SKE_ROWS_MIN_LOG2 - 1), L.SKE_EROWSCAP),
                          (two(L.SKE_ROWS_MAX_LOG2 + 1), L.SKE_EROWSCAP)]),
    }[name]
    fam["name"] = name
    return fam


def _info_while_recording(pkg, F):
    """The code of the family's info inside a recording that info does not
    refuse.  The failed wait leaves the capture in a state the runtime may not
    leave again, so it is a context and a thread of its own (the capture is
    thread-local), both given up afterwards."""
    import threading
    got = {}

    def run():
        ctx = pkg.Context(0)
        lib = ctx.lib
        try:
            assert getattr(lib, f"ske_{F['name']}_init")(ctx.ptr, 1, *F["args"]) == OK
            assert lib.ske_capture_begin(ctx.ptr) == OK
            got["rc"] = getattr(lib, F["info"])(ctx.ptr, 1, C.byref(F["struct"]()))
            g = C.c_void_p()
            if lib.ske_capture_end(ctx.ptr, C.byref(g)) == OK and g.value:
                lib.ske_graph_free(ctx.ptr, g)
        finally:
            ctx.close()

    t = threading.Thread(target=run)
    t.start()
    t.join()
    return got.get("rc")


@pytest.mark.parametrize("name", ["cms", "hh", "tp", "tally", "seen", "rows"])
def test_lifecycle_codes(pkg, engine, name):
    from rtsas_amd.engine import DeviceBuffer
    F = _family(pkg, name)
    lib, ctx = engine.ctx.lib, engine.ctx.ptr
    oid, top = 3, F["max"]

    def call(what, i, *args):
        return getattr(lib, f"ske_{name}_{what}")(ctx, i, *args)

    def info(i):
        """the return code and, for the families with an info record, its fields"""
        if F["struct"] is None:
            out = np.full(pkg._lib.SKE_TP_BINS, 0xAB, np.uint64)
            rc = lib.ske_tp_read(ctx, i, pkg._lib.ptr(out))
            return rc, out
        rec = F["struct"]()
        rc = getattr(lib, F["info"])(ctx, i, C.byref(rec))
        return rc, {k: getattr(rec, k) for k, _ in rec._fields_}

    def last_error():
        return lib.ske_last_hip_error(ctx).decode()

    # an id at the maximum, a capacity outside the bounds, an id never initialised
    assert call("init", top, *F["args"]) == EINVAL
    for args, code in F["bad"]:
        assert call("init", oid, *args) == code, args
    outside = EINVAL if F["checked"] else F["nosuch"]
    for i, code in ((oid, F["nosuch"]), (top, outside)):
        assert info(i)[0] == code
        if F["reset"]:
            assert call("reset", i) == code
        assert call("free", i) == code

    assert call("init", oid, *F["args"]) == OK
    assert call("init", oid, *F["args"]) == F["exists"]

    # a recording: one time-profile add is what it holds
    tid = oid if name == "tp" else 200
    if name != "tp":
        engine.tp_init(tid)
    n = 64
    epoch = DeviceBuffer(engine.ctx, n * 8)
    epoch.from_host(np.arange(n, dtype=np.int64) * 3600)
    seen = {}

    def refusals():
        engine.tp_add(tid, epoch, n)
        if F["reset"]:
            seen["reset"] = (call("reset", oid), last_error())
        if F["info_refuses"]:
            seen["info"] = (info(oid)[0], last_error())
        seen["free"] = (call("free", oid), last_error())

    g = engine.capture(refusals)
    try:
        freed = f"{F['noun']} cannot be freed while a recorded graph may point to it"
        if F["reset"]:
            assert seen["reset"] == (EBUSY, f"ske_{name}_reset waits for the stream and cannot be recorded")
        if F["info_refuses"]:
            assert seen["info"] == (EBUSY, f"{F['info']} waits for the stream and cannot be recorded")
        assert seen["free"] == (EBUSY, freed)
        # the recorded graph is alive
        assert call("free", oid) == EBUSY and last_error() == freed
        assert info(oid)[0] == OK
    finally:
        g.free()

    if not F["info_refuses"]:
        # info takes no notice of a recording: its wait for the stream fails
        assert _info_while_recording(pkg, F) == EHIP

    # free, then the id is free again; a new object under it is empty
    assert call("free", oid) == OK
    assert info(oid)[0] == F["nosuch"] and call("free", oid) == F["nosuch"]
    assert call("init", oid, *F["args"]) == OK
    rc, rec = info(oid)
    assert rc == OK
    if F["struct"] is None:
        assert (rec == 0).all()
    else:
        assert rec == F["empty"]
    assert call("free", oid) == OK
    if name != "tp":
        engine.tp_free(tid)
    epoch.free()
