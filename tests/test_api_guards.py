"""The host API's scope guards (csrc/sketch_ctx.h): cleanup that must not
depend on every early return remembering it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_pass_times_survives_failed_staging(engine):
    """ske_swipes opens its pass-timing marks (kinds 8: the host-fed call, 6:
    its H2D copies) before it stages the items.  A call whose staging fails
    (offsets that decrease: SKE_EINVAL) must leave no mark behind: the next
    call's marks are read by ske_pass_times, twice, and the failed call
    contributes nothing (a half-recorded mark made every later
    ske_pass_times fail in hipEventElapsedTime)."""
    from rtsas_amd._lib import SKE_EINVAL, SKE_MEM_HOST, SKE_OK
    from rtsas_amd.engine import PASS_KINDS
    engine.reserve(0, 0.01, 1000)
    engine.hll_reserve(2)
    engine.set_option("pass_timing", 1)
    lib, ctx = engine.ctx.lib, engine.ctx.ptr
    n = 8
    ids = np.frombuffer(b"10001100021000310004100051000610007100080000", np.uint8).copy()
    slot = np.zeros(n, np.uint32)
    good = (np.arange(n + 1) * 5).astype(np.uint32)
    bad = good.copy()
    bad[4] = 12  # 0 5 10 15 12 25 ...: decreases once, offs[n] >= offs[0]
    out = np.full(n, 7, np.uint8)

    def swipes(offs):
        return lib.ske_swipes(ctx, 0, _p(slot), _p(ids), _p(offs), n, _p(out), SKE_MEM_HOST)

    assert swipes(bad) == SKE_EINVAL
    assert swipes(good) == SKE_OK
    assert not out.any()  # nothing was added to the chain
    for _ in range(2):
        ms = (C.c_double * PASS_KINDS)()
        cnt = (C.c_uint64 * PASS_KINDS)()
        assert lib.ske_pass_times(ctx, ms, cnt, 0) == SKE_OK
        assert cnt[8] == 1 and cnt[6] == 1
        assert cnt[0] == 1 and cnt[7] == 1  # the one K1 kernel and the one D2H copy
