"""The redis-py facade, pinned: a fixed script of commands runs on a
``SketchClient`` over a context stub (tests/facade_stub.py), and for each step
the reply (or the exception's type and text) and the native calls made, with
their scalar arguments, are compared with tests/golden/facade_transcript.json.

What this pins is dispatch, arity, argument checks, key-table transitions and
the native call sequence; the stub leaves every output zeroed, so the values
are the GPU suite's business.  The expectation was recorded from the facade as
it stood before it was split into modules (commit f72973a) with
``python tests/test_facade_transcript.py --write`` and must only ever be
re-recorded from a revision whose behaviour is the wanted one."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "facade_transcript.json")


def _norm(v):
    """A reply as JSON can hold it."""
    if isinstance(v, BaseException):
        return {"raised": type(v).__name__, "text": str(v)}
    if isinstance(v, (bytes, bytearray)):
        return {"bytes": bytes(v).hex()}
    if isinstance(v, np.ndarray):
        return {"array": str(v.dtype), "values": v.tolist()}
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [_norm(x) for x in v]
    if isinstance(v, dict):
        return {(k.decode() if isinstance(k, bytes) else str(k)): _norm(x) for k, x in v.items()}
    if isinstance(v, set):
        return sorted(_norm(x) for x in v)
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if type(v).__name__ in ("BFInfo", "CMSInfo"):
        return {type(v).__name__: _norm(vars(v))}
    return f"<{type(v).__name__}>"


class _Recorder:
    def __init__(self, pkg, decode_responses=True, fail=None):
        from facade_stub import StubContext
        self.ctx = StubContext(pkg.load_library(), fail)
        self.cl = pkg.SketchClient(decode_responses=decode_responses, context=self.ctx)
        self.steps = []

    def do(self, label, fn, *args, **kw):
        n0 = len(self.ctx.log)
        try:
            reply = fn(*args, **kw)
            if hasattr(reply, "__next__"):
                reply = list(reply)
        except Exception as e:  # the facade's own refusals, whatever their type
            reply = e
        self.steps.append({"step": label, "reply": _norm(reply), "calls": self.ctx.log[n0:]})
        return reply

    def ex(self, *cmd):
        return self.do(" ".join(map(repr, cmd)), self.cl.execute_command, *cmd)

    def table(self, label):
        k = self.cl.keys
        self.steps.append({"step": label, "kind": _norm(k.kind), "fid": _norm(k.fid), "slot": _norm(k.slot),
                           "cid": _norm(k.cid), "day_keys": _norm(k.day_keys),
                           "slots_released": k.slots_released})


# command -> (a call on a key of its own kind, fewer arguments than it takes, more than it takes or None);
# {K} is the key.  Run on a missing key and on keys of the two other kinds as well.
_COMMANDS = [
    ("bf", ("BF.RESERVE", "{K}", 0.01, 1000), ("BF.RESERVE", "{K}", 0.01), None),
    ("bf", ("BF.ADD", "{K}", "a"), ("BF.ADD", "{K}"), ("BF.ADD", "{K}", "a", "b")),
    ("bf", ("BF.MADD", "{K}", "a", 2, 3.5), ("BF.MADD", "{K}"), None),
    ("bf", ("BF.EXISTS", "{K}", "a"), ("BF.EXISTS", "{K}"), ("BF.EXISTS", "{K}", "a", "b")),
    ("bf", ("BF.MEXISTS", "{K}", "a", b"b"), ("BF.MEXISTS", "{K}"), None),
    ("bf", ("BF.INFO", "{K}"), ("BF.INFO",), ("BF.INFO", "{K}", "x")),
    ("bf", ("BF.SCANDUMP", "{K}", 0), ("BF.SCANDUMP", "{K}"), ("BF.SCANDUMP", "{K}", 0, 1)),
    ("bf", ("BF.SCANDUMP", "{K}", 5), None, None),
    ("bf", ("BF.LOADCHUNK", "{K}", 9, b"abcd"), ("BF.LOADCHUNK", "{K}", 9), ("BF.LOADCHUNK", "{K}", 9, b"x", 1)),
    ("bf", ("BF.LOADCHUNK", "{K}", 2, b"abcd"), None, None),
    ("bf", ("BF.LOADCHUNK", "{K}", 1, b"junk"), None, None),
    ("bf", ("BF.CARD", "{K}"), ("BF.CARD",), ("BF.CARD", "{K}", "x")),
    ("cms", ("CMS.INITBYDIM", "{K}", 100, 5), ("CMS.INITBYDIM", "{K}", 100), ("CMS.INITBYDIM", "{K}", 100, 5, 1)),
    ("cms", ("CMS.INITBYPROB", "{K}", 0.01, 0.01), ("CMS.INITBYPROB", "{K}", 0.01),
     ("CMS.INITBYPROB", "{K}", 0.01, 0.01, 1)),
    ("cms", ("CMS.INCRBY", "{K}", "a", 1, "b", "2"), ("CMS.INCRBY", "{K}", "a"), None),
    ("cms", ("CMS.INCRBY", "{K}", "a", 1, "b"), None, None),  # an even argument count
    ("cms", ("CMS.QUERY", "{K}", "a", "b"), ("CMS.QUERY", "{K}"), None),
    ("cms", ("CMS.MERGE", "{K}", 1, "{K}"), ("CMS.MERGE", "{K}", 1), None),
    ("cms", ("CMS.MERGE", "{K}", 2, "{K}", "{K}", "WEIGHTS", 3, -4), None, None),
    ("cms", ("CMS.MERGE", "{K}", 2, "{K}", "{K}", b"weights", 3), None, None),  # the wrong count of weights
    ("cms", ("CMS.MERGE", "{K}", 2, "{K}", "{K}", "WEIGHT", 3, 4), None, None),
    ("cms", ("CMS.MERGE", "{K}", 0, "{K}"), None, None),
    ("cms", ("CMS.MERGE", "{K}", 2, "{K}"), None, None),
    ("cms", ("CMS.INFO", "{K}"), ("CMS.INFO",), ("CMS.INFO", "{K}", "x")),
    ("hll", ("PFADD", "{K}", "a", "b"), ("PFADD",), None),
    ("hll", ("PFADD", "{K}"), None, None),
    ("hll", ("PFCOUNT", "{K}"), ("PFCOUNT",), None),
    ("hll", ("PFCOUNT", "{K}", "{K}2", "nokey"), None, None),
    ("hll", ("PFMERGE", "{K}", "{K}2"), ("PFMERGE",), None),
    ("hll", ("PFMERGE", "{K}3"), None, None),
    ("hll", ("GET", "{K}"), ("GET",), ("GET", "{K}", "x")),
    ("hll", ("SET", "{K}", "not an hll string"), ("SET", "{K}"), ("SET", "{K}", "a", "b")),
    ("any", ("EXISTS", "{K}", "{K}", "nokey"), ("EXISTS",), None),
    ("any", ("TYPE", "{K}"), ("TYPE",), ("TYPE", "{K}", "x")),
]


def _fill(cmd, key):
    return tuple(a.replace("{K}", key) if isinstance(a, str) else a for a in cmd)


def _link():
    return dict(entries=100, bytes=128, bits=1024, size=0, error=0.01, bpe=9.585, hashes=7)


def _commands(pkg, steps):
    """Every command execute_command knows: on a key of its own kind, on a
    missing key, on keys of the other kinds, with too few and too many
    arguments.  A fresh client per command, so none depends on another."""
    for kind, own, few, many in _COMMANDS:
        for case in ("own", "missing", "other-a", "other-b"):
            r = _Recorder(pkg)
            r.ex("BF.RESERVE", "bf", 0.01, 100)
            r.ex("CMS.INITBYDIM", "cms", 10, 2)
            r.ex("PFADD", "hll", "x")
            r.ex("PFADD", "hll2", "y")
            others = [k for k in ("bf", "cms", "hll") if k != kind]
            key = {"own": kind if kind != "any" else "bf", "missing": "nokey", "other-a": others[0],
                   "other-b": others[1]}[case]
            r.steps.clear()
            r.ex(*_fill(own, key))
            r.table("table")
            steps.append({"case": f"{own[0]} / {case}", "steps": r.steps})
        r = _Recorder(pkg)
        for cmd in (few, many):
            if cmd is not None:
                r.ex(*_fill(cmd, "k"))
        steps.append({"case": f"{own[0]} / arity", "steps": r.steps})


def _reserve_and_generic(pkg, steps):
    r = _Recorder(pkg)
    for cmd in (("BF.RESERVE", "k", 0, 100), ("BF.RESERVE", "k", 1, 100), ("BF.RESERVE", "k", -0.5, 100),
                ("BF.RESERVE", "k", "rate", 100), ("BF.RESERVE", "k", 0.01, "cap"), ("BF.RESERVE", "k", 0.01, 0),
                ("BF.RESERVE", "k", None, 100), ("BF.RESERVE", "k", 0.01, 100, "EXPANSION", 0),
                ("BF.RESERVE", "k", 0.01, 100, "EXPANSION"), ("BF.RESERVE", "k", 0.01, 100, "BOGUS"),
                ("BF.RESERVE", "k0", 0.01, 100, "expansion", 0, b"nonscaling"),
                ("BF.RESERVE", "k1", "0.001", "5000", "EXPANSION", "4"),
                ("BF.RESERVE", "k2", 0.01, 100, "NONSCALING"), ("bf.reserve", b"k3", 0.5, 7),
                ("BF.RESERVE", "k3", 0.5, 7), (b"Type", "k3"), ("TYPE", b"k2"),
                ("SET", "k1", "junk"), ("SET", "h", "junk"), ("GET", "k1"), ("GET", "nokey"),
                ("PFADD", "h", 1), ("GET", "h"), ("CMS.INITBYPROB", "c", 0.01, 0.01), ("GET", "c"), ("TYPE", "c"),
                ("TYPE", "h"), ("TYPE", "nokey"), ("EXISTS", "k1", "c", "h", "h", "nokey"),
                ("UNLINK", "k1", "nokey"), ("DEL", "c", "h", "k0"), ("PING",), ("PING", "extra"), ("NOSUCH", "k"),
                (), ("FLUSHDB", "ASYNC"), ("EXISTS", "k2", "k3")):
        r.ex(*cmd)
    r.table("table after FLUSHDB")
    # SET of a valid HLL string: over nothing, over an HLL key, over keys of the other kinds
    hyll = pkg.formats.encode_hll(np.zeros(16384, np.uint8))
    r.ex("BF.ADD", "b", "x")
    r.ex("CMS.INITBYDIM", "c", 4, 2)
    for key in ("fresh", "fresh", "b", "c"):
        r.ex("SET", key, hyll)
    r.table("table after SET")
    r.ex("PFADD", "hll:unique:L1:2025-03-19", "a")
    r.ex("FLUSHALL")
    r.table("table after FLUSHALL")
    steps.append({"case": "BF.RESERVE options, generic keys, SET / GET, FLUSHALL", "steps": r.steps})
    # replies as bytes
    r = _Recorder(pkg, decode_responses=False)
    for cmd in (("BF.RESERVE", "b", 0.01, 100), ("BF.INFO", "b"), ("CMS.INITBYDIM", "c", 4, 2), ("CMS.INFO", "c"),
                ("PFADD", "h", "a"), ("TYPE", "b"), ("TYPE", "c"), ("TYPE", "h"), ("TYPE", "x"), ("PING",),
                ("PFMERGE", "h2", "h"), ("SET", "h3", pkg.formats.encode_hll(np.zeros(16384, np.uint8))),
                ("BF.LOADCHUNK", "b", 9, b"abcd"), ("FLUSHALL",)):
        r.ex(*cmd)
    r.do("scan_iter()", r.cl.scan_iter)
    r.do("day_keys('x')", r.cl.day_keys, "x")
    steps.append({"case": "decode_responses=False", "steps": r.steps})


def _surfaces(pkg, steps):
    r = _Recorder(pkg)
    bf, cms = r.cl.bf(), r.cl.cms()
    r.do("bf().reserve", bf.reserve, "b", 0.01, 100)
    r.do("bf().reserve again", bf.reserve, "b", 0.01, 100)
    r.do("bf().create expansion", bf.create, "b2", 0.01, 100, expansion=4)
    r.do("bf().reserve noScale", bf.reserve, "b3", 0.01, 100, noScale=True)
    r.do("bf().reserve expansion 0 noScale", bf.reserve, "b4", 0.01, 100, 0, True)
    r.do("bf().reserve expansion 0", bf.reserve, "b5", 0.01, 100, 0)
    r.do("bf().add", bf.add, "b", "a")
    r.do("bf().madd", bf.madd, "b", "a", "b")
    r.do("bf().exists", bf.exists, "b", "a")
    r.do("bf().mexists", bf.mexists, "b", "a", "b")
    info = r.do("bf().info", bf.info, "b")
    r.do("bf().info.get / []", lambda: [info.get("capacity"), info["insertedNum"], info.expansionRate])
    r.do("bf().info missing", bf.info, "nokey")
    r.do("bf().card", bf.card, "b")
    r.do("bf().card missing", bf.card, "nokey")
    r.do("cms().initbydim", cms.initbydim, "c", 10, 2)
    r.do("cms().initbyprob", cms.initbyprob, "c2", 0.01, 0.01)
    r.do("cms().incrby", cms.incrby, "c", ["a", "b"], [1, 2])
    r.do("cms().incrby uneven", cms.incrby, "c", ["a", "b"], [1])
    r.do("cms().query", cms.query, "c", "a", "b")
    r.do("cms().merge", cms.merge, "c", 2, ["c", "c2"])
    r.do("cms().merge weights", cms.merge, "c", 2, ["c", "c2"], [1, 2])
    r.do("cms().merge wrong weights", cms.merge, "c", 2, ["c", "c2"], [1])
    r.do("cms().merge wrong type", cms.merge, "c", 1, ["b"])
    cinfo = r.do("cms().info", cms.info, "c")
    r.do("cms().info.get / []", lambda: [cinfo.get("width"), cinfo["depth"], cinfo.count])
    r.do("bf_links", r.cl.bf_links, "b")
    r.do("bf_link_bits missing", r.cl.bf_link_bits, "nokey", 0)
    r.do("bf_scandump", r.cl.bf_scandump, "b", 0)
    r.do("bf_loadchunk header", r.cl.bf_loadchunk, "loaded", 1,
         pkg.formats.bf_dump_header(3, [_link()], 2, False))
    r.do("bf_loadchunk header on a key", r.cl.bf_loadchunk, "c", 1,
         pkg.formats.bf_dump_header(3, [_link()], 2, False))
    r.do("bf_loadchunk header without links", r.cl.bf_loadchunk, "loaded2", 1,
         pkg.formats.bf_dump_header(3, [], 2, True))
    r.do("cms_add_packed", r.cl.cms_add_packed, "c", *pkg.pack(["a", "b", "c"]), None, [1, 0, 1], 0)
    r.do("cms_add_packed increments", r.cl.cms_add_packed, "c", *pkg.pack(["a", "b"]), [5, 6])
    r.do("cms_add_packed bad mask", r.cl.cms_add_packed, "c", *pkg.pack(["a", "b"]), None, [1])
    r.do("cms_query_packed", r.cl.cms_query_packed, "c", *pkg.pack(["a"]))
    r.do("cms_table", r.cl.cms_table, "c")
    r.do("MAX_SCANDUMP_SIZE", lambda: r.cl.MAX_SCANDUMP_SIZE)
    r.table("table")
    steps.append({"case": "bf() and cms() on the client", "steps": r.steps})

    r = _Recorder(pkg)
    p = r.cl.pipeline()
    r.do("pipeline bf().reserve", lambda: p.bf().reserve("b", 0.01, 100) is p)
    r.do("pipeline bf().create expansion noScale", lambda: p.bf().create("b2", 0.01, 100, expansion=4,
                                                                          noScale=True) is p)
    r.do("pipeline bf().add", lambda: p.bf().add("b", "a") is p)
    r.do("pipeline bf().madd", lambda: p.bf().madd("b", "a", "b") is p)
    r.do("pipeline bf().exists", lambda: p.bf().exists("b", "a") is p)
    r.do("pipeline bf().mexists", lambda: p.bf().mexists("b", "a", "b") is p)
    r.do("pipeline pfadd / pfcount / pfmerge", lambda: p.pfadd("h", "a").pfcount("h").pfmerge("d", "h") is p)
    r.do("len(pipeline)", len, p)
    r.do("pipeline queue", lambda: list(p._cmds))
    r.do("pipeline execute", p.execute)
    r.do("len(pipeline) after", len, p)
    r.table("table")
    with r.cl.pipeline() as q:
        q.pfadd("h", "z")
        r.do("pipeline raises", q.execute_command("BF.INFO", "nokey").execute)
    steps.append({"case": "bf() on a pipeline", "steps": r.steps})


def _pipeline(pkg, steps):
    r = _Recorder(pkg)
    p = r.cl.pipeline()
    p.pfadd("h1", "a", "b").pfadd("h2", "c").execute_command(b"pfadd", "h1").pfadd("h2", "d", "e")
    p.pfcount("h1", "h2")
    p.bf().add("b", "x")
    p.bf().madd("b", "y", "z")
    p.execute_command("bf.add", b"b", "w")
    p.bf().add("b2", "x")  # another key: a run of its own
    p.bf().exists("b", "x")
    p.bf().mexists("b", "x", "y")
    p.execute_command("BF.EXISTS", "b", "x", "y")  # mis-arity: the whole run answers the error
    p.bf().exists("b2", "x")
    p.pfadd("h1", "f")
    p.pfcount("h1")
    p.pfadd("b", "f")  # WRONGTYPE inside a run of PFADDs
    p.pfadd("h3", "g")
    p.execute_command("PFADD")  # no key: not batched
    p.execute_command("BF.ADD", "b")  # too short: not batched
    p.execute_command("BF.EXISTS", "h1", "x")
    p.execute_command("BF.MADD", "h1", "x")
    p.execute_command("CMS.INITBYDIM", "c", 4, 2).execute_command("CMS.INCRBY", "c", "a", 1)
    p.execute_command("TYPE", "h3").execute_command("NOSUCH")
    r.do("execute(raise_on_error=False)", p.execute, raise_on_error=False)
    r.table("table")
    steps.append({"case": "pipeline runs", "steps": r.steps})


def _rollbacks(pkg, steps):
    for cmd, failing, again in (
            (("BF.RESERVE", "k", 0.01, 100), "ske_bf_reserve", ("BF.RESERVE", "k2", 0.01, 100)),
            (("CMS.INITBYDIM", "k", 10, 2), "ske_cms_init", ("CMS.INITBYDIM", "k2", 10, 2)),
            (("BF.LOADCHUNK", "k", 1, pkg.formats.bf_dump_header(3, [_link()], 2, False)), "ske_bf_load_header",
             ("BF.RESERVE", "k2", 0.01, 100))):
        r = _Recorder(pkg)
        r.ex("BF.ADD", "first", "a")          # fid 0 is taken: the id that comes back is not the first
        if failing != "ske_cms_init":
            r.ex("CMS.INITBYDIM", "firstc", 4, 2)
        r.ctx.fail[failing] = (-2, "ERR out of device memory (stub)")
        r.ex(*cmd)
        r.ex("TYPE", "k")
        r.table("table after the failure")
        r.ctx.fail.clear()
        r.ex(*again)
        r.table("table after the next create")
        steps.append({"case": f"rollback: {failing} fails", "steps": r.steps})
    # BF.ADD's own create failing leaves what it leaves (pinned as it is)
    r = _Recorder(pkg, fail={"ske_bf_reserve": (-2, "ERR out of device memory (stub)")})
    r.ex("BF.ADD", "k", "a")
    r.table("table")
    steps.append({"case": "BF.ADD: ske_bf_reserve fails", "steps": r.steps})


def _key_table(pkg, steps):
    r = _Recorder(pkg)
    k = r.cl.keys
    r.ex("PFADD", "h0", "a")
    r.do("bind fresh slot beyond _next_slot", k.bind, b"far", 5)
    r.do("bind same slot again", k.bind, b"far", 5)
    r.do("bind another slot", k.bind, b"far", 6)
    r.do("bind a slot another key holds", k.bind, b"other", 5)
    r.do("bind a skipped slot", k.bind, b"near", 3)
    r.ex("BF.ADD", "b", "a")
    r.do("bind a Bloom key", k.bind, b"b", 7)
    r.do("key_slot(create=False) missing", r.cl.key_slot, "nokey", create=False)
    r.do("key_slot existing", r.cl.key_slot, "far")
    r.do("key_slot create", r.cl.key_slot, "made")
    r.do("key_slot wrong type", r.cl.key_slot, "b")
    r.do("type_of / expect", lambda: [k.type_of(b"far"), k.type_of(b"nokey"), k.expect(b"far", "hll"),
                                      k.expect(b"nokey", "bf")])
    r.do("expect wrong type", k.expect, b"b", "cms")
    r.table("table after binds")
    for name in ("hll:unique:L1:2025-03-19", "hll:unique:L1:2025-03-20", "hll:unique:L10:2025-03-19",
                 "hll:unique:L1", "hll:unique:L1:2025-3-19", "hll:unique:L1:2025-03-19x", ":2025-03-19",
                 "hll:unique:A:B:2025-01-01"):
        r.ex("PFADD", name, "a")
    r.ex("BF.ADD", "bf:L1:2025-03-19", "a")
    r.ex("CMS.INITBYDIM", "cms:L1:2025-03-19", 4, 2)

    def scans():
        r.do("day_keys L1", r.cl.day_keys, "hll:unique:L1")
        r.do("day_keys L10", r.cl.day_keys, b"hll:unique:L10")
        r.do("day_keys A", r.cl.day_keys, "hll:unique:A")
        r.do("day_keys bf", r.cl.day_keys, "bf:L1")
        r.do("scan_iter()", r.cl.scan_iter)
        r.do("scan_iter(match)", r.cl.scan_iter, match="hll:unique:L1:*")
        r.do("scan_iter(match class)", r.cl.scan_iter, match="*:2025-03-[12][0-9]", count=10)
        for t in ("string", "MBbloom--", "CMSk-TYPE", "hll", "bf", "cms", "hash"):
            r.do(f"scan_iter(_type={t})", r.cl.scan_iter, _type=t)
        r.do("scan_iter(match, _type)", r.cl.scan_iter, match="*L1:*", _type="string")

    scans()
    r.do("slots_released", lambda: k.slots_released)
    r.ex("DEL", "hll:unique:L1:2025-03-19", "hll:unique:L10:2025-03-19", "bf:L1:2025-03-19", "nokey")
    r.do("slots_released after DEL", lambda: k.slots_released)
    scans()
    r.ex("PFADD", "reuse", "a")  # takes a freed slot
    r.table("table after DEL")
    # swipes: with the stub no swipe is valid, so a tentative key is released again
    r.do("swipes one key", r.cl.swipes, "b", "hll:unique:S:2025-03-19", ["1", "2", "3"])
    r.do("slots_released after swipes", lambda: k.slots_released)
    r.do("swipes key per item", r.cl.swipes, "b", ["s1", "far", "s1"], [1, 2, 3])
    r.do("swipes without filter", r.cl.swipes, "nokey", ["s1", "s2"], [1, 2])
    r.do("swipes packed, empty", r.cl.swipes, "b", "s1", packed=pkg.pack([]))
    r.do("swipes wrong key count", r.cl.swipes, "b", ["s1"], [1, 2])
    r.do("swipes wrong hll type", r.cl.swipes, "b", "b", [1])
    r.do("swipes wrong bf type", r.cl.swipes, "far", "s1", [1])
    r.do("slots_released after all swipes", lambda: k.slots_released)
    slots = np.asarray([5, 5], np.uint32)
    r.do("swipes_slots", r.cl.swipes_slots, "b", slots, *pkg.pack([1, 2]))
    r.do("swipes_slots missing filter", r.cl.swipes_slots, "nokey", slots, *pkg.pack([1, 2]))
    r.do("swipes_fixed", r.cl.swipes_fixed, "b", slots, np.zeros((2, 8), np.uint8))
    r.do("swipes_fixed bad slots", r.cl.swipes_fixed, "b", slots[:1], np.zeros((2, 8), np.uint8))
    r.do("swipes_fixed bad ids", r.cl.swipes_fixed, "b", slots, np.zeros(8, np.uint8))
    r.do("release_unused_slot", lambda: (r.cl.key_slot("tmp"), k.release_unused_slot(b"tmp"), k.slots_released))
    r.do("drop", lambda: [k.drop(b"far"), k.drop(b"far")])
    r.table("final table")
    steps.append({"case": "key table", "steps": r.steps})


def _hll(pkg, steps):
    r = _Recorder(pkg)
    cl = r.cl
    r.do("pfadd_calls", cl.pfadd_calls, [("h1", "a"), ("h2",), ("h1", "b", "c"), ("h3", 1)])
    r.do("pfadd", cl.pfadd, "h1", "a")
    r.do("pfadd_packed", cl.pfadd_packed, [0, 1], *pkg.pack(["a", "b"]), changed=True)
    r.do("pfadd_packed no replies", cl.pfadd_packed, [0, 1], *pkg.pack(["a", "b"]))
    r.do("pfcount none", cl.pfcount)
    r.do("pfcount missing", cl.pfcount, "nokey")
    r.do("pfcount", cl.pfcount, "h1", "h2")
    r.do("pfcount_each", cl.pfcount_each, ["h1", "nokey", "h3"])
    r.do("pfcount_each missing only", cl.pfcount_each, ["nokey"])
    r.do("pfcount_groups", cl.pfcount_groups, [["h1", "h2"], ["nokey"], []])
    r.do("pfcount_groups empty", cl.pfcount_groups, [])
    r.do("pfmerge", cl.pfmerge, "d", "h1", "nokey", "h2")
    r.do("hll_registers missing", lambda: int(cl.hll_registers("nokey").sum()))
    r.do("hll_registers", lambda: int(cl.hll_registers("h1").sum()))
    r.do("hll_dense", lambda: len(cl.hll_dense("h1")))
    r.do("hll_dense missing", cl.hll_dense, "nokey")
    r.do("hll_load_registers", cl.hll_load_registers, "loaded", np.zeros(16384, np.uint8))
    r.do("hll_load_registers short", cl.hll_load_registers, "loaded2", np.zeros(5, np.uint8))
    r.do("dump_hll", cl.dump_hll, "h1")
    r.do("dump_hll missing", cl.dump_hll, "nokey")
    r.do("load_hll", cl.load_hll, "h9", pkg.formats.encode_hll(np.zeros(16384, np.uint8)))
    r.table("table")
    steps.append({"case": "HLL calls", "steps": r.steps})


def _ingest(pkg, steps):
    """The device ingest's call order.  With the stub as it is every message
    decodes "on the device" and hits the key table; hooks on the device-to-host
    copies send all of them through the host path, or make all of them miss the
    key table (one first-seen key, which no valid swipe reaches)."""
    msgs = [b'{"student_id": 1, "timestamp": "2025-03-19T10:00:00", "lecture_id": "L1"}',
            b'{"student_id": 2, "timestamp": "2025-03-19T23:30:00-05:00", "lecture_id": "L2"}',
            b'not json', b'{"student_id": 3, "timestamp": "2025-03-19T10:00:00"}']
    r = _Recorder(pkg)
    r.ex("BF.ADD", "b", "1")
    r.do("ingest", r.cl.ingest, "b", msgs)
    r.do("ingest again", r.cl.ingest, "b", msgs)
    r.do("ingest code form", r.cl.ingest, "b", msgs, "p:", "code")
    r.do("ingest empty", r.cl.ingest, "b", [])
    r.do("ingest str payloads, no filter", r.cl.ingest, "nokey", [m.decode() for m in msgs])
    r.ex("PFADD", "h", "a")
    r.ex("DEL", "h")
    r.do("ingest after a slot was released", r.cl.ingest, "b", msgs)
    r.ctx.hooks["ske_memcpy"] = lambda dst, src, nbytes, to_host: to_host and C.memset(dst, 1, nbytes)
    r.do("ingest, host path", r.cl.ingest, "b", msgs)
    r.do("ingest, host path, code form", r.cl.ingest, "b", msgs, "p:", "code")
    r.ex("BF.ADD", "xL1", "a")
    r.do("ingest, host path, wrong type", r.cl.ingest, "b", msgs, "x", "code")
    n = len(msgs)
    r.ctx.hooks["ske_memcpy"] = lambda dst, src, nbytes, to_host: to_host and nbytes == 4 * n and C.memset(
        dst, 0xFF, nbytes)  # the slot column: no key found
    r.ctx.hooks["ske_keytab_lookup"] = lambda cols, n, slots, nmiss: nmiss and setattr(nmiss._obj, "value", n)
    r.do("ingest, first-seen key", r.cl.ingest, "b", msgs)
    r.do("slots_released", lambda: r.cl.keys.slots_released)
    r.ex("PFADD", "L1", "a")
    r.do("ingest, first-seen key that exists", r.cl.ingest, "b", msgs, "", "code")
    r.do("ingest, first-seen key of another kind", r.cl.ingest, "b", msgs, "x", "code")
    r.ctx.hooks.clear()
    r.do("ingest more than the buffers hold", r.cl.ingest_packed, "b", np.zeros(8, np.uint8),
         np.zeros(2000, np.uint32))
    r.table("table")
    steps.append({"case": "ingest", "steps": r.steps})


def record(pkg) -> list:
    steps: list = []
    for part in (_commands, _reserve_and_generic, _surfaces, _pipeline, _rollbacks, _key_table, _hll, _ingest):
        part(pkg, steps)
    return json.loads(json.dumps(steps))  # tuples as lists, as the file holds them


def test_facade_transcript(pkg):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = record(pkg)
    assert [c["case"] for c in got] == [c["case"] for c in want]
    for g, w in zip(got, want):
        assert [s["step"] for s in g["steps"]] == [s["step"] for s in w["steps"]], g["case"]
        for gs, ws in zip(g["steps"], w["steps"]):
            assert gs == ws, f"{g['case']}: {gs['step']}"


def test_bf_loadchunk_header_n2(pkg):
    """A link's n2 (last byte of its header record) makes RedisBloom probe mod
    2^n2; the device probes mod bits.  A header whose n2 is not log2(bits) is
    "ERR received bad data": no native call, no key left behind.  n2 == log2(bits)
    (here 1024 bits, n2 = 10) loads as ever."""
    def hdr(n2):
        return pkg.formats.bf_dump_header(3, [_link()], 2, False)[:-1] + bytes([n2])

    for bad in (9, 11, 64, 255):
        r = _Recorder(pkg)
        e = r.do("bad n2", r.cl.bf_loadchunk, "k", 1, hdr(bad))
        assert type(e).__name__ == "ResponseError" and str(e) == "ERR received bad data"
        assert r.steps[-1]["calls"] == []
        assert r.ex("TYPE", "k") == "none" and r.cl.keys.fid == {}
    r = _Recorder(pkg)
    assert r.do("n2 = log2(bits)", r.cl.bf_loadchunk, "k", 1, hdr(10)) is True
    assert [c[0] for c in r.steps[-1]["calls"]] == ["ske_bf_load_header"]
    assert r.ex("TYPE", "k") == "MBbloom--"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: test_facade_transcript.py --write   (re-records the expectation)")
    with open(GOLDEN, "w") as f:
        json.dump(record(ge.load_package()), f, indent=0, sort_keys=True)
        f.write("\n")
