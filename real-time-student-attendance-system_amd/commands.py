"""The command surface over a ``SketchClient``: the table ``execute_command``
looks a command up in, redis-py's ``bf()`` / ``cms()`` objects with their info
classes, and the pipeline."""
from __future__ import annotations

from .encoding import encode, pack
from .exceptions import ResponseError, WRONGTYPE
from .keyspace import KIND_TYPE_NAMES


def text(word) -> str:
    return word.decode() if isinstance(word, bytes) else str(word)


def token(word) -> str:
    """A command name or an option word as upper-case text (Redis compares
    both without regard to case)."""
    return text(word).upper()


def arity_error(name: str) -> ResponseError:
    return ResponseError(f"ERR wrong number of arguments for '{name.lower()}' command")


def _get(c, a):
    k = encode(a[0])
    if KIND_TYPE_NAMES.get(c.keys.type_of(k), "string") != "string":
        raise ResponseError(WRONGTYPE)
    return c.dump_hll(k)


def _mget(c, a):
    """GET's rule per key, over the bulk dump; a missing or non-string key
    answers None, as Redis' MGET does."""
    keys = [encode(k) for k in a]
    hll = [k for k in keys if c.keys.type_of(k) == "hll"]
    got = dict(zip(hll, c.dump_hlls(hll)))
    return [got.get(k) for k in keys]


def _mset(c, a):
    if len(a) % 2:
        raise arity_error("mset")
    c.load_hlls([(a[i], encode(a[i + 1])) for i in range(0, len(a), 2)])


def _then_ok(method):
    """A command whose facade method replies True (or nothing) and Redis OK."""
    def handler(c, a):
        method(c, a)
        return c._ok()
    return handler


# NAME -> (fewest arguments, most arguments or None, handler(client, arguments)).
# The handlers that are more than a call are the ``_cmd_*`` methods of the
# subsystem they belong to (client_bloom.py, client_cms.py).
COMMANDS = {
    "BF.RESERVE": (3, None, lambda c, a: c._cmd_bf_reserve(a)),
    "BF.ADD": (2, 2, lambda c, a: c._cmd_bf_add(a)),
    "BF.MADD": (2, None, lambda c, a: c._bf_madd_reply(encode(a[0]), a[1:])),
    "BF.EXISTS": (2, 2, lambda c, a: c._cmd_bf_mexists(a)[0]),
    "BF.MEXISTS": (2, None, lambda c, a: c._cmd_bf_mexists(a)),
    "BF.INFO": (1, 1, lambda c, a: c._flat(c.bf_info(a[0]))),
    "BF.SCANDUMP": (2, 2, lambda c, a: list(c.bf_scandump(a[0], a[1]))),
    "BF.LOADCHUNK": (3, 3, _then_ok(lambda c, a: c.bf_loadchunk(a[0], a[1], a[2]))),
    "BF.CARD": (1, 1, lambda c, a: c._cmd_bf_card(a)),
    "CMS.INITBYDIM": (3, 3, lambda c, a: c.cms_initbydim(a[0], a[1], a[2])),
    "CMS.INITBYPROB": (3, 3, lambda c, a: c.cms_initbyprob(a[0], a[1], a[2])),
    "CMS.INCRBY": (3, None, lambda c, a: c._cmd_cms_incrby(a)),
    "CMS.QUERY": (2, None, lambda c, a: c.cms_query(a[0], *a[1:])),
    "CMS.MERGE": (3, None, lambda c, a: c._cmd_cms_merge(a)),
    "CMS.INFO": (1, 1, lambda c, a: c._flat(c.cms_info(a[0]))),
    "PFADD": (1, None, lambda c, a: c.pfadd(*a)),
    "PFCOUNT": (1, None, lambda c, a: c.pfcount(*a)),
    "PFMERGE": (1, None, _then_ok(lambda c, a: c.pfmerge(*a))),
    "GET": (1, 1, _get),
    "SET": (2, 2, _then_ok(lambda c, a: c.load_hll(a[0], encode(a[1])))),
    "MGET": (1, None, _mget),
    "MSET": (2, None, _then_ok(_mset)),
    "DEL": (1, None, lambda c, a: c.delete(*a)),
    "EXISTS": (1, None, lambda c, a: c.exists(*a)),
    "TYPE": (1, 1, lambda c, a: c.type(a[0])),
    "FLUSHALL": (0, None, _then_ok(lambda c, a: c.flushall())),
    "PING": (0, None, lambda c, a: c._s("PONG")),
}
COMMANDS["UNLINK"] = COMMANDS["DEL"]
COMMANDS["FLUSHDB"] = COMMANDS["FLUSHALL"]


class BloomCommands:
    """``client.bf()`` surface of redis-py (redis.commands.bf.BFCommands), over
    a client or a pipeline: anything with ``execute_command``.  On a pipeline
    every command replies the pipeline."""

    def __init__(self, client):
        self.client = client

    def create(self, key, errorRate, capacity, expansion=None, noScale=None):
        args = ["BF.RESERVE", key, errorRate, capacity]
        if expansion is not None:
            args += ["EXPANSION", expansion]
        if noScale:
            args += ["NONSCALING"]
        reply = self.client.execute_command(*args)
        return reply if isinstance(reply, Pipeline) else True

    reserve = create

    def add(self, key, item):
        return self.client.execute_command("BF.ADD", key, item)

    def madd(self, key, *items):
        return self.client.execute_command("BF.MADD", key, *items)

    def exists(self, key, item):
        return self.client.execute_command("BF.EXISTS", key, item)

    def mexists(self, key, *items):
        return self.client.execute_command("BF.MEXISTS", key, *items)

    def info(self, key):
        return BFInfo(self.client.bf_info(key))

    def card(self, key):
        return self.client.execute_command("BF.CARD", key)


class CMSCommands:
    """``client.cms()`` surface of redis-py (redis.commands.bf.CMSCommands)."""

    def __init__(self, client):
        self.client = client

    def initbydim(self, key, width, depth):
        self.client.execute_command("CMS.INITBYDIM", key, width, depth)
        return True

    def initbyprob(self, key, error, probability):
        self.client.execute_command("CMS.INITBYPROB", key, error, probability)
        return True

    def incrby(self, key, items, increments):
        return self.client.cms_incrby(key, list(items), list(increments))

    def query(self, key, *items):
        return self.client.execute_command("CMS.QUERY", key, *items)

    def merge(self, destKey, numKeys, srcKeys, weights=[]):
        self.client.cms_merge(destKey, numKeys, list(srcKeys), list(weights))
        return True

    def info(self, key):
        return CMSInfo(self.client.cms_info(key))


class _Info:
    """redis.commands.bf.info: the fields as attributes, ``get`` and ``[]``."""

    def get(self, item):
        return getattr(self, item)

    __getitem__ = get


class CMSInfo(_Info):
    """redis.commands.bf.info.CMSInfo attribute names."""

    def __init__(self, d: dict):
        self.width = d["width"]
        self.depth = d["depth"]
        self.count = d["count"]


class BFInfo(_Info):
    """redis.commands.bf.info.BFInfo attribute names."""

    def __init__(self, d: dict):
        self.capacity = d["Capacity"]
        self.size = d["Size"]
        self.filterNum = d["Number of filters"]
        self.insertedNum = d["Number of items inserted"]
        self.expansionRate = d["Expansion rate"]


class Pipeline:
    """redis-py pipeline: commands are queued and executed on ``execute()``.

    Consecutive compatible commands run as ONE device batch with Redis's
    sequential replies: a run of PFADDs (any keys) becomes one exact-order
    ske_hll_pfadd; a run of BF.EXISTS/BF.MEXISTS on one key one
    ske_bf_mexists; a run of BF.ADD/BF.MADD on one key one ske_bf_madd."""

    def __init__(self, client):
        self.client = client
        self._cmds: list[tuple] = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.reset()

    def __len__(self):
        return len(self._cmds)

    def reset(self):
        self._cmds = []

    def execute_command(self, *args, **options):
        self._cmds.append(args)
        return self

    def pfadd(self, name, *values):
        return self.execute_command("PFADD", name, *values)

    def pfcount(self, *sources):
        return self.execute_command("PFCOUNT", *sources)

    def pfmerge(self, dest, *sources):
        return self.execute_command("PFMERGE", dest, *sources)

    def bf(self) -> BloomCommands:
        return BloomCommands(self)

    def execute(self, raise_on_error: bool = True) -> list:
        cmds, self._cmds = self._cmds, []
        out: list = []
        i = 0
        cl = self.client

        def run_end(i, family, min_len, key=None):
            """End of the run of `family` commands (on `key`) that starts at i."""
            j = i + 1
            while (j < len(cmds) and token(cmds[j][0]) in family and len(cmds[j]) >= min_len
                   and (key is None or encode(cmds[j][1]) == key)):
                j += 1
            return j

        while i < len(cmds):
            name = token(cmds[i][0])
            j = i + 1
            try:
                if name == "PFADD" and len(cmds[i]) >= 2:
                    j = run_end(i, ("PFADD",), 2)
                    out.extend(cl.pfadd_calls([c[1:] for c in cmds[i:j]]))
                elif name in ("BF.EXISTS", "BF.MEXISTS") and len(cmds[i]) >= 3:
                    key = encode(cmds[i][1])
                    j = run_end(i, ("BF.EXISTS", "BF.MEXISTS"), 3, key)
                    if any(token(c[0]) == "BF.EXISTS" and len(c) != 3 for c in cmds[i:j]):
                        raise arity_error("bf.exists")
                    items = [x for c in cmds[i:j] for x in c[2:]]
                    buf, offs = pack(items)
                    res = cl.bf_mexists_packed(key, buf, offs)
                    p = 0
                    for c in cmds[i:j]:
                        m = len(c) - 2
                        r = [int(x) for x in res[p:p + m]]
                        out.append(r[0] if token(c[0]) == "BF.EXISTS" else r)
                        p += m
                elif name in ("BF.ADD", "BF.MADD") and len(cmds[i]) >= 3:
                    key = encode(cmds[i][1])
                    j = run_end(i, ("BF.ADD", "BF.MADD"), 3, key)
                    items = [x for c in cmds[i:j] for x in c[2:]]
                    res = cl._bf_madd_reply(key, items)
                    p = 0
                    for c in cmds[i:j]:
                        m = len(c) - 2
                        out.append(res[p] if token(c[0]) == "BF.ADD" else res[p:p + m])
                        p += m
                else:
                    out.append(cl.execute_command(*cmds[i]))
            except ResponseError as e:
                out.extend([e] * (j - i))
            i = j
        if raise_on_error:
            for r in out:
                if isinstance(r, ResponseError):
                    raise r
        return out
