"""SketchClient -- the redis-py call surface of the reference's hot path,
executed on MI355X through libsketch.

The reference builds one ``redis.Redis(host, port, decode_responses=True)``
client per process (attendance_processor.py:37-41, data_generator.py:45-49)
and uses exactly these calls on the validate-and-count path:

=====================================================  ====================================
reference call (file:line)                             here
=====================================================  ====================================
``execute_command('BF.EXISTS', key, id)`` (ap.py:109)  ``execute_command`` -> ske_bf_mexists
``execute_command('BF.RESERVE', key, err, cap)`` (:83) ``execute_command`` -> ske_bf_reserve
``execute_command('BF.ADD', key, id)`` (dg.py:59)      ``execute_command`` -> ske_bf_madd
``pfadd(hll_key, student_id)`` (ap.py:129)             ``pfadd`` -> ske_hll_pfadd
``pfcount(hll_key)`` (ap.py:152)                       ``pfcount`` -> ske_hll_pfcount
=====================================================  ====================================

plus the north-star surface: ``bf().reserve/add/madd/exists/mexists/info``,
``pfmerge``, ``pipeline()`` and the batched ``swipes()`` (the fused K1 kernel:
BF.EXISTS then valid-gated PFADD for a whole batch of events).

Per-student counters (attendance_analysis.py:99-118, there pandas over
Cassandra rows) are RedisBloom Count-Min Sketch keys: the six ``CMS.*``
commands, ``cms()`` with redis-py's surface and the bulk ``cms_add_packed``.

Semantics kept from Redis / RedisBloom / redis-py:
  * argument encoding as redis-py (``encoding.encode``);
  * ``BF.EXISTS``/``BF.MEXISTS`` on a missing key answer 0 (so the
    reference's probe at attendance_processor.py:78 never raises and its
    ``BF.RESERVE`` branch never runs -- reproduced, not "fixed");
  * ``BF.ADD``/``BF.MADD`` auto-create a chain (error 0.01, capacity 100,
    expansion 2); ``BF.RESERVE`` on an existing key -> ``ERR item exists``;
  * ``PFADD key`` with no elements creates the key and replies 1;
    ``PFCOUNT`` of missing keys -> 0; keys of the other type -> WRONGTYPE.

The client is composed per native unit (csrc/sketch_api_*.cpp): the key table
(keyspace.py), Bloom (client_bloom.py), Count-Min Sketch (client_cms.py),
heavy-hitter sets beside a CMS key (client_hh.py), HLL (client_hll.py), the
fused swipe path (client_swipes.py), the device ingest (client_ingest.py),
the time profiles (client_tp.py), the tallies (client_tally.py), the
seen-row sets (client_seen.py) and the row logs (client_rows.py);
commands.py holds the command table, ``bf()`` / ``cms()`` and the pipeline.  Here: the constructor, the generic key commands and
``execute_command``.
"""
from __future__ import annotations

from ._lib import Context
from .client_bloom import BloomMixin
from .client_cms import CmsMixin
from .client_hh import HhMixin
from .client_hll import HllMixin
from .client_ingest import IngestMixin
from .client_rows import RowsMixin
from .client_seen import SeenMixin
from .client_swipes import SwipesMixin
from .client_tally import TallyMixin
from .client_tp import TimeProfileMixin
from .commands import (BFInfo, BloomCommands, CMSCommands, CMSInfo, COMMANDS, Pipeline,  # noqa: F401
                       arity_error, text)
from .encoding import encode
from .exceptions import ResponseError
from .keyspace import (BF_TYPE_NAME, CMS_TYPE_NAME, KIND_TYPE_NAMES, TYPE_NAME_KINDS,  # noqa: F401
                       KeySpace, redis_glob)


class SketchClient(BloomMixin, CmsMixin, HhMixin, HllMixin, SwipesMixin, IngestMixin, TimeProfileMixin,
                   TallyMixin, SeenMixin, RowsMixin):
    """Drop-in for ``redis.Redis`` on the reference's Bloom + HLL calls."""

    def __init__(self, host: str = "localhost", port: int = 6379, db: int = 0,
                 decode_responses: bool = False, device: int = 0,
                 context: Context | None = None, **_ignored):
        self.ctx = context if context is not None else Context(device)
        self.decode_responses = decode_responses
        self.keys = KeySpace(self.ctx)
        self.host, self.port, self.db = host, port, db
        self._ingest = None  # client_ingest.IngestState, made by the first ingest
        self._hh_init_registry()
        self._tp_init_registry()
        self._tally_init_registry()
        self._seen_init_registry()
        self._rows_init_registry()

    # ------------------------------------------------------------ helpers
    def _ok(self):
        return "OK" if self.decode_responses else b"OK"

    def _s(self, text: str):
        return text if self.decode_responses else text.encode()

    def _flat(self, info: dict) -> list:
        """An info reply as Redis sends it: [name, value, name, value, ...]."""
        return [x for k, v in info.items() for x in (self._s(k), v)]

    def close(self) -> None:
        pass  # the device context lives as long as the client object

    def ping(self) -> bool:
        return True

    # ------------------------------------------------------------ generic keys
    def delete(self, *names) -> int:
        if self._hh:  # heavy-hitter sets go with the CMS key they read
            for n in names:
                self._hh_release(encode(n))
        return sum(self.keys.drop(encode(n)) for n in names)

    def exists(self, *names) -> int:
        return sum(encode(n) in self.keys.kind for n in names)

    def scan_iter(self, match=None, count=None, _type=None):
        """SCAN over the key table, redis-py's iterator form (one pass, sorted;
        MATCH in Redis' own glob dialect, ``redis_glob``).  (redis-py's
        ``keys()`` is not offered: ``self.keys`` is the key table.)"""
        pat = encode(match if match is not None else "*")
        every = pat == b"*"  # SCAN's own bypass (the glob rule alone would skip an empty key name)
        for k in sorted(self.keys.kind):
            if (every or redis_glob(pat, k)) and (
                    _type is None or self.keys.kind[k] == TYPE_NAME_KINDS.get(_type, _type)):
                yield k.decode() if self.decode_responses else k

    def day_keys(self, stem) -> list:
        """The README-form day keys <stem>:YYYY-MM-DD that exist (sorted),
        from the key table's index -- no scan over every key."""
        ks = sorted(self.keys.day_keys.get(encode(stem), ()))
        return [k.decode() for k in ks] if self.decode_responses else ks

    def type(self, name):
        return self._s(KIND_TYPE_NAMES.get(self.keys.type_of(encode(name)), "none"))

    def flushall(self, *_a, **_k) -> bool:
        if self._hh:
            self._hh_release(None)
        if self._tp:
            self._tp_release()
        if self._tally:
            self._tally_release()
        if self._seen:
            self._seen_release()
        if self._rows:
            self._rows_release()
        for key in list(self.keys.kind):
            self.keys.drop(key)
        return True

    flushdb = flushall

    # ------------------------------------------------------------ commands
    def execute_command(self, *args, **options):
        if not args:
            raise ResponseError("ERR empty command")
        name = text(args[0])
        if name.upper() not in COMMANDS:
            raise ResponseError(f"ERR unknown command '{name}'")
        lo, hi, handler = COMMANDS[name.upper()]  # fewest / most arguments (None: unbounded)
        a = args[1:]
        if len(a) < lo or (hi is not None and len(a) > hi):
            raise arity_error(name)
        return handler(self, a)

    def pipeline(self, transaction: bool = True, shard_hint=None) -> Pipeline:
        return Pipeline(self)

    def bf(self) -> BloomCommands:
        return BloomCommands(self)

    def cms(self) -> CMSCommands:
        return CMSCommands(self)


Redis = SketchClient  # redis.Redis(host=..., port=..., decode_responses=True) drop-in
