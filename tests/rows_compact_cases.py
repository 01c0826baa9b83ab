"""Row logs for the compaction tests (tests/test_rows_compact.py on the device,
tests/test_rows_compact_host.py on the host): rows given column by column, ids
and epochs whose 32-bit halves cannot be confused, and logs whose survivors are
a given pattern of positions.  No fixture lives here, so it is a plain module."""
import numpy as np

# the eight lecture lengths of tests/test_rows.py
LECTURES = [b"", b"L", b"CS101-L", b"CS101-L0", b"CS101-L01", b"x" * 32, b"y" * 33, "\u00dcn\u00ef-7".encode()]


def i64(v):
    """Python ints as their low 64 bits, signed"""
    return np.asarray([((int(x) + (1 << 63)) % (1 << 64)) - (1 << 63) for x in v], np.int64)


class Rows:
    """n rows given column by column; what tests/test_rows.py's ``append`` takes"""

    def __init__(self, lectures, ids, ep, valid):
        self.lectures = list(lectures)
        self.idv = np.asarray(ids, np.int64)
        self.ids = [str(v).encode() for v in self.idv.tolist()]
        self.ep = np.asarray(ep, np.int64)
        self.valid = np.asarray(valid, np.uint8)
        self.n = len(self.ids)

    def log(self):
        from rtsas_amd.client_rows import lecture_digest
        return (np.asarray([lecture_digest(x) for x in self.lectures], np.uint64), self.ep, self.idv, self.valid)

    def oracle_rows(self):
        return (self.lectures, self.ids, self.ep.tolist(), self.valid.tolist(), None)


def wild(i):
    """an id and an epoch half whose high and low 32-bit words differ and are unique per row index"""
    i = np.asarray(i, np.int64)
    ids = i64(((int(k) * 2654435761 + 12345) % (1 << 32)) << 32 | ((~int(k)) % (1 << 32)) for k in i)
    lo = np.asarray([(int(k) * 40503 + 7) % (1 << 32) for k in i], np.int64)
    return ids, lo


def patterned(keep, cutoff, seed=0):
    """A log whose survivors under ``cutoff`` are exactly the positions with
    ``keep``: a row to remove is, in turn, an earlier write of the next kept
    row (the other is_valid) or a row of its own below the cutoff; behind the
    last kept row every one is below the cutoff."""
    n = len(keep)
    ids, lo = wild(np.arange(n) + 1000 * seed)
    ep = cutoff + (lo & 0xFFFF)
    lec = [LECTURES[(3 * i + seed) % len(LECTURES)] for i in range(n)]
    valid = (np.arange(n) // 3 % 2).astype(np.uint8)
    nxt = None
    for i in range(n - 1, -1, -1):
        if keep[i]:
            nxt = i
        elif nxt is not None and i % 2 == 0:
            lec[i], ids[i], ep[i], valid[i] = lec[nxt], ids[nxt], ep[nxt], 1 - valid[nxt]
        else:
            ep[i] = cutoff - 1 - (i % 5)
    return Rows(lec, ids, ep, valid)
