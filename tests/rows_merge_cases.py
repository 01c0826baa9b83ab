"""Inputs shared by the group-merge tests (test_rows_group_merge_host.py and
test_sharded_exact_gloo.py on the CPU, test_rows_group_merge.py on the GPU): a
random batch of attendance rows in test_rows_group.random_batch's style, the
split of batches over ranks by lecture, and the three per-student filters of
StudentCounts._EXACT as rows_group keywords.  No fixture lives here: a plain
module."""
import zlib

import numpy as np

from rows_group_cases import DAY0, LATE

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
LECTURES = ("a", "bb", "CS101-L01", "CS101-L02", "MA201", "PH301-2025", "x" * 30)
# StudentCounts._EXACT as rows_group / rows_group_oracle keywords
FILTERS = {"attended": dict(), "late": dict(late_from=LATE), "invalid": dict(valid=False)}


def random_batch(n, seed, nids=None, lectures=LECTURES):
    """n rows with repeats: ids of both signs and the extremes, epochs on the
    filters' boundaries (32399, 32400, -1) and around, either validity"""
    rng = np.random.default_rng(seed)
    pool = np.asarray([I64_MIN, -1, 0, I64_MAX] + rng.integers(-(1 << 62), 1 << 62, (nids or max(n // 5, 1))).tolist(),
                      dtype=object)
    ids = [str(int(v)) for v in pool[rng.integers(0, pool.size, n)]]
    marks = np.asarray([LATE - 1, LATE, -1, 86399, 86400, DAY0 + LATE, DAY0 + LATE - 1, -86400 - 1])
    ep = np.where(rng.random(n) < 0.5, marks[rng.integers(0, marks.size, n)], rng.integers(-200000, 200000, n))
    return ([lectures[j] for j in rng.integers(0, len(lectures), n)], ids, ep.astype(np.int64).tolist(),
            rng.integers(0, 2, n).tolist(), None)


def lecture_owner(lecture, world: int) -> int:
    """the rank that owns a lecture: a hash of its name, the same in every process"""
    return zlib.crc32(str(lecture).encode()) % world


def split_by_lecture(batches, world: int, owner=lecture_owner):
    """``world`` lists of batches: every row goes to its lecture's owner, the
    arrival order kept inside each part"""
    parts = [[] for _ in range(world)]
    for lectures, ids, epochs, valid, take in batches:
        assert take is None
        valid = [0] * len(ids) if valid is None else valid
        rows = [([], [], [], []) for _ in range(world)]
        for row in zip(lectures, ids, epochs, valid):
            dst = rows[owner(row[0], world)]
            for col, v in zip(dst, row):
                col.append(v)
        for r in range(world):
            if rows[r][0]:
                parts[r].append(rows[r] + (None,))
    return parts


def merge_entries(parts):
    """the parts' (keys, counts) end to end, as uint64 words"""
    keys = np.concatenate([np.asarray(p["keys"]).view(np.uint64) for p in parts] + [np.zeros(0, np.uint64)])
    counts = np.concatenate([np.asarray(p["counts"], np.uint64) for p in parts] + [np.zeros(0, np.uint64)])
    return keys, counts
