"""Inputs shared by the row log group-by tests (test_rows_group_host.py on the
CPU, test_rows_group.py on the GPU): the count sets of the median select and a
hand-built batch of attendance rows.  No fixture lives here: a plain module."""

DAY0 = 1742169600  # 2025-03-17T00:00:00Z, a Monday
LATE = 9 * 3600

# group counts: the digit boundaries of the 8-bit radix rounds, all equal, n = 1, 2, 3, even and odd n
COUNT_SETS = {
    "digits_odd": [255, 256, 257, 65535, 65536],
    "digits_even": [65536, 255, 65535, 257, 256, 1],
    "all_equal": [7] * 6,
    "all_equal_256": [256] * 5,
    "n1": [5],
    "n2": [9, 3],
    "n3": [4, 1, 9],
    "even_far": [1, 1, 70000, 70000],
}

IDS = [-(1 << 40), -5, -1, 0, 7, 1001, 1002, 1003, 20000, (1 << 62) + 3]
# a skewed draw: a few students attend far more than the others
DRAW = [4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 0, 1, 2, 3, 6, 7, 8, 9, 4, 5, 1, 4]
SECONDS = [8 * 3600 + 3599, 9 * 3600, 0, 86399, 12 * 3600 + 30 * 60, 7 * 3600 + 5]


def hand_batches():
    """Two batches in arrival order, about 270 rows: three lectures over a week,
    epochs at 08:59:59 and 09:00:00, a negative epoch, negative ids, a lecture
    with one student ("solo") and one with two ("pair"), and a second batch
    that redelivers every fourth of the first 48 rows with is_valid flipped."""
    lectures, ids, epochs, valid = [], [], [], []
    for i in range(240):
        lectures.append(("CS101", "MA201", "PH301")[(i * 5 + i // 7) % 3])
        ids.append(str(IDS[DRAW[(i * 3 + i // 11) % len(DRAW)]]))
        epochs.append(DAY0 + (i % 7) * 86400 + SECONDS[(i + i // 6) % len(SECONDS)])
        valid.append(0 if i % 3 == 0 else 1)
    extra = [("CS101", "-5", -1, 1), ("CS101", "7", -1, 0), ("MA201", "0", -86400 * 3 - 1, 1),
             ("solo", "1001", DAY0 + LATE, 1), ("solo", "1001", DAY0 + LATE + 1, 0), ("solo", "1001", DAY0 + 86400, 1),
             ("pair", "-1", DAY0 + LATE - 1, 1), ("pair", "7", DAY0 + LATE, 1), ("pair", "7", DAY0 + LATE + 60, 0)]
    for lec, i, e, v in extra:
        lectures.append(lec), ids.append(i), epochs.append(e), valid.append(v)
    again = range(0, 48, 4)
    second = ([lectures[i] for i in again] + ["solo"], [ids[i] for i in again] + ["1001"],
              [epochs[i] for i in again] + [DAY0 + LATE + 1], [1 - valid[i] for i in again] + [1], None)
    return [(lectures, ids, epochs, valid, None), second]
