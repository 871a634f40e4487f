"""Rounds of a batch of families: what StructureScore.local_scores and CITester.tests share."""

# Largest number of count bins one round keeps on the device (int64: 128 MiB).  A batch with more runs in
# several rounds; a single family above the budget runs alone.
SCORE_BIN_BUDGET = 1 << 24


def rounds(sizes, budget):
    """Consecutive runs of families whose bins stay within `budget`; a family above it is a run of its own."""
    out, cur, bins = [], [], 0
    for i, s in enumerate(sizes):
        if cur and bins + s > budget:
            out.append(cur)
            cur, bins = [], 0
        cur.append(i)
        bins += s
    if cur:
        out.append(cur)
    return out
