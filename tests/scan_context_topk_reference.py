"""numpy yardstick of the selection of ssf_scan_context_match_topk (include/ssf_frontend.h,
DESIGN.md §6.12), written from the definition alone.  It does not import the product code.

  For one query with eligible prefix [0, n_eligible), k >= 1 and exclusion E >= 0: walk the
  candidates in the total order (dist, index), a NaN distance counting as +infinity; take a
  candidate when its index differs by more than E from every index already taken; stop at k taken
  or when the prefix is exhausted.  Slot j is the j-th taken candidate (index, dist, shift), dist
  and shift copied from the rows; an unfilled slot is (-1, 1.0, 0).
"""
import numpy as np

NONE = (-1, np.float32(1.0), 0)


def select_topk(dist_row, shift_row, n_eligible, k, exclusion):
    """-> (idx [k] int32, dist [k] float32, shift [k] int32)."""
    n, k, E = int(n_eligible), int(k), int(exclusion)
    assert k >= 1 and E >= 0 and 0 <= n <= len(dist_row)
    d = np.asarray(dist_row, np.float32)[:n]
    s = np.asarray(shift_row, np.int32)[:n]
    key = np.where(np.isnan(d), np.float32(np.inf), d)
    order = np.lexsort((np.arange(n), key))                        # by key, then by index
    taken = []
    for i in order:
        if len(taken) == k:
            break
        if all(abs(int(i) - t) > E for t in taken):
            taken.append(int(i))
    idx = np.full(k, NONE[0], np.int32)
    dist = np.full(k, NONE[1], np.float32)
    shift = np.full(k, NONE[2], np.int32)
    for j, i in enumerate(taken):
        idx[j], dist[j], shift[j] = i, d[i], s[i]
    return idx, dist, shift
