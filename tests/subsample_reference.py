"""numpy yardstick of ssf_subsample_batch (include/ssf_frontend.h), written from
the definition's words, not from the kernel: the textbook sequential SplitMix64 generator, the
selection as np.lexsort((index, key))[:nb], quota and replacement as the definition states them.
Host only; one frame per call."""
import numpy as np

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
OK, EMPTY, SHORT = 0, -1, -2


def finalise(z):
    """the SplitMix64 finaliser F on a python int (mod 2^64)"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class SplitMix64:
    """The textbook generator: state += gamma, output = F(state)."""

    def __init__(self, seed):
        self.state = seed & M64

    def next(self):
        self.state = (self.state + GAMMA) & M64
        return finalise(self.state)


def stream_seed(seed, tag, stream):
    """s(stream) = F(F(F(seed + gamma) + tag) + stream)"""
    return finalise(finalise(finalise(seed + GAMMA) + tag) + stream)


def keys_sequential(seed, tag, stream, count, key_bits=32):
    """key(stream, 0 .. count - 1): the high words of the generator's first `count` outputs,
    truncated to key_bits"""
    g = SplitMix64(stream_seed(seed, tag, stream))
    return np.array([(g.next() >> 32) >> (32 - key_bits) for _ in range(count)], dtype=np.uint64)


def _finalise_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keys_random_access(seed, tag, stream, count, key_bits=32):
    """the same keys by the random-access formula key(stream, i) = (F(s + (i + 1) gamma) >> 32)
    >> (32 - key_bits), vectorised (uint64 arithmetic wraps mod 2^64)"""
    s = np.uint64(stream_seed(seed, tag, stream))
    with np.errstate(over="ignore"):
        i1 = np.arange(1, count + 1, dtype=np.uint64)
        z = _finalise_np(s + i1 * np.uint64(GAMMA))
    return (z >> np.uint64(32)) >> np.uint64(32 - key_bits)


def _smallest(keys, members, m):
    """the m members smallest in the total order (key, index), ascending in that order"""
    members = np.asarray(members, dtype=np.int64)
    order = np.lexsort((members, keys[members]))[:m]
    return members[order]


def subsample(pts, nb, seed, tag, cls=None, z_min=None, quota=-1, key_bits=32):
    """One frame.  pts [N, >= 3] f32 -> (idx [nb] int32, xyz [3, nb] f32, n, status)."""
    pts = np.asarray(pts, np.float32)
    N = pts.shape[0]
    if z_min is None:
        surv = np.ones(N, bool)
    else:
        with np.errstate(invalid="ignore"):
            surv = np.logical_not(pts[:, 2] < np.float32(z_min))     # a NaN z survives
    n = int(surv.sum())
    idx = np.zeros(nb, np.int32)
    zero = (idx, np.zeros((3, nb), np.float32))
    if n == 0:
        return (*zero, n, EMPTY)
    k0 = keys_random_access(seed, tag, 0, N, key_bits)
    if quota >= 0:
        fg = surv & (np.asarray(cls) != 0)
        bg = surv & (np.asarray(cls) == 0)
        k_fg = min(int(fg.sum()), quota, nb)
        if int(bg.sum()) < nb - k_fg:
            return (*zero, n, SHORT)
        idx = np.concatenate([_smallest(k0, np.flatnonzero(fg), k_fg),
                              _smallest(k0, np.flatnonzero(bg), nb - k_fg)]).astype(np.int32)
    elif n > nb:
        idx = _smallest(k0, np.flatnonzero(surv), nb).astype(np.int32)
    else:                                   # 1 <= n <= nb: with replacement, stream 1 at 32 bits
        k1 = keys_random_access(seed, tag, 1, nb, 32)
        rank = (k1 * np.uint64(n)) >> np.uint64(32)
        idx = np.flatnonzero(surv)[rank.astype(np.int64)].astype(np.int32)
    return idx, np.ascontiguousarray(pts[idx, :3].T), n, OK


def subsample_batch(pts, sizes, nb, seed, tags=None, cls=None, z_min=None, quota=-1, key_bits=32):
    """F frames packed back to back -> (idx [F, nb], xyz [F, 3, nb], n [F], status [F])."""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = []
    for f in range(len(sizes)):
        a, b = off[f], off[f + 1]
        out.append(subsample(pts[a:b], nb, seed, f if tags is None else int(tags[f]),
                             None if cls is None else cls[a:b], z_min, quota, key_bits))
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
            np.array([o[2] for o in out], np.int32), np.array([o[3] for o in out], np.int32))
