"""Loop detection by appearance: Scan Context descriptors (Kim & Kim, IROS 2018) compared
exhaustively on the device (scan_context.hip; the definitions are in
include/ssf_frontend.h).

``describe`` <- ssf_scan_context_batch: the 20 ring x 60 sector descriptor of ragged clouds in
the sensor frame.  ``match`` <- ssf_scan_context_match: every query against every database
descriptor at all 60 column shifts, and per query the nearest candidate of an eligible prefix of
the database in the order (dist, index).  ``match_topk`` <- ssf_scan_context_match_topk: per
query the k best candidates whose indices lie more than an exclusion window apart, for a caller
that verifies several places (LoopCloser(sc_candidates=...)).  ``ScanContextDB`` keeps the descriptors of a sequence's
keyframes in one growing device buffer.  The CPU implementations' ring-key kd-tree and sector-key
coarse alignment are not built: the exhaustive search replaces both.  There is no host path.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _abi
from .frontend import Frontend, _ptr, _stream

RINGS, SECTORS = _abi.SC_RINGS, _abi.SC_SECTORS
SECTOR_ANGLE = 2.0 * math.pi / SECTORS


def sc_params(max_range=None, lidar_height=None, threshold=None):
    """ssf_sc_params: max_range (80 m), lidar_height (2 m), threshold (0.13, the acceptance
    distance a caller such as LoopCloser applies; the kernels do not read it)."""
    p = _abi.ScParams()
    _abi.lib().ssf_sc_params_default(C.byref(p))
    try:
        if max_range is not None:
            p.max_range = float(max_range)
        if lidar_height is not None:
            p.lidar_height = float(lidar_height)
        if threshold is not None:
            p.threshold = float(threshold)
    except (TypeError, ValueError):
        raise ValueError("sc_params: the parameters are numbers") from None
    if not (math.isfinite(p.max_range) and p.max_range > 0.0):
        raise ValueError("sc_params: max_range must be finite and positive")
    if not math.isfinite(p.lidar_height):
        raise ValueError("sc_params: lidar_height must be finite")
    if math.isnan(p.threshold):
        raise ValueError("sc_params: threshold is not a number")
    return p


def parse_detector(text):
    """"radius" | "scan-context[:THRESHOLD]" (the --map-detector command-line form) ->
    (detector, threshold or None)."""
    kind, sep, thr = str(text).partition(":")
    kind = kind.replace("-", "_")
    if kind not in ("radius", "scan_context"):
        raise ValueError(f"detector {text!r}: radius or scan-context[:THRESHOLD]")
    if not sep:
        return kind, None
    if kind == "radius" or not thr:
        raise ValueError(f"detector {text!r}: only scan-context takes a :THRESHOLD")
    try:
        return kind, float(thr)
    except ValueError:
        raise ValueError(f"detector {text!r}: THRESHOLD must be a number") from None


def parse_candidates(text):
    """"K[:EXCLUSION]" (the --map-sc-candidates command-line form) -> (K, exclusion or None):
    K in 1 .. 8 places verified per keyframe, no two within EXCLUSION keyframes of each other."""
    k, sep, excl = str(text).partition(":")
    try:
        k = int(k)
        excl = int(excl) if sep else None
    except ValueError:
        raise ValueError(f"candidates {text!r}: K[:EXCLUSION], two integers") from None
    if not 1 <= k <= _abi.SC_MAX_TOPK:
        raise ValueError(f"candidates {text!r}: K outside 1 .. {_abi.SC_MAX_TOPK}")
    if excl is not None and excl < 0:
        raise ValueError(f"candidates {text!r}: EXCLUSION is negative")
    return k, excl


def eligible_prefix(stamps, cur_stamp, time_gap) -> int:
    """The number of leading keyframes whose stamp is more than time_gap older than cur_stamp;
    the count stops at the first keyframe that is not, whatever comes after it."""
    n = 0
    for s in stamps:
        if not (cur_stamp - s > time_gap):
            break
        n += 1
    return n


def _check_desc(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3
            and tuple(t.shape[1:]) == (RINGS, SECTORS)):
        raise _abi.SSFError(f"{what}: expected an [n, {RINGS}, {SECTORS}] float32 CUDA tensor")
    return t.contiguous()


def describe(fe: Frontend, pts: torch.Tensor, off: torch.Tensor, h_off: torch.Tensor, params=None):
    """Clouds in the sensor frame ([total, 3] or [total, 4] float32 on the device, x y z first) at
    int64 offsets (device and host copies, as frame_offsets gives them) -> [F, 20, 60] float32."""
    if not (isinstance(pts, torch.Tensor) and pts.is_cuda and pts.dtype == torch.float32 and pts.dim() == 2):
        raise _abi.SSFError("scan_context.describe: expected an [n, 3] or [n, 4] float32 CUDA tensor")
    params = params or sc_params()
    F = int(h_off.numel()) - 1
    pts = pts.contiguous()
    desc = torch.empty((max(F, 0), RINGS, SECTORS), dtype=torch.float32, device=pts.device)
    ho = h_off.contiguous()
    fe._check(_abi.lib().ssf_scan_context_batch(fe._h, _stream(fe.device), F, _ptr(pts), int(pts.shape[1]),
                                                _ptr(off), C.c_void_p(ho.data_ptr()), C.byref(params),
                                                _ptr(desc)), "ssf_scan_context_batch")
    return desc


def describe_one(fe: Frontend, pts: torch.Tensor, params=None) -> torch.Tensor:
    """One cloud -> [20, 60]."""
    h = torch.tensor([0, int(pts.shape[0])], dtype=torch.int64)
    return describe(fe, pts, h.to(pts.device), h, params)[0]


def match(fe: Frontend, queries: torch.Tensor, db: torch.Tensor, n_eligible, full: bool = False):
    """queries [Q, 20, 60] against db [N, 20, 60]; n_eligible: one count for every query or Q of
    them, each 0 .. N.  -> (idx [Q] int32, dist [Q] float32, shift [Q] int32) on the device: per
    query the smallest (dist, index) among candidates 0 .. n_eligible - 1, idx -1 where there is
    none.  full=True: also (dist [Q, N], shift [Q, N]) of every pair."""
    queries = _check_desc(queries, "scan_context.match: queries")
    db = _check_desc(db, "scan_context.match: db")
    Q, N = int(queries.shape[0]), int(db.shape[0])
    ne = np.asarray(n_eligible, np.int64).reshape(-1)
    if ne.size == 1:
        ne = np.repeat(ne, Q)
    if ne.size != Q:
        raise ValueError(f"scan_context.match: {ne.size} n_eligible for {Q} queries")
    if Q and (ne.min() < 0 or ne.max() > N):
        raise ValueError(f"scan_context.match: n_eligible outside 0 .. {N}")
    h_ne = torch.from_numpy(ne.astype(np.int32))
    dev = queries.device
    d_ne = h_ne.to(dev)
    best = torch.empty((Q, _abi.SC_BEST_STRIDE), dtype=torch.int32, device=dev)
    dist = torch.empty((Q, N), dtype=torch.float32, device=dev) if full else None
    shift = torch.empty((Q, N), dtype=torch.int32, device=dev) if full else None
    fe._check(_abi.lib().ssf_scan_context_match(fe._h, _stream(fe.device), Q, _ptr(queries), N,
                                                _ptr(db) if N else None, _ptr(d_ne),
                                                C.c_void_p(h_ne.data_ptr()), _ptr(dist), _ptr(shift),
                                                _ptr(best)), "ssf_scan_context_match")
    out = (best[:, _abi.SC_BEST["INDEX"]], best[:, _abi.SC_BEST["DIST"]].view(torch.float32),
           best[:, _abi.SC_BEST["SHIFT"]])
    return out + (dist, shift) if full else out


def _check_topk(k, exclusion, what):
    """k in 1 .. SC_MAX_TOPK and exclusion >= 0, both integers -> (k, exclusion)."""
    for name, v in (("k", k), ("exclusion", exclusion)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: {name} is an integer, not {v!r}")
    if not 1 <= k <= _abi.SC_MAX_TOPK:
        raise ValueError(f"{what}: k outside 1 .. {_abi.SC_MAX_TOPK}")
    if exclusion < 0:
        raise ValueError(f"{what}: exclusion is negative")
    return int(k), min(int(exclusion), 2 ** 31 - 1)


def match_topk(fe: Frontend, queries: torch.Tensor, db: torch.Tensor, n_eligible, k: int, exclusion: int = 0,
               full: bool = False):
    """``match`` with the k best places per query instead of the one best candidate
    (ssf_scan_context_match_topk): the candidates 0 .. n_eligible - 1 are walked in the order
    (dist, index) and one is taken when its index differs by more than `exclusion` from every index
    already taken, until k are taken or none is left.  k in 1 .. 8, exclusion >= 0 (ValueError
    before any device call).  -> (idx [Q, k] int32, dist [Q, k] float32, shift [Q, k] int32) on the
    device, in rank order, an unfilled slot (-1, 1.0, 0); column 0 is ``match``'s result bit for
    bit.  full=True: also (dist [Q, N], shift [Q, N]) of every pair."""
    k, exclusion = _check_topk(k, exclusion, "scan_context.match_topk")
    queries = _check_desc(queries, "scan_context.match_topk: queries")
    db = _check_desc(db, "scan_context.match_topk: db")
    Q, N = int(queries.shape[0]), int(db.shape[0])
    ne = np.asarray(n_eligible, np.int64).reshape(-1)
    if ne.size == 1:
        ne = np.repeat(ne, Q)
    if ne.size != Q:
        raise ValueError(f"scan_context.match_topk: {ne.size} n_eligible for {Q} queries")
    if Q and (ne.min() < 0 or ne.max() > N):
        raise ValueError(f"scan_context.match_topk: n_eligible outside 0 .. {N}")
    h_ne = torch.from_numpy(ne.astype(np.int32))
    dev = queries.device
    d_ne = h_ne.to(dev)
    best = torch.empty((Q, k, _abi.SC_BEST_STRIDE), dtype=torch.int32, device=dev)
    dist = torch.empty((Q, N), dtype=torch.float32, device=dev) if full else None
    shift = torch.empty((Q, N), dtype=torch.int32, device=dev) if full else None
    fe._check(_abi.lib().ssf_scan_context_match_topk(fe._h, _stream(fe.device), Q, _ptr(queries), N,
                                                     _ptr(db) if N else None, _ptr(d_ne),
                                                     C.c_void_p(h_ne.data_ptr()), _ptr(dist), _ptr(shift),
                                                     _ptr(best), k, exclusion), "ssf_scan_context_match_topk")
    out = (best[:, :, _abi.SC_BEST["INDEX"]], best[:, :, _abi.SC_BEST["DIST"]].view(torch.float32),
           best[:, :, _abi.SC_BEST["SHIFT"]])
    return out + (dist, shift) if full else out


class ScanContextDB:
    """The descriptors of a sequence's keyframes in one device buffer [capacity, 20, 60]; the
    capacity doubles with the contents kept (as ssf.MapCloud's store does), between growths
    nothing is allocated.  The buffer is allocated at the first append."""

    def __init__(self, fe: Frontend, capacity: int = 256):
        self.fe = fe
        self.capacity = max(int(capacity), 1)
        self.buf = None
        self.n = 0
        self.generation = 0              # bumped when the descriptors move to a larger buffer

    def __len__(self):
        return self.n

    def descriptors(self) -> torch.Tensor:
        """[n, 20, 60], a view of the buffer."""
        if self.buf is None:
            return torch.empty((0, RINGS, SECTORS), dtype=torch.float32, device=self.fe.device)
        return self.buf[:self.n]

    def append(self, desc: torch.Tensor) -> int:
        """One descriptor [20, 60] or several [k, 20, 60] -> the index of the first."""
        d = desc.unsqueeze(0) if desc.dim() == 2 else desc
        d = _check_desc(d, "ScanContextDB.append")
        k, first = int(d.shape[0]), self.n
        if self.buf is None:
            while self.capacity < k:
                self.capacity *= 2
            self.buf = torch.empty((self.capacity, RINGS, SECTORS), dtype=torch.float32, device=d.device)
        if first + k > self.capacity:
            while self.capacity < first + k:
                self.capacity *= 2
            new = torch.empty((self.capacity, RINGS, SECTORS), dtype=torch.float32, device=self.buf.device)
            new[:first].copy_(self.buf[:first])
            self.buf = new
            self.generation += 1
        self.buf[first:first + k].copy_(d)
        self.n = first + k
        return first

    def query(self, desc: torch.Tensor, n_eligible=None):
        """A descriptor [20, 60] against the stored prefix 0 .. n_eligible - 1 (default: all)
        -> (idx, dist, shift) as Python numbers, idx -1 without a candidate.  Several
        descriptors [Q, 20, 60] -> the three device tensors of ``match``."""
        n_el = self.n if n_eligible is None else n_eligible
        one = desc.dim() == 2
        q = desc.unsqueeze(0) if one else desc
        idx, dist, shift = match(self.fe, q, self.descriptors(), n_el)
        if not one:
            return idx, dist, shift
        return int(idx[0]), float(dist[0]), int(shift[0])

    def query_topk(self, desc: torch.Tensor, k: int, exclusion: int = 0, n_eligible=None):
        """A descriptor [20, 60] against the stored prefix -> the at most k places ``match_topk``
        takes, a list of (idx, dist, shift) tuples of Python numbers in rank order (unfilled
        slots dropped).  Several descriptors [Q, 20, 60] -> the three [Q, k] device tensors."""
        k, exclusion = _check_topk(k, exclusion, "ScanContextDB.query_topk")
        n_el = self.n if n_eligible is None else n_eligible
        one = desc.dim() == 2
        q = desc.unsqueeze(0) if one else desc
        idx, dist, shift = match_topk(self.fe, q, self.descriptors(), n_el, k, exclusion)
        if not one:
            return idx, dist, shift
        rows = zip(idx[0].tolist(), dist[0].tolist(), shift[0].tolist())
        return [(i, d, s) for i, d, s in rows if i >= 0]
