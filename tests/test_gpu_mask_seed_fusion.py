"""The fused seeding passes of k_mask_pose (mask_seed.hpp): pass 0 also forms the k-means++
distances to the first centre and leaves their 64-point block totals, and the candidate stream
also labels Lloyd iteration 0 under both candidates.

Every case: the k-means++ indices, KM_ITER and EM_ITER equal oracle.mask_and_pose, the mask is
equal byte for byte, t within 1e-5 m.  The index equalities are conditions, not tolerances, so the
draws are chosen on the CPU (`_draws`, `_margins`): with D(i) the squared distance to the first
centre and cs its in-order cumulative sum, a candidate draw u picks the first i with
cs[i] >= u pot.  A draw is admitted when u pot lies more than MARGIN = 1e-9 of the potential above
cs[i - 1] and below cs[i]: the kernel's sums differ from the oracle's by their order only, at most
n 2^-53 = 4.6e-13 of the potential at n = 4099, so neither side's answer sits on a tie.  Three
draws have a one-sided or no margin by construction, and need none:
  u = 0.0        u pot = 0 exactly on both sides and cs[0] >= 0: index 0, whatever the rounding
  u = 1 - 2^-53  no i reaches u pot or only the last does: both clamp to n - 1; the lower side
                 (cs[n - 2] below u pot, i.e. D(n - 1) > MARGIN pot) is checked
  block ends     u pot is put midway between cs[i - 1] and cs[i]: margin D(i) / (2 pot), checked
Frames are subsets of one synthetic scan (at most 4099 points), a launch takes milliseconds.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import frame

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
STORAGE = {"f32": np.float32, "f64": np.float64}
# partial blocks, empty slots, and one, two and three trips of the two-deep 768-thread loop
SIZES = [2, 63, 64, 65, 767, 768, 769, 1537, 4099]


@functools.lru_cache(maxsize=None)
def _cloud(n, seq=11):
    """n points spread over a 64 x 65 scan (float32 pos1, flow)"""
    p, f, _ = frame(seq, 2, n_az=65)
    idx = np.linspace(0, p.shape[0] - 1, n).round().astype(np.int64)
    return np.ascontiguousarray(p[idx]), np.ascontiguousarray(f[idx])


def _first_centre(n, u0):
    """RandomState.choice(n, p = 1 / n) of the draw u0, as the oracle does it"""
    cdf = np.cumsum(np.full(n, 1.0 / n))
    cdf /= cdf[-1]
    hit = np.nonzero(cdf > u0)[0]
    return int(hit[0]) if len(hit) else n - 1


def _cumsum(p, f, c0):
    """in-order cumulative sum of D(i), the oracle's expression"""
    X = np.concatenate([f, p], axis=1).astype(np.float64)
    Xc = X - X.sum(axis=0) / len(X)
    c = Xc[c0]
    d = (-2.0 * (Xc @ c) + c @ c) + (Xc * Xc).sum(axis=1)
    return np.cumsum(np.maximum(d, 0.0))


def _margins(cs, u):
    """(index, margin below, margin above) of the candidate draw u, margins in units of pot"""
    pot, rv, n = cs[-1], u * cs[-1], len(cs)
    hit = np.nonzero(cs >= rv)[0]
    i = int(hit[0]) if len(hit) else n - 1
    if rv == 0.0:
        return 0, np.inf, np.inf
    below = (rv - cs[i - 1]) / pot if i > 0 else np.inf
    above = (cs[i] - rv) / pot if i < n - 1 else np.inf      # past the end: both clamp to n - 1
    return i, below, above


def _draws(p, f, seed, u0=None, u1=None, u2=None):
    """three draws for the frame: given ones kept, the others the first of default_rng(seed) whose
    candidate indices clear MARGIN on both sides; every candidate draw is checked"""
    rng = np.random.default_rng(seed)
    n = len(p)
    u0 = rng.random() if u0 is None else u0
    cs = _cumsum(p, f, _first_centre(n, u0))
    out = [u0]
    for u in (u1, u2):
        for _ in range(100):
            v = rng.random() if u is None else u
            _, below, above = _margins(cs, v)
            if min(below, above) > MARGIN:
                break
            assert u is None, (u, below, above)
        else:
            raise AssertionError("no draw clears the margin")
        out.append(v)
    return np.array(out)


def _block_end_draw(cs, i):
    assert i % 64 == 63 and cs[i] > cs[i - 1]
    return 0.5 * (cs[i - 1] + cs[i]) / cs[-1]


@functools.lru_cache(maxsize=None)
def _frontend(G, queue=0):
    import ssf
    fe = ssf.Frontend(64, device=0)
    fe.mask_split(G)
    if queue:
        fe.mask_schedule(None, queue)
    return fe


def _launch(storage, G, frames, queue=0):
    """frames [(pos1, flow, draws)] as one ragged batch -> (out [F, 32], [mask per frame])"""
    import ssf
    dev = torch.device("cuda", 0)
    sizes = [len(fr[0]) for fr in frames]
    cat = lambda k: torch.from_numpy(np.concatenate([fr[k] for fr in frames]).astype(STORAGE[storage])).to(dev)
    off, h_off = ssf.frame_offsets(sizes, dev)
    out, bg = _frontend(G, queue).mask_pose(cat(0), cat(1), off, h_off, draws=np.stack([fr[2] for fr in frames]))
    torch.cuda.synchronize()
    out, bg = out.cpu().numpy(), bg.cpu().numpy()
    e = np.cumsum([0] + sizes)
    return out, [bg[e[k]:e[k + 1]] for k in range(len(sizes))]


def _check(oracle, tag, fr, o, bg):
    p, f, draws = fr
    ref = oracle.mask_and_pose(p, f, draws)
    info = ref["info"]
    print(f"{tag}: n={len(p)} centres {int(o[22])},{int(o[23])} / {int(info['center0'])},{int(info['center1'])} "
          f"km {int(o[19])}/{int(info['kmeans_iter'])} em {int(o[20])}/{int(info['em_iter'])} "
          f"mask diff {int((bg != ref['bg_mask']).sum())} dt {np.abs(o[0:3] - ref['t']).max():.3e}")
    assert o[16] == ref["rc"] == 0, (tag, o[16], ref["rc"])
    assert (int(o[22]), int(o[23])) == (int(info["center0"]), int(info["center1"])), tag
    assert int(o[19]) == int(info["kmeans_iter"]) and int(o[20]) == int(info["em_iter"]), tag
    assert np.array_equal(bg, ref["bg_mask"]), tag
    assert np.abs(o[0:3] - ref["t"]).max() < 1e-5, tag
    return ref


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("storage", sorted(STORAGE))
def test_block_and_trip_edges(oracle, dev, storage, n):
    p, f = _cloud(n)
    fr = (p, f, _draws(p, f, 100 + n))
    out, bg = _launch(storage, 1, [fr])
    _check(oracle, f"{storage} n={n}", fr, out[0], bg[0])


N_EDGE = 1537


def _edge_frames():
    p, f = _cloud(N_EDGE)
    n = len(p)
    cs = _cumsum(p, f, _first_centre(n, 0.37))
    top = 1.0 - 2.0 ** -53
    assert (cs[-1] - cs[-2]) / cs[-1] > MARGIN            # D(n - 1): cs[n - 2] is clear of u pot
    ends = _block_end_draw(cs, 383), _block_end_draw(cs, 767)
    assert all(_margins(cs, u)[0] == i and min(_margins(cs, u)[1:]) > MARGIN for u, i in zip(ends, (383, 767)))
    return {
        "first_centre_0": (p, f, _draws(p, f, 1, u0=0.0)),
        "first_centre_last": (p, f, _draws(p, f, 2, u0=(n - 0.5) / n)),
        "candidate_draw_0": (p, f, _draws(p, f, 3, u0=0.37, u1=0.0)),
        "candidate_draw_top": (p, f, np.array([0.37, _draws(p, f, 4, u0=0.37)[1], top])),
        "candidate_block_ends": (p, f, np.array([0.37, ends[0], ends[1]])),
        "candidates_equal": (p, f, np.repeat(_draws(p, f, 5, u0=0.37)[:2], [1, 2])),
    }


@pytest.mark.parametrize("case", ["first_centre_0", "first_centre_last", "candidate_draw_0", "candidate_draw_top",
                                  "candidate_block_ends", "candidates_equal"])
def test_draw_edges(oracle, dev, case):
    fr = _edge_frames()[case]
    out, bg = _launch("f32", 1, [fr])
    ref = _check(oracle, case, fr, out[0], bg[0])
    n = N_EDGE
    c0 = int(ref["info"]["center0"])
    if case == "first_centre_0":
        assert c0 == 0
    if case == "first_centre_last":
        assert c0 == n - 1
    cs = _cumsum(fr[0], fr[1], c0)
    picks = [_margins(cs, u)[0] for u in fr[2][1:]]
    assert int(ref["info"]["center1"]) in picks
    if case == "candidate_draw_0":
        assert picks[0] == 0
    if case == "candidate_draw_top":
        assert picks[1] == n - 1
    if case == "candidate_block_ends":
        assert picks == [383, 767]
    if case == "candidates_equal":
        assert picks[0] == picks[1]


@pytest.mark.parametrize("n", [1537, 4099])
@pytest.mark.parametrize("G", [1, 2, 3])
def test_parts(oracle, dev, G, n):
    """parts start at multiples of 128; G > 1 exchanges the part potentials (exchange_prefix) and
    the 2 potentials + 28 sums of the candidate stream (exchange<30>)"""
    p, f = _cloud(n)
    fr = (p, f, _draws(p, f, 200 + n))
    out, bg = _launch("f32", G, [fr])
    _check(oracle, f"split {G} n={n}", fr, out[0], bg[0])
    ref, rbg = _launch("f32", 1, [fr])
    assert [int(v) for v in out[0][[22, 23, 19, 20]]] == [int(v) for v in ref[0][[22, 23, 19, 20]]]
    assert np.array_equal(bg[0], rbg[0])


def test_ticket_reuse_keeps_no_totals(oracle, dev):
    """a frame queue of 2 work-groups over 7 frames of different sizes: a work-group's block totals
    and Lloyd sums of one frame must not reach its next; every frame as launched one per work-group"""
    frames = []
    for k, n in enumerate([4099, 65, 1537, 2, 769, 64, 768]):
        p, f = _cloud(n, seq=12 + k)
        frames.append((p, f, _draws(p, f, 300 + k)))
    ref, rbg = _launch("f32", 1, frames)
    out, bg = _launch("f32", 1, frames, queue=2)
    assert np.array_equal(out.view(np.uint64), ref.view(np.uint64))
    assert all(np.array_equal(a, b) for a, b in zip(bg, rbg))
    for k, fr in enumerate(frames):
        _check(oracle, f"queue frame {k}", fr, out[k], bg[k])


def test_iteration_0_ends_the_fit(oracle, dev):
    """two blobs of 0.05 m spread 400 m apart: tol = 1e-4 x the mean column variance is about 0.7,
    and moving the two seeded centres (data points) to their blobs' means shifts them by about
    0.03 in all, so Lloyd meets tol at iteration 0 and mask_lloyd runs no pass"""
    rng = np.random.default_rng(17)
    n = 1000
    side = rng.random(n) < 0.4
    p = (rng.standard_normal((n, 3)) * 0.05 + np.where(side[:, None], 400.0, 0.0)).astype(np.float32)
    f = (rng.standard_normal((n, 3)) * 0.05 + np.where(side[:, None], 0.5, 0.0)).astype(np.float32)
    fr = (p, f, _draws(p, f, 400))
    assert int(oracle.mask_and_pose(p, f, fr[2])["info"]["kmeans_iter"]) == 1
    for G in (1, 2):
        out, bg = _launch("f32", G, [fr])
        _check(oracle, f"iteration 0 ends the fit, split {G}", fr, out[0], bg[0])
        assert int(out[0][19]) == 1
