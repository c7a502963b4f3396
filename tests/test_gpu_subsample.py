"""ssf_subsample_batch (k_subsample) bit for bit against tests/subsample_reference.py, the numpy
yardstick: idx, n, status, and xyz equal to the gather.  Every launch here goes through _launch,
which surrounds each output buffer with sentinels and checks them.

Shapes are the smallest that reach each path: survivor counts on both sides of nb (the switch
between the with- and the without-replacement rule), nb from one sort element to the 8192 the
LDS buffer holds, strides 3 and 4, one 200 k frame (the multi-pass select and the strided loops
at full length), truncated keys (ties: the index digits of the select), the z cut, the quota, and
more frames with tags than one launch's tag chunk holds."""
import ctypes as C

import numpy as np
import pytest
import torch

import subsample_reference as SR

pytestmark = pytest.mark.gpu
GUARD = 64
SENT_I, SENT_F = -777, -777.0


@pytest.fixture(scope="module")
def fe(dev):
    import ssf
    return ssf.Frontend(64, device=dev.index or 0)


def _guarded(shape, dtype, sent, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), sent, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _launch(fe, dev, frames, nb, seed, tags=None, cls=None, z_min=None, quota=-1, key_bits=32, want_xyz=True):
    """frames: list of [N, stride] f32 arrays -> (idx, xyz, n, status) numpy, guards checked"""
    import ssf
    from ssf import _abi
    from ssf.frontend import _ptr, _stream
    F = len(frames)
    stride = frames[0].shape[1]
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(frames).astype(np.float32)).reshape(-1, stride)).to(dev)
    off, h_off = ssf.frame_offsets([len(f) for f in frames], dev)
    d_cls = None if cls is None else torch.from_numpy(np.concatenate(cls).astype(np.uint8)).to(dev)
    bufs = [_guarded((F, nb), torch.int32, SENT_I, dev), _guarded((F, 3, nb), torch.float32, SENT_F, dev),
            _guarded((F,), torch.int32, SENT_I, dev), _guarded((F,), torch.int32, SENT_I, dev)]
    (bi, idx), (bx, xyz), (bn, n), (bs, st) = bufs
    h_tag = None if tags is None else np.array([int(t) for t in tags], dtype=np.uint64)
    rc = _abi.lib().ssf_subsample_batch(
        fe._h, _stream(dev), F, _ptr(pts), stride, _ptr(off), C.c_void_p(h_off.data_ptr()), _ptr(d_cls), nb,
        float(0.0 if z_min is None else z_min), 0 if z_min is None else 1, quota, seed,
        None if h_tag is None else h_tag.ctypes.data_as(C.c_void_p), key_bits, _ptr(idx),
        _ptr(xyz) if want_xyz else None, _ptr(n), _ptr(st))
    assert rc == _abi.SSF_OK, _abi.lib().ssf_last_error(fe._h)
    torch.cuda.synchronize()
    for buf, _ in bufs:
        b = buf.cpu().numpy()
        assert np.all(b[:GUARD] == b[0]) and np.all(b[-GUARD:] == b[0]) and b[0] in (SENT_I, SENT_F)
    if not want_xyz:
        assert np.all(bx.cpu().numpy() == SENT_F)
    return idx.cpu().numpy(), xyz.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()


def _check(got, frames, nb, seed, tags=None, cls=None, z_min=None, quota=-1, key_bits=32):
    ref = SR.subsample_batch(np.concatenate(frames), [len(f) for f in frames], nb, seed, tags,
                             None if cls is None else np.concatenate(cls), z_min, quota, key_bits)
    for name, g, r in zip(("idx", "xyz", "n", "status"), got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r, equal_nan=(name == "xyz")), name
    return ref


def _cloud(rng, n, stride):
    return (rng.standard_normal((n, stride)) * 10).astype(np.float32)


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("nb", [1, 100, 2048, 8192])
def test_survivor_counts_around_nb(fe, dev, nb, stride):
    rng = np.random.default_rng(nb * 10 + stride)
    sizes = [1, nb - 1, nb, nb + 1, 5000]                 # nb = 1: a frame of 0 points -> EMPTY
    frames = [_cloud(rng, n, stride) for n in sizes]
    got = _launch(fe, dev, frames, nb, 1234)
    ref = _check(got, frames, nb, 1234)
    assert list(ref[2]) == sizes
    assert list(ref[3]) == [SR.EMPTY if n == 0 else SR.OK for n in sizes]
    for f, n in enumerate(sizes):
        distinct = len(set(got[0][f].tolist()))
        assert distinct == nb if n > nb else distinct <= max(n, 1)


def test_one_large_frame(fe, dev):
    rng = np.random.default_rng(5)
    frames = [_cloud(rng, 200_000, 3)]
    _check(_launch(fe, dev, frames, 8192, 99, tags=[2 ** 63 + 3]), frames, 8192, 99, tags=[2 ** 63 + 3])


@pytest.mark.parametrize("key_bits", [4, 1])
def test_truncated_keys_tie_break_by_index(fe, dev, key_bits):
    rng = np.random.default_rng(key_bits)
    frames = [_cloud(rng, 300, 3), _cloud(rng, 5000, 4)[:, :3].copy()]
    got = _launch(fe, dev, frames, 64, 7, key_bits=key_bits)
    _check(got, frames, 64, 7, key_bits=key_bits)
    keys = SR.keys_random_access(7, 0, 0, 300, key_bits)[got[0][0]]
    assert len(np.unique(keys)) < 64                       # ties decided slots


def test_z_cut(fe, dev):
    rng = np.random.default_rng(8)
    nb, z_min = 100, -3.3
    none = _cloud(rng, 400, 4)
    none[:, 2] = np.abs(none[:, 2])
    some = _cloud(rng, 400, 4)
    exact = _cloud(rng, 400, 4)
    exact[:, 2] = -10.0
    exact[rng.permutation(400)[:nb], 2] = 1.0
    gone = _cloud(rng, 400, 4)
    gone[:, 2] = -3.5
    nan = _cloud(rng, 400, 4)
    nan[::3, 2] = np.nan
    edge = _cloud(rng, 400, 4)
    edge[:, 2] = np.float32(z_min)                         # z == z_min is not below it
    frames = [none, some, exact, gone, nan, edge]
    ref = _check(_launch(fe, dev, frames, nb, 3, z_min=z_min), frames, nb, 3, z_min=z_min)
    assert ref[2][0] == 400 and 0 < ref[2][1] < 400 and ref[2][2] == nb and ref[2][3] == 0 and ref[2][5] == 400
    assert list(ref[3]) == [SR.OK, SR.OK, SR.OK, SR.EMPTY, SR.OK, SR.OK]
    assert np.isnan(nan[ref[0][4], 2]).any()


def test_quota(fe, dev):
    rng = np.random.default_rng(13)
    nb, quota, N = 256, 100, 1000
    frames, cls = [], []
    for n_fg in (0, 7, 100, 350):
        frames.append(_cloud(rng, N, 3))
        c = np.zeros(N, np.uint8)
        c[rng.permutation(N)[:n_fg]] = 1
        cls.append(c)
    short = _cloud(rng, 7 + (nb - 7) - 1, 3)               # 7 foreground, the background one short
    c = np.zeros(len(short), np.uint8)
    c[:7] = 1
    frames.append(short)
    cls.append(c)
    frames.append(_cloud(rng, 7 + (nb - 7), 3))            # the same with exactly enough
    cls.append(c.tolist() + [0])
    cls[-1] = np.array(cls[-1], np.uint8)
    got = _launch(fe, dev, frames, nb, 21, cls=cls, quota=quota)
    ref = _check(got, frames, nb, 21, cls=cls, quota=quota)
    assert list(ref[3]) == [SR.OK] * 4 + [SR.SHORT, SR.OK]
    for f, n_fg in enumerate((0, 7, 100, 350)):
        k = min(n_fg, quota)
        assert cls[f][got[0][f]].tolist() == [1] * k + [0] * (nb - k)
    # with the z cut: the counts are those of the survivors
    frames[3][:, 2] = np.where(cls[3] == 1, -5.0, 1.0)     # every foreground point is cut
    got = _launch(fe, dev, frames, nb, 21, cls=cls, quota=quota, z_min=-3.3)
    _check(got, frames, nb, 21, cls=cls, quota=quota, z_min=-3.3)
    assert cls[3][got[0][3]].sum() == 0 and got[2][3] == N - 350


def test_batch_of_three_is_its_frames(fe, dev):
    rng = np.random.default_rng(17)
    nb = 512
    frames = [_cloud(rng, 0, 3), _cloud(rng, 300, 3), _cloud(rng, 5000, 3)]
    tags = [11, 12, 13]
    a = _launch(fe, dev, frames, nb, 1234, tags=tags)
    _check(a, frames, nb, 1234, tags=tags)
    b = _launch(fe, dev, frames, nb, 1234, tags=tags)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for f in range(3):                                     # each frame alone: the bits of its slice
        one = _launch(fe, dev, [frames[f]], nb, 1234, tags=[tags[f]])
        for x, y in zip(a, one):
            assert np.array_equal(x[f], y[0])
    sw = _launch(fe, dev, frames, nb, 1234, tags=[11, 13, 12])
    _check(sw, frames, nb, 1234, tags=[11, 13, 12])
    assert not np.array_equal(sw[0][1], a[0][1]) and not np.array_equal(sw[0][2], a[0][2])
    assert np.array_equal(sw[2], a[2]) and np.array_equal(sw[3], a[3])
    # no tags: the frame's position
    _check(_launch(fe, dev, frames, nb, 1234), frames, nb, 1234, tags=[0, 1, 2])
    c = _launch(fe, dev, frames, nb, 1234, tags=tags, want_xyz=False)
    assert np.array_equal(c[0], a[0])


def test_more_tagged_frames_than_one_launch_holds(fe, dev):
    rng = np.random.default_rng(19)
    frames = [_cloud(rng, 10 + (k % 3), 3) for k in range(258)]
    tags = [1000 - k for k in range(258)]
    _check(_launch(fe, dev, frames, 4, 6, tags=tags), frames, 4, 6, tags=tags)


def test_wrapper_and_argument_errors(fe, dev):
    import ssf
    from ssf import _abi, asf
    rng = np.random.default_rng(23)
    frames = [_cloud(rng, 700, 4), _cloud(rng, 90, 4)]
    pts = torch.from_numpy(np.concatenate(frames)).to(dev)
    off, h_off = ssf.frame_offsets([700, 90], dev)
    idx, xyz, n, st = asf.subsample(fe, pts, off, h_off, 128, 55, tags=[4, 2 ** 63 + 4], z_min=-3.3)
    got = (idx.cpu().numpy(), xyz.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy())
    _check(got, frames, 128, 55, tags=[4, 2 ** 63 + 4], z_min=-3.3)
    assert asf.subsample(fe, pts, off, h_off, 128, 55, want_xyz=False)[1] is None
    for kw in (dict(nb=0), dict(nb=8193), dict(quota=3), dict(key_bits=0), dict(key_bits=33)):
        with pytest.raises(ssf.SSFError, match="subsample_batch"):
            asf.subsample(fe, pts, off, h_off, **dict(dict(nb=16, seed=1), **kw))
    with pytest.raises(ssf.SSFError):
        asf.subsample(fe, pts[:, :2].contiguous(), off, h_off, 16, 1)
    # a frame above the limit is rejected on the host (the device pointers are never touched)
    big = torch.tensor([0, _abi.SAMPLE_MAX_POINTS + 1], dtype=torch.int64)
    fake = C.c_void_p(16)
    rc = _abi.lib().ssf_subsample_batch(fe._h, None, 1, fake, 3, fake, C.c_void_p(big.data_ptr()), None, 16, 0.0, 0,
                                        -1, 1, None, 32, fake, None, fake, fake)
    assert rc == _abi.SSF_E_ARG and b"2^24" in _abi.lib().ssf_last_error(fe._h)
