"""The yardstick of the map-cloud tests: pcl::transformPointCloud(cloud, out, Eigen::Affine3d) as
PCL 1.10's detail::Transformer<double>::se3 writes it, in numpy float64, one ufunc per operation
(numpy never fuses a multiply with an add):

    out[r] = (float)(((T[r][0]*(double)x + T[r][1]*(double)y) + T[r][2]*(double)z) + T[r][3])

left to right in double, one rounding to float, intensity copied.  Independent of the code under
test, so every comparison against it is bit for bit (``same_bits``)."""
import numpy as np


def transform(xyzi, T):
    """[n, 4] float32 points through T -> [n, 4] float32.  T is one pose (4x4 or 3x4) or one
    pose per point ([n, 3, 4] or [n, 4, 4]); either way every point sees the same scalar
    expression."""
    T = np.asarray(T, np.float64)
    p = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    out = p.copy()
    for r in range(3):
        a, b, c, d = (T[..., r, k] for k in range(4))
        out[:, r] = (((a * x + b * y) + c * z) + d).astype(np.float32)
    return out


def map_points(clouds, Ts):
    """mapCloudPtr: every keyframe cloud through its pose, keyframe order then input order."""
    parts = [transform(c, T) for c, T in zip(clouds, Ts)]
    return np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def cloud(rng, n, half=80.0):
    """n seeded points in +-half m with intensities of the indexInRow + row/100 form
    (src/frameFeature.cpp:77)."""
    xyz = rng.uniform(-half, half, (n, 3)).astype(np.float32)
    inten = (rng.integers(0, 1800, n).astype(np.float32) + rng.integers(0, 64, n).astype(np.float32) / np.float32(100))
    return np.concatenate([xyz, inten.astype(np.float32)[:, None]], 1).astype(np.float32)
