"""csrc/numpy_rng.hpp (the host RandomState behind the GMM k-means++ draws) against numpy itself:
tests/host/numpy_rng_main.cpp, a plain g++ program that includes only that header, is fed
commands on stdin and its output compared with np.random.RandomState.  No GPU, no library."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "numpy_rng_main.cpp")
CSRC = os.path.join(REPO, "ssf-slam_amd", "csrc")


@pytest.fixture(scope="module")
def rng_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("numpy_rng") / "numpy_rng_main")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, commands):
    """One process, one fresh (unseeded) state: the output lines of the commands."""
    r = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return r.stdout.split()


def _bits(values):
    return np.array(values, np.float64).view(np.uint64)


def _choice_ref(n, us):
    """RandomState.choice(n, p=ones/n) for the uniform draws us, as numpy computes it."""
    cdf = np.cumsum(np.full(n, 1.0 / n))
    cdf /= cdf[-1]
    return cdf, [min(int(np.searchsorted(cdf, u, side="right")), n - 1) for u in us]


def _choices(exe, cases):
    """cases: [(n, [u, ...])] asked in this order of one state -> [[index, ...]] per case."""
    out = _run(exe, [f"choice {n} {float(u)!r}" for n, us in cases for u in us])
    got, k = [], 0
    for _, us in cases:
        got.append([int(v) for v in out[k:k + len(us)]])
        k += len(us)
    return got


@pytest.mark.parametrize("seed", [0, 1, 123, 20240000, 2**32 - 1])
def test_random_sample_bit_equal(rng_exe, seed):
    got = _run(rng_exe, [f"seed {seed}", "sample 1000"])
    ref = np.random.RandomState(seed).random_sample(1000)
    assert np.array_equal(_bits([float(v) for v in got]), ref.view(np.uint64))


def test_seed_restarts_the_stream_and_unseeded_is_5489(rng_exe):
    got = [float(v) for v in _run(rng_exe, ["sample 10", "seed 1", "sample 7", "seed 123", "sample 1000"])]
    assert np.array_equal(_bits(got[:10]), np.random.RandomState(5489).random_sample(10).view(np.uint64))
    assert np.array_equal(_bits(got[10:17]), np.random.RandomState(1).random_sample(7).view(np.uint64))
    assert np.array_equal(_bits(got[17:]), np.random.RandomState(123).random_sample(1000).view(np.uint64))


def test_choice_uniform_matches_searchsorted(rng_exe):
    edge = [0.0, 0.5, np.nextafter(1.0, 0.0)]
    cases = []
    for n in (1, 2, 3, 7):                   # every cdf entry and its two float neighbours
        cdf, _ = _choice_ref(n, [])
        cases.append((n, edge + [v for c in cdf for v in (np.nextafter(c, 0.0), c, np.nextafter(c, 2.0))]))
    for n in (1000, 131072):
        cases.append((n, edge + list(np.random.default_rng(n).random(200))))
    got = _choices(rng_exe, cases)
    for (n, us), g in zip(cases, got):
        assert g == _choice_ref(n, us)[1], n


def test_choice_cache_eviction_keeps_answers_right(rng_exe):
    """More than 8 cached sizes clear the table: after 10 distinct n in a row the first n is
    computed afresh and still answers like numpy (and so does every n on the way)."""
    us = [0.0, 0.31, 0.5, 0.77, np.nextafter(1.0, 0.0)]
    cases = [(n, us) for n in range(11, 21)] + [(11, us), (12, us)]
    got = _choices(rng_exe, cases)
    for (n, _), g in zip(cases, got):
        assert g == _choice_ref(n, us)[1], n
