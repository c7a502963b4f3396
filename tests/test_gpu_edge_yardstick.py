"""The device's edge selection (the third bit plane of every feature kernel: k_feat_wave_reg<*, true>
and the second wave kernel, k_feat_chunk<*, true> and its flagged twin, k_bin_curv<*, true>, both
k_select<true>) and k_edge_table against the independent yardsticks of tests/feature_reference.py
(select_edges) and tests/edge_reference.py (line_table) -- not against the CPU oracle, which
tests/test_edge_host.py holds to the same yardsticks, cases and bars.

Selection: every case of tests/edge_cases.py as a frame of one ragged launch (an empty frame among
them), in every input order launch_extract_planes routes differently, padded past the single-read
capacity and at a stride of 4097 floats; edge_span 1, 3, 10, 63, 64, 65 and 200, edge_min at,
below and above a curvature value.  Bar: bit equality of lists and counts; every count within
the batch's max_points; a second identical launch gives equal bits.

Line table: hand-made edge clouds (frame sizes around 5, the 1024-thread stride and the 8192-edge
LDS cap, both paths in one launch, exact ties, degenerate covariances, thresholds met exactly),
bars of edge_cases.compare_table.
"""
import numpy as np
import pytest
import torch

import edge_cases as ec
import feature_cases as fc
import feature_reference as ref
from test_feature_host import bits_equal, seen_cloud
from test_gpu_feature_yardstick import _frames as plane_frames

pytestmark = pytest.mark.gpu
F32 = np.float32


def _selection_frames(n_rows, layout):
    """the plane test's frames of this layout (its yardstick runs are shared, never changed)
    plus the edge rows' -> [(name, pts, keep, extract_planes of the seen cloud)]"""
    out = list(plane_frames(n_rows, layout))
    for cs in fc.edge_rows(n_rows):
        pts, keep = fc.layout(cs, layout)
        out.append((cs.name, pts, keep, ref.extract_planes(seen_cloud(pts, keep), n_rows)))
    return out


def _run_selection(dev, n_rows, frames, what):
    import ssf
    fe = ssf.Frontend(n_rows, device=dev.index or 0)
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([f[1] for f in frames]))).to(dev)
    off, h_off = ssf.frame_offsets([len(f[1]) for f in frames], dev)
    keep = None
    if frames[0][2] is not None:
        keep = torch.from_numpy(np.concatenate([f[2] for f in frames])).to(dev)
    h = [int(v) for v in h_off]
    n_edges = 0
    for tag, em, span in ec.selection_runs(n_rows):
        fe.edge_config(edge_min=float(em), edge_span=span)
        got = []
        for _ in range(2):                                       # the second launch: equal bits
            pb, eb = fe.extract_features_batch(pts, off, h_off, keep=keep)
            torch.cuda.synchronize()
            got.append((pb.count.cpu().numpy(), pb.xyzi.cpu().numpy(), eb.count.cpu().numpy(), eb.xyzi.cpu().numpy()))
        pcount, plane, ecount, edge = got[0]
        assert int(ecount.max()) <= eb.max_points, (what, tag, int(ecount.max()), eb.max_points)
        if span == 1:
            assert eb.max_points == max(len(f[1]) for f in frames), (what, tag)
        for f, (name, _, _, y) in enumerate(frames):
            E, _ = ref.select_edges(y["rx"], y["cv"], y["off"], n_rows, em, span)
            o = h[f]
            assert int(ecount[f]) == len(E), (what, name, tag, "edge count", int(ecount[f]), len(E))
            assert bits_equal(edge[o:o + len(E)], E), (what, name, tag, "edge list")
            assert int(pcount[f]) == len(y["planes"]) and bits_equal(plane[o:o + len(y["planes"])], y["planes"]), \
                (what, name, tag, "plane list")
            assert np.array_equal(got[1][3][o:o + len(E)].view(np.uint32), edge[o:o + len(E)].view(np.uint32)), \
                (what, name, tag, "second launch")
            n_edges += len(E)
        assert np.array_equal(got[1][2], ecount) and np.array_equal(got[1][0], pcount), (what, tag, "second launch")
    assert n_edges > 0
    return n_edges


@pytest.mark.parametrize("layout", fc.LAYOUTS)
@pytest.mark.parametrize("n_rows", [16, 64])
def test_edge_selection_equals_yardstick(dev, n_rows, layout):
    frames = _selection_frames(n_rows, layout)
    assert [f[0] for f in frames][2] == "empty" and len(frames[2][1]) == 0          # between full ones
    _run_selection(dev, n_rows, frames, (n_rows, layout))


@pytest.mark.parametrize("n_rows", [16, 64])
def test_edge_selection_binned_stage(dev, n_rows):
    """one frame padded with NaN points past 262144: every frame of the launch takes the binned
    stage's edge instantiations (k_bin_curv<*, true>, the binned k_select<true>)"""
    frames = _selection_frames(n_rows, "rowmajor")
    dense = next(c for c in fc.cases(n_rows) if c.name == "dense")
    big = fc.binned(dense)
    assert len(big) > fc.BINNED_POINTS
    frames.insert(1, ("dense, padded", big, None, ref.extract_planes(big, n_rows)))
    _run_selection(dev, n_rows, frames, (n_rows, "binned"))


@pytest.mark.parametrize("n_rows", [16, 64])
def test_edge_selection_of_wide_points(dev, n_rows):
    """points 4097 floats apart: no wave kernel runs, k_feat_chunk<*, true> (not its flagged
    twin) does every chunk -- the rows of every length and the non-finite rows"""
    frames = []
    for name, pts, keep, y in _selection_frames(n_rows, "rowmajor"):
        if name.startswith("lengths") or name in ("nonfinite", "empty"):
            wide = np.full((len(pts), 4097), 7.0, F32)
            wide[:, :3] = pts
            frames.append((name, wide, keep, y))
    assert len(frames) >= 3
    _run_selection(dev, n_rows, frames, (n_rows, "wide"))


# ------------------------------------------------------------------------------- line table
def _edge_batch(dev, frames, extra_rows=0):
    import ssf
    xyzi = np.concatenate([fr for _, fr in frames] + [np.zeros((extra_rows, 4), F32)]).astype(F32)
    counts = [len(fr) for _, fr in frames]
    off, h_off = ssf.frame_offsets(counts, dev)
    return ssf.PlaneBatch(torch.from_numpy(xyzi).to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), off, h_off,
                          max(counts))


def _table(dev, fe, frames, out=None):
    eb = _edge_batch(dev, frames)
    line, valid = fe.edge_table(eb, out=out)
    torch.cuda.synchronize()
    return line.cpu().numpy(), valid.cpu().numpy(), [int(v) for v in eb.h_off]


@pytest.mark.parametrize("batch", ec.line_batches(), ids=lambda b: b.name)
def test_edge_table_against_yardstick(dev, batch, capsys):
    import ssf
    fe = ssf.Frontend(64, device=dev.index or 0)
    fe.edge_config(max_nn_d2=batch.max_nn_d2, line_ratio=batch.line_ratio)
    line, valid, h = _table(dev, fe, batch.frames)
    worst, unclear, cen, signs = 0.0, 0, 0, []
    for f, (fname, fr) in enumerate(batch.frames):
        y = ec.yardstick_table(fname, fr, batch.max_nn_d2, batch.line_ratio)
        L, V = line[h[f]:h[f + 1]], valid[h[f]:h[f + 1]]
        bad, st = ec.compare_table(L, V, y, batch.max_nn_d2, batch.exact, ec.always_asserted(fname))
        assert not bad, (batch.name, fname, bad)
        worst, unclear, cen = max(worst, st["worst_dir"]), unclear + st["unclear_ratio"], cen + st["cen_differs"]
        signs += [(fname,) + s for s in st["signs"]]
    line2, valid2, _ = _table(dev, fe, batch.frames)
    assert np.array_equal(line2.view(np.uint32), line.view(np.uint32)) and np.array_equal(valid2, valid)
    with capsys.disabled():
        print(f"\n  {batch.name}: worst device-to-yardstick direction gap {worst:.3g} (bar {ec.DIR_TOL:.3g}), {cen} centroid "
              f"rows one float off, {unclear} rows with an unasserted ratio test; open signs (frame, row, device, "
              f"yardstick): {signs[:6]}")


def test_edge_table_around_an_empty_frame(dev):
    """the 8193-edge frame (global memory), a 6-edge frame, an empty frame and a 1025-edge frame
    in one launch: with the empty frame taken out the others' rows and valid bytes keep their
    bits, and rows past the last frame of a larger buffer are never written"""
    import ssf
    batch = next(b for b in ec.line_batches() if b.name == "mixed")
    fe = ssf.Frontend(64, device=dev.index or 0)
    fe.edge_config(max_nn_d2=batch.max_nn_d2, line_ratio=batch.line_ratio)
    total = sum(len(fr) for _, fr in batch.frames)
    out = (torch.full((total + 8, 6), 7.5, dtype=torch.float32, device=dev),
           torch.full((total + 8,), 0x5a, dtype=torch.uint8, device=dev))
    line, valid, h = _table(dev, fe, batch.frames, out=out)
    assert line.shape[0] == total + 8 and np.all(line[total:] == 7.5) and np.all(valid[total:] == 0x5a)
    assert not np.any(line[:total] == 7.5) and set(np.unique(valid[:total]).tolist()) <= {0, 1}
    full = [fr for fr in batch.frames if len(fr[1])]
    assert len(full) == len(batch.frames) - 1 and h[2] == h[3]                      # the empty one is frame 2
    line2, valid2, h2 = _table(dev, fe, tuple(full))
    assert h2 == h[:3] + h[4:]
    assert np.array_equal(line2.view(np.uint32), line[:total].view(np.uint32)) and np.array_equal(valid2, valid[:total])
