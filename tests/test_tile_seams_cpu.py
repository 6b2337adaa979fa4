"""CPU: the tile-seam cases of the ICP, plane, correspondence and grid GPU tests, looked at on the references alone -- no GPU and no
library -- to show that the GPU assertions bite.

The two-level kernels reduce tiles of 1 024 rows and then walk the tiles with a strided loop.  A wrong stride or pitch loses or
repeats a tile; an unwritten partial is a word that is read and was never written.  What the GPU tests can see of either:
  (a) the workspace fill: 0xA5 bytes read as a double are about -2^-421, which no sum would show; 0xFF bytes are NaN;
  (b) a lost tile: without the rows of tile 8, or of tile 16, the reference's integer count changes (the GPU tests hold counts to
      equality) and at least one fp64 sum moves by more than 1000 times the bound the GPU tests allow, count * 2^-52 * sum |term|;
  (c) every tile below each cloud's count holds a row that contributes, so no tile's partial is zero by accident;
  (d) the grid test's four M give 16, 64, 128 and 256 slot tiles: 1, 1, 2 and 4 steps of the 64-wide scan with a carry."""
import numpy as np

import corr_ransac_ref as C
import grid_knn_ref as R
import icp_ref as I
import plane_ref as P
import test_corr_ransac_gpu as TC
import test_grid_knn_gpu as TG
import test_icp_gpu as TI
import test_plane_gpu as TP

TILE = 1024
N = 16385                                                          # 17 tiles: tiles 8 and 16 are chunk 0's second and third trip


def test_the_two_fills_read_as_doubles_floats_and_integers():
    a5, ff = np.full(8, 0xA5, np.uint8), np.full(8, 0xFF, np.uint8)
    assert 0 < abs(a5.view(np.float64)[0]) < 1e-100 and 0 < abs(a5.view(np.float32)[0]) < 1e-15          # invisible in any sum
    assert np.isnan(ff.view(np.float64)[0]) and np.isnan(ff.view(np.float32)).all()
    assert ff.view(np.int64)[0] == -1 and (ff.view(np.int32) == -1).all()
    assert np.isnan(1.0 + ff.view(np.float64)[0])                    # one such word poisons the sum it enters


def assert_tiles_are_seen(rows, terms, n, what):
    """rows int64 [m]: the row each term comes from; terms [m, W] fp64: what the reference adds up for one cloud of count n."""
    tiles = -(-n // TILE)
    assert set((rows // TILE).tolist()) == set(range(tiles)), what            # (c)
    count = len(np.unique(rows))
    sums, bound = terms.sum(0), count * 2.0 ** -52 * np.abs(terms).sum(0)
    seen = 0
    for tile in (8, 16):
        if tile >= tiles:
            continue
        keep = rows // TILE != tile
        assert len(np.unique(rows[keep])) != count, what             # (b) the count, held to equality
        moved = np.abs(terms[keep].sum(0) - sums)
        print("%s, without tile %d: the sums move by up to %.3g times the bound" % (what, tile, (moved / np.maximum(bound, 1e-300)).max()))
        assert (moved > 1000.0 * bound).any(), what                  # (b) a sum, by far more than the bound
        seen += 1
    return seen


def test_icp_a_lost_tile_is_seen_and_every_tile_contributes():
    src, tgt, normals, n_src, T = TI.seam_case(N)
    m = np.float32(0.15 ** 2)
    zeros = np.zeros(3, np.int32)
    ev = I.icp_step(src, tgt, None, T, zeros, zeros, m, 0.0, R.default_cell(m), I.POINT, flags=I.EVAL_ONLY, n_src=n_src)
    seen = 0
    for metric in (I.PLANE, I.POINT):
        for b in range(3):
            n = int(n_src[b])
            t, rows, part = I.step_terms(I.transform(T[b], src[b, :n]), tgt[b], normals[b], ev["corr"][b, :n], metric)
            if metric == I.POINT:
                assert np.array_equal(t.sum(0), ev["sums"][b]) and part.sum() == ev["count"][b]       # the terms icp_step itself adds up
            seen += assert_tiles_are_seen(rows, t, n, "ICP metric %d cloud %d" % (metric, b))
    assert seen == 2 * 3                                             # cloud 0: tiles 8 and 16; cloud 2: tile 8; cloud 1 ends at tile 8


def test_plane_a_lost_tile_is_seen_and_every_tile_contributes():
    pts, counts, assign, H, seed = TP.seam_case(N)
    ref = P.fit_plane(pts, TP.THR, H, seed, n_points=counts, assign=assign.copy())
    assert (ref["status"] == 0).all()
    seen = 0
    for b in range(3):
        n = int(counts[b])
        inl = P.inliers(pts[b], n, assign[b], ref["plane0"][b], TP.THR)          # the first refit round's inliers
        seen += assert_tiles_are_seen(np.flatnonzero(inl), P.refit_terms(pts[b], inl, ref["plane0"][b]), n, "plane cloud %d" % b)
    assert seen == 3


def test_correspondences_a_lost_tile_is_seen_and_every_tile_contributes():
    counts, seed = TC.SEAM_CASES[N]
    c = TC.sized_case(N)
    ref = C.ransac(c["src"], c["tgt"], c["ps"], c["pt"], TC.THR, TC.SEAM_H, seed, 0.9, list(counts))
    assert (ref["status"] == 0).all() and np.array_equal(ref["best_count"], TC.true_pairs(counts))
    seen = 0
    for b in range(3):
        n = int(counts[b])
        inl, p, q, dd = C.inliers(c["src"][b], c["tgt"][b], c["ps"][b], c["pt"][b], n, ref["T"][b], TC.THR)
        seen += assert_tiles_are_seen(np.flatnonzero(inl), C.refit_terms(p[inl], q[inl], dd[inl]), n, "correspondences cloud %d" % b)
    assert seen == 3


def slot_capacity(rows):
    """csrc/slot_table.h: the power of two >= 2 * rows, and >= 64."""
    return 64 if rows <= 32 else 1 << (2 * rows - 1).bit_length()


def test_the_grid_sizes_give_16_64_128_and_256_slot_tiles():
    assert [slot_capacity(r) for r in (0, 1, 32, 33, 4095, 4096, 4097)] == [64, 64, 64, 128, 8192, 8192, 16384]       # the header's own asserts
    tiles = [slot_capacity(M) // TILE for _, M in TG.DISC_SIZES]
    assert tiles == [16, 64, 128, 256] and [-(-t // 64) for t in tiles] == [1, 1, 2, 4]
    assert slot_capacity(3000) // TILE == 8                          # the largest table of the suite before these sizes
    assert slot_capacity(32769) // TILE == 128                       # the K = 1 walk of tests/test_icp_gpu.py
