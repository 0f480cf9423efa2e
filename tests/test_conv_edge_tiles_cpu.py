"""The edge-strip tiling (tests/conv_edge_geometry.py, the restatement of csrc/fvit_conv.h's edge_tiling / tile_pos) and the count of the band kernel's
column groups that hold a real position.  CPU only; tests/test_gpu_conv_edge_tiles.py checks the restatement against the tile counts the driver reports."""
import pytest

from tests import conv_edge_geometry as G

HEIGHTS = [1, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 56, 57]


@pytest.mark.parametrize("H", HEIGHTS)
def test_the_strip_never_adds_tiles_and_every_other_width_is_tiled_as_before(H):
    for W in range(1, 65):
        before, after = G.tiles_per_image(H, W, 0), G.tiles_per_image(H, W, 1)
        assert before == -(-W // 16) * -(-H // 8)
        if 1 <= W % 16 <= 8 and H > 8:
            assert G.tiling(H, W, 1) == (W // 16, -(-H // 8), -(-H // 16)) and after < before, (H, W)
        else:
            assert G.tiling(H, W, 1) == G.tiling(H, W, 0) and after == before, (H, W)


@pytest.mark.parametrize("edge", [0, 1])
@pytest.mark.parametrize("H", HEIGHTS)
def test_every_pixel_belongs_to_exactly_one_tile(H, edge):
    for W in range(1, 65):
        tiles = G.tile_pixels(H, W, edge)
        assert len(tiles) == G.tiles_per_image(H, W, edge) and all(tiles), (H, W)          # no empty tile
        seen = [p for t in tiles for p in t]
        assert len(seen) == H * W and set(seen) == {(y, x) for y in range(H) for x in range(W)}, (H, W)


def test_the_shapes_the_gpu_tests_use():
    assert G.tiles_per_image(56, 56, 0) == 28 and G.tiles_per_image(56, 56) == 21 + 4
    assert G.tiling(24, 24) == (1, 3, 2) and G.tiling(13, 21) == (1, 2, 1) and G.tiling(20, 8) == (0, 3, 2) and G.tiling(16, 17) == (1, 2, 1)
    assert G.tiling(9, 25) == (2, 2, 0)                                                      # Wr = 9: no strip
    assert G.tiling(8, 24) == (2, 1, 0)                                                      # one tile row: a strip tile would save nothing


def test_band_groups():
    assert G.band_geometry(28, 28) == (7, 4, 13)
    assert G.band_geometry(14, 14) == (14, 1, 14) and G.band_geometry(7, 30) == (7, 1, 14)
    for W in range(1, 31):
        for H in range(1, 60):
            rows, bands, groups = G.band_geometry(H, W)
            assert 1 <= groups <= 14 and rows * bands >= H
            assert (rows - 1) * (W + 2) + W - 1 < groups * 16                                # the last real position is inside the last group kept
