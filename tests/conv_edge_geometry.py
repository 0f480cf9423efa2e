"""The tile and column-group geometry of csrc/fvit_conv.h (edge_tiling, tile_pos) and csrc/fvit_conv_band.hip (band_groups) restated in Python: what tests/test_conv_edge_tiles_cpu.py
reasons about and what tests/test_gpu_conv_edge_tiles.py holds the driver's reported tile counts to.  No GPU, no library.

conv3x3_c64_halo_kernel and stem_fused_kernel tile an H x W map with 8 x 16 tiles.  When the last tile column would hold Wr = W mod 16 in 1 .. 8 real
columns and the map is more than one tile high, those columns are tiled by a strip of transposed 16 x 8 tiles instead (fvit_tune "conv_edge_tiles",
default 1).  conv3x3_c128_band_kernel numbers a band's positions over the padded pitch W + 2 and runs them in 14 groups of 16; ``band_geometry`` says how
many of them hold a real position (13 at 28 x 28: DESIGN section 7 on why the kernel still runs 14)."""
TH, TW = 8, 16
BAND_POSITIONS = 224


def _ceil(a: int, b: int) -> int:
    return (a + b - 1) // b


def strip_applies(H: int, W: int) -> bool:
    return 1 <= W % TW <= TH and _ceil(H, TW) < _ceil(H, TH)


def tiling(H: int, W: int, edge_tiles: int = 1):
    """(tiles_x, tiles_y, strips) per image: tiles_x * tiles_y plain tiles, then ``strips`` strip tiles."""
    if edge_tiles and strip_applies(H, W):
        return W // TW, _ceil(H, TH), _ceil(H, TW)
    return _ceil(W, TW), _ceil(H, TH), 0


def tiles_per_image(H: int, W: int, edge_tiles: int = 1) -> int:
    tx, ty, strips = tiling(H, W, edge_tiles)
    return tx * ty + strips


def tile_pixels(H: int, W: int, edge_tiles: int = 1):
    """For every tile of one image, in the kernels' numbering, the list of map pixels (y, x) it stores."""
    tx, ty, strips = tiling(H, W, edge_tiles)
    out = []
    for t in range(tx * ty + strips):
        if t < tx * ty:
            y0, x0, th, tw = (t // tx) * TH, (t % tx) * TW, TH, TW
        else:
            y0, x0, th, tw = (t - tx * ty) * TW, tx * TW, TW, TH
        out.append([(y, x) for y in range(y0, min(y0 + th, H)) for x in range(x0, min(x0 + tw, W))])
    return out


def band_geometry(H: int, W: int):
    """(rows per band, bands per image, 16-position groups that hold a real position) of the row-band kernel, W <= 30."""
    pw = W + 2
    rows = min(BAND_POSITIONS // pw, H)
    return rows, _ceil(H, rows), _ceil((rows - 1) * pw + W, 16)
