"""The VAE's tile plan (vae_api.hip vae_tile_plan), asked without a device through the diagnostics export s2v_diag_vae_tile_plan: whether a call
tiles, and for every tile in raster order its input window, output size, blend extents against the tile above / to the left, crop and paste
offset, plus the size of the whole output -- for the tiled decode (latents in, pixels out) and the tiled encode (pixels in, latents out).
The expected plans are built here from the reference's rule as the oracle writes it: oracle/vae_ref.py tile_geometry / encode_tile_geometry
(the int() truncations) and the range(0, n, overlap) loops, slices, blends and crops of decode_tiled / encode_tiled.  A tile's output is
in * scale decoding and in // scale encoding (the library refuses an encode whose tile sides are no multiples of the scale; the plan itself is
defined for every size)."""
import ctypes

import pytest

from oracle import vae_ref

TINY = dict(block_out_channels=(16, 16, 32, 32), sample_height=96, sample_width=160)  # the tiny config of the GPU tests
REAL = dict(block_out_channels=(128, 256, 256, 512), sample_height=480, sample_width=720)
FIELDS = ("y", "x", "h", "w", "oh", "ow", "bv", "bh", "ch", "cw", "py", "px")  # Tile (vae_api.hip)
MAX_TILES = 4096


@pytest.fixture(scope="module")
def diag(s2v):
    L = s2v._lib.diag_lib()
    L.s2v_diag_vae_tile_plan.argtypes = [ctypes.c_int32] * 7 + [ctypes.POINTER(ctypes.c_int32)] * 2 + [ctypes.c_int32]
    return L


def plan(L, cfg, encode, H, W, tiling=1):
    head, tiles = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * (12 * MAX_TILES))()
    rc = L.s2v_diag_vae_tile_plan(cfg["sample_height"], cfg["sample_width"], len(cfg["block_out_channels"]), int(encode), H, W, tiling, head,
                                  tiles, MAX_TILES)
    assert rc == 0, L.s2v_last_error()
    tiled, rows, cols, out_h, out_w = head
    return dict(tiled=bool(tiled), rows=rows, cols=cols, out_h=out_h, out_w=out_w,
                tiles=[dict(zip(FIELDS, tiles[12 * k:12 * k + 12])) for k in range(rows * cols)])


def geometry(cfg, encode):
    """(input-side tile, overlap, blend extent, crop limit) per axis and the scale, from the oracle's two geometry functions"""
    sc = 2 ** (len(cfg["block_out_channels"]) - 1)
    tg = vae_ref.encode_tile_geometry(cfg) if encode else vae_ref.tile_geometry(cfg)
    tin = (tg["ts_h"], tg["ts_w"]) if encode else (tg["tl_h"], tg["tl_w"])
    return tin, (tg["ov_h"], tg["ov_w"]), (tg["bl_h"], tg["bl_w"]), (tg["lim_h"], tg["lim_w"]), sc


def expected(cfg, encode, H, W, tiling=1):
    """decode() / decode_tiled() and encode_moments() / encode_tiled() of the oracle with the tensors replaced by their shapes"""
    (tin_h, tin_w), (ov_h, ov_w), (bl_h, bl_w), (lim_h, lim_w), sc = geometry(cfg, encode)
    out = (lambda n: n // sc) if encode else (lambda n: n * sc)
    if not (tiling and (W > tin_w or H > tin_h)):
        one = dict(y=0, x=0, h=H, w=W, oh=out(H), ow=out(W), bv=0, bh=0, ch=out(H), cw=out(W), py=0, px=0)
        return dict(tiled=False, rows=1, cols=1, out_h=out(H), out_w=out(W), tiles=[one])
    rows = []
    for i in range(0, H, ov_h):
        rows.append([dict(y=i, x=j, h=len(range(H)[i:i + tin_h]), w=len(range(W)[j:j + tin_w])) for j in range(0, W, ov_w)])
    py = 0
    for i, row in enumerate(rows):
        px = 0
        for j, t in enumerate(row):
            t["oh"], t["ow"] = out(t["h"]), out(t["w"])
            t["bv"] = min(rows[i - 1][j]["oh"], t["oh"], bl_h) if i > 0 else 0  # _blend_v: ext = min(a.shape[3], b.shape[3], ext)
            t["bh"] = min(row[j - 1]["ow"], t["ow"], bl_w) if j > 0 else 0
            t["ch"], t["cw"] = len(range(t["oh"])[:lim_h]), len(range(t["ow"])[:lim_w])  # tile[:, :, :, :lim_h, :lim_w]
            t["py"], t["px"] = py, px
            px += t["cw"]  # torch.cat(res, dim=4)
        py += row[0]["ch"]  # torch.cat(res_rows, dim=3)
    return dict(tiled=True, rows=len(rows), cols=len(rows[0]), out_h=py, out_w=px, tiles=[t for row in rows for t in row])


def check(L, cfg, encode, H, W, tiling=1):
    got, exp = plan(L, cfg, encode, H, W, tiling), expected(cfg, encode, H, W, tiling)
    assert got == exp, (encode, H, W, tiling)
    # the crops tile the output exactly: every row of tiles is as wide as the output, the rows stack to its height
    t, cols = got["tiles"], got["cols"]
    for r in range(got["rows"]):
        assert sum(x["cw"] for x in t[r * cols:(r + 1) * cols]) == got["out_w"], (encode, H, W, r)
    assert sum(t[r * cols]["ch"] for r in range(got["rows"])) == got["out_h"], (encode, H, W)
    return got


@pytest.mark.parametrize("encode", [False, True], ids=["decode", "encode"])
def test_tiny_config_every_window(diag, encode):
    """every window from 1 x 1 to two past three overlaps plus a tile in each axis: untiled, the threshold, every ragged last tile"""
    (tin_h, tin_w), (ov_h, ov_w), _, _, _ = geometry(TINY, encode)
    tiled = 0
    for H in range(1, 3 * ov_h + tin_h + 3):
        for W in range(1, 3 * ov_w + tin_w + 3):
            tiled += check(diag, TINY, encode, H, W)["tiled"]
    assert tiled > 0
    for H, W in ((1, 1), (tin_h, tin_w), (tin_h + 1, tin_w + 1), (3 * ov_h + 1, 3 * ov_w + 1)):  # tiling switched off: one tile whatever the size
        assert not check(diag, TINY, encode, H, W, tiling=0)["tiled"]


def real_sizes(encode):
    (tin_h, tin_w), (ov_h, ov_w), (bl_h, bl_w), _, sc = geometry(REAL, encode)
    unit = sc if encode else 1  # input elements per latent
    below = ((bl_h - 1, bl_w - 1) if encode else ((bl_h - 1) // sc, (bl_w - 1) // sc))  # the largest last tile (in latents) whose output is below the blend extent
    return {"shipped": [(480, 720), (720, 1280)] if encode else [(60, 90), (90, 160)],
            "threshold": [(tin_h + a, tin_w + b) for a in (-1, 0, 1) for b in (-1, 0, 1)],
            "overlap-multiples": [(k * ov_h, m * ov_w) for k in (1, 2, 3) for m in (1, 2, 4)],
            "last-tile-1-wide": [(k * ov_h + 1, m * ov_w + 1) for k in (2, 3) for m in (2, 4)],
            "last-tile-below-blend": [(2 * ov_h + unit * a, 3 * ov_w + unit * b) for a, b in ((1, 1), (2, 3), below)]}


@pytest.mark.parametrize("kind", ["shipped", "threshold", "overlap-multiples", "last-tile-1-wide", "last-tile-below-blend"])
@pytest.mark.parametrize("encode", [False, True], ids=["decode", "encode"])
def test_real_config(diag, encode, kind):
    (tin_h, tin_w), (ov_h, ov_w), (bl_h, bl_w), _, _ = geometry(REAL, encode)
    for H, W in real_sizes(encode)[kind]:
        got = check(diag, REAL, encode, H, W)
        last = got["tiles"][-1]
        if kind == "threshold":
            assert got["tiled"] == (H > tin_h or W > tin_w)
        if kind == "overlap-multiples":
            assert got["rows"] == H // ov_h and got["cols"] == W // ov_w and (last["h"], last["w"]) == (min(ov_h, H), min(ov_w, W))
        if kind == "last-tile-1-wide":
            assert (last["h"], last["w"]) == (1, 1) and (last["oh"], last["ow"]) == ((0, 0) if encode else (8, 8))
        if kind == "last-tile-below-blend":
            assert 0 < last["oh"] < bl_h and 0 < last["ow"] < bl_w and last["bv"] == last["oh"] and last["bh"] == last["ow"]


def test_shipped_sizes_are_the_documented_grids(diag):
    """the two decodes and encodes the pipeline runs: 3 x 3 tiles for 480 x 720, 4 x 5 for 720 x 1280, and the output is the input times / over eight"""
    for (h, w), grid in (((60, 90), (3, 3)), ((90, 160), (4, 5))):
        d, e = plan(diag, REAL, False, h, w), plan(diag, REAL, True, 8 * h, 8 * w)
        assert (d["rows"], d["cols"]) == grid == (e["rows"], e["cols"])
        assert (d["out_h"], d["out_w"]) == (8 * h, 8 * w) and (e["out_h"], e["out_w"]) == (h, w)
