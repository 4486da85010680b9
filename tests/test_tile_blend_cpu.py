"""Tiled VAE -- the parts that need no GPU: every refusal of mdx_tile_blend_f32 (on the host, before any launch), its C
declaration against include/mdx.h, the refusals of AutoencoderKL.enable_tiling, and the numpy restatement the GPU tests compare
against (tests/_tile_util.py) on hand-computed values."""
import ctypes
import os
import re

import numpy as np
import pytest

import _tile_util as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20         # disjoint non-null addresses P, 2P, ...: nothing is dereferenced by a refused call


def _table(values):
    return (ctypes.c_int * len(values))(*values)


def test_blend_argument_validation_without_gpu():
    from minddiffusion_amd import _lib
    lib = _lib.load()

    def call(tiles=P, out=2 * P, off=3 * P, host=(0, 0, 4, 8, 12), ny=1, nx=4, wrap=0, NB=2, C=3, Hc=8, Wc=20, h=8, w=8, ry=4,
             rx=4, mode=0):
        t = None if host is None else _table(host)
        return lib.mdx_tile_blend_f32(tiles, out, off, t, ny, nx, wrap, NB, C, Hc, Wc, h, w, ry, rx, mode, None)

    def refused(msg, **kw):
        assert call(**kw) == -1
        err = lib.mdx_last_error()
        assert b"mdx_tile_blend_f32" in err and msg in err, err

    for name in ("tiles", "out", "off", "host"):
        refused(b"null pointer", **{name: None})
    for kw in ({"NB": 0}, {"C": 0}, {"h": 0}, {"w": -1}, {"ny": 0}, {"nx": 0}, {"Hc": 0}, {"Wc": 0}):
        refused(b"bad extents", **kw)
    refused(b"larger than the canvas", h=9)
    refused(b"larger than the canvas", w=21)
    refused(b"an offset leaves the canvas", host=(0, 0, 4, 8, 13))
    refused(b"an offset leaves the canvas", host=(0, -1, 4, 8, 12))
    refused(b"an offset leaves the canvas", host=(1, 0, 4, 8, 12))
    refused(b"start at 0 and end at L - w", host=(0, 0, 4, 8, 11))
    refused(b"must ascend", host=(0, 0, 8, 4, 12))
    refused(b"uncovered", host=(0, 0, 12), nx=2)
    refused(b"wrap_x must be 0 or 1", wrap=2)
    # the wrapped axis: its own rule
    refused(b"must start at 0", host=(0, 4, 8, 12, 16), wrap=1)
    refused(b"an offset leaves the canvas", host=(0, 0, 8, 16, 20), wrap=1)
    refused(b"uncovered", host=(0, 0, 4, 8, 11), wrap=1)             # 20 - 11 > 8: column 19 lies under no tile
    for kw in ({"ry": 0}, {"rx": 0}, {"ry": -3}, {"ry": 4097}, {"rx": 4097}):
        refused(b"ramps must be in [1, 4096]", **kw)
    for mode in (2, -1):
        refused(b"unknown mode", mode=mode)
    refused(b"out overlaps tiles", out=P + 64)
    refused(b"out overlaps tiles", tiles=2 * P + 64)


def test_the_blend_entry_is_declared_as_the_header_declares_it():
    from minddiffusion_amd import _lib, ops
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.S)
    kinds = {"int": _lib.c_int, "float": _lib.c_float, "mdx_stream_t": _lib.c_void_p}
    name = "mdx_tile_blend_f32"
    args = [a.strip() for a in re.search(rf"\bint {name}\s*\(([^)]*)\)", header).group(1).split(",")]
    res, argtypes = _lib.SIGNATURES[name]
    assert res is _lib.c_int and len(argtypes) == len(args) == 17
    for a, ty in zip(args, argtypes):
        want = _lib.c_void_p if "*" in a else kinds[a.rsplit(" ", 1)[0].replace("const ", "")]
        assert ty is want, (name, a)
    assert args[-1].startswith("mdx_stream_t")
    assert hasattr(_lib.load(), name)
    modes = dict(re.findall(r"\b(MDX_TILE_[A-Z]+) = (\d+)", header))
    assert {k: int(v) for k, v in modes.items()} == {"MDX_TILE_RAW": ops.TILE_MODES["raw"], "MDX_TILE_UNIT": ops.TILE_MODES["unit"]}


def test_python_refusals_of_tile_blend():
    import torch
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    g = ops.WindowGrid((8, 20), (8, 8), (4, 4))
    with pytest.raises(MdxError, match="GPU"):
        ops.tile_blend(torch.zeros(8, 3, 8, 8), g, 4)


def _vae():
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
    return AutoencoderKL(ddconfig=dict(TINY_VAE_DDCONFIG), embed_dim=4, device="cpu")


def test_enable_tiling_refusals_and_state():
    from minddiffusion_amd._lib import MdxError
    vae = _vae()
    assert vae.tiling is None and vae.factor == 2
    for kw in ({"tile": 16, "overlap": 16}, {"tile": 16, "overlap": 17}, {"tile": (16, 8), "overlap": (4, 8)},
               {"tile": 16, "overlap": -1}, {"tile": -16, "overlap": 0}, {"tile": 0, "overlap": 0},
               {"tile": True, "overlap": 0}, {"tile": 16, "overlap": False}, {"tile": 16.0, "overlap": 4},
               {"tile": (16, 16, 16), "overlap": 4}, {"tile": 16, "overlap": 4, "max_tile_batch": 0},
               {"tile": 16, "overlap": 4, "max_tile_batch": True}, {"tile": 16, "overlap": 4, "max_tile_batch": 2.0},
               {"tile": 4096, "overlap": 2049}):
        with pytest.raises(MdxError, match="enable_tiling"):
            vae.enable_tiling(**kw)
        assert vae.tiling is None                                       # a refused call leaves the setting alone
    assert vae.enable_tiling(tile=(16, 24), overlap=(4, 0), max_tile_batch=3) is vae
    assert vae.tiling == {"tile": (16, 24), "overlap": (4, 0), "max_tile_batch": 3}
    vae.enable_tiling()
    assert vae.tiling == {"tile": (64, 64), "overlap": (16, 16), "max_tile_batch": 8}
    assert vae.disable_tiling() is vae and vae.tiling is None


def test_the_tile_grid_of_a_canvas():
    vae = _vae().enable_tiling(tile=16, overlap=4)
    assert vae._tiles_for(16, 16, False) is None and vae._tiles_for(8, 16, True) is None      # fits one tile: the plain path
    t = vae._tiles_for(16, 40, False)
    assert (t["lat"].oy, t["lat"].ox) == ([0], [0, 12, 24]) == ([0], T.offsets(40, 16, 12))
    assert (t["img"].oy, t["img"].ox, t["img"].h, t["img"].w) == ([0], [0, 24, 48], 32, 32)
    assert (t["ramp_lat"], t["ramp_img"]) == ((4, 4), (8, 8)) and t["rows"].host.tolist() == [0, 1, 2]
    t = vae._tiles_for(24, 40, True)
    assert t["lat"].wrap_x and t["lat"].ox == [0, 12, 24, 36] == T.offsets(40, 16, 12, wrap=True) and t["lat"].oy == [0, 8]
    assert t["img"].wrap_x and t["img"].ox == [0, 24, 48, 72] and t["img"].oy == [0, 16]
    t = vae._tiles_for(8, 40, False)                                    # a tile larger than the canvas becomes its extent
    assert (t["lat"].h, t["lat"].w, t["img"].h, t["img"].w) == (8, 16, 16, 32)
    vae.enable_tiling(tile=16, overlap=0)
    assert vae._tiles_for(16, 40, False)["ramp_img"] == (1, 1)
    assert vae.latent_shape((2, 3, 32, 80)) == (2, 4, 16, 40)          # no whole-canvas plan is built for a tiled canvas
    assert not vae.encoder._plans


def test_the_numpy_blend_is_the_stated_arithmetic():
    assert T.ramp(8, 4).tolist() == [1, 2, 3, 4, 4, 3, 2, 1] and T.ramp(8, 8).tolist() == [1, 2, 3, 4, 4, 3, 2, 1]
    assert T.ramp(8, 1).tolist() == [1] * 8 and T.ramp(5, 2).tolist() == [1, 2, 2, 2, 1]
    # two 1 x 4 tiles at x = 0 and 2 on a 1 x 6 canvas, ramp 2: weights 1 2 2 1
    tiles = np.array([[1, 2, 3, 4], [10, 20, 30, 40]], np.float32).reshape(2, 1, 1, 4)
    out, cnt = T.blend_ref(tiles, [0], [0, 2], 1, 6, 1, 2)
    assert cnt.tolist() == [[1, 1, 2, 2, 1, 1]]
    f = np.float32
    want = [f(1), f(2), (f(2) * f(3) + f(1) * f(10)) / f(3), (f(1) * f(4) + f(2) * f(20)) / f(3), f(30), f(40)]
    assert out.dtype == np.float32 and out.reshape(-1).tolist() == [float(v) for v in want]
    unit, _ = T.blend_ref(tiles / f(40), [0], [0, 2], 1, 6, 1, 2, mode="unit")
    raw, _ = T.blend_ref(tiles / f(40), [0], [0, 2], 1, 6, 1, 2)
    assert np.array_equal(unit, np.clip((raw + f(1)) / f(2), 0, 1)) and unit.max() == 1.0
    # wrapped: a tile at 4 on a canvas of 6 covers columns 4 5 0 1
    out, cnt = T.blend_ref(tiles, [0], [0, 4], 1, 6, 1, 1)
    assert cnt.tolist() == [[2, 2, 1, 1, 1, 1]]
    assert out.reshape(-1).tolist() == [(1 + 30) / 2, (2 + 40) / 2, 3, 4, 10, 20]
    assert np.allclose(T.blend_ref64(tiles, [0], [0, 4], 1, 6, 1, 1), out)
