"""CPU check of the result-tile liveness rule of the products with R (mpse_plans.h out_tile_live): a 64 x 64 tile of the
(a, sigma) x l result against the structural mask of the centre, bytes [(column / 64) * pitch + a / 16] over rows a and
columns (sigma, l) - against the same rule stated element by element in numpy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_outmask") / "libplan_emu_outmask.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(REPO, "tests", "host_emu", "plan_emu_outmask.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.emu_out_tiles_live.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.emu_grouped_plan_outmask.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(C.c_longlong)]
    return lib


def _live(emu, mask, d, Dr, M):
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    out = np.zeros(((M + 63) // 64, (Dr + 63) // 64), dtype=np.uint8)
    emu.emu_out_tiles_live(mask.ctypes.data, mask.shape[1], d, Dr, M, out.ctypes.data)
    return out.astype(bool)


def _reference(mask, d, Dr, M):
    """element (a, sigma, l) is read iff the byte of its 16 x 64 block is set; a tile is live iff it holds such an element"""
    Dl = M // d
    a, sg, l = np.meshgrid(np.arange(Dl), np.arange(d), np.arange(Dr), indexing="ij")
    read = mask[(sg * Dr + l) // 64, a // 16] != 0                                 # (Dl, d, Dr)
    rows = read.reshape(M, Dr)
    tm, tn = (M + 63) // 64, (Dr + 63) // 64
    pad = np.zeros((tm * 64, tn * 64), dtype=bool)
    pad[:M, :Dr] = rows
    return pad.reshape(tm, 64, tn, 64).any(axis=(1, 3))


# (Dl, d, Dr): 4, 8, 2 values of a per tile; 64 % d != 0; a tile inside one a; tiles across a 16-row boundary of the
# mask (d = 24: a = 13 .. 16 in tile 5); a ragged last tile row and a last tile column past Dr
SHAPES = [(256, 16, 256), (256, 8, 512), (128, 32, 512), (320, 12, 256), (32, 128, 128), (64, 24, 64), (48, 4, 192),
          (40, 10, 96), (16, 1, 64)]


@pytest.mark.parametrize("Dl,d,Dr", SHAPES)
def test_out_tile_live_matches_elementwise_rule(emu, Dl, d, Dr):
    rng = np.random.default_rng(7 + Dl + d + Dr)
    assert (d * Dr) % 64 == 0                      # (the vector kernels' mask needs whole 64-element column tiles)
    nkt, ntn = (Dl + 15) // 16, d * Dr // 64
    pitch = ((nkt + 7) // 8) * 8
    for density in (0.0, 0.03, 0.5, 1.0):
        mask = np.zeros((ntn, pitch), dtype=np.uint8)
        mask[:, :nkt] = rng.random((ntn, nkt)) < density
        got, want = _live(emu, mask, d, Dr, Dl * d), _reference(mask, d, Dr, Dl * d)
        assert np.array_equal(got, want), (density, np.argwhere(got != want)[:5])
        if density == 0.0:
            assert not got.any()
        if density == 1.0:
            assert got.all()


def test_two_sector_pattern_half_dead(emu):
    """two bond sectors cut at a tile edge: the tiles with q(a) != q(l) are dead, half of them"""
    Dl, d, Dr, cut = 256, 16, 256, 128
    sec_l, sec_r = np.arange(Dl) >= cut, np.arange(Dr) >= cut
    allowed = np.broadcast_to(sec_l[:, None, None] == sec_r[None, None, :], (Dl, d, Dr)).reshape(Dl, d * Dr)
    mask = allowed.reshape(Dl // 16, 16, d * Dr // 64, 64).any(axis=(1, 3)).T.astype(np.uint8)     # [tn][kt]
    pitch = ((Dl // 16 + 7) // 8) * 8
    full = np.zeros((mask.shape[0], pitch), dtype=np.uint8)
    full[:, :mask.shape[1]] = mask
    live = _live(emu, full, d, Dr, Dl * d)
    want = (np.arange(Dl * d // 64)[:, None] * 64 // d >= cut) == (np.arange(Dr // 64)[None, :] * 64 >= cut)
    assert np.array_equal(live, want) and live.sum() * 2 == live.size


def test_grouped_plan_orders_a_masked_launch(emu):
    """a launch that takes the result mask records its dead tiles in the launch order: ordered whatever its size"""
    out = (C.c_longlong * 4)()
    for M, N, split2 in ((4096, 512, 0), (4096, 256, 1), (2048, 512, 0)):
        emu.emu_grouped_plan_outmask(M, N, 96, split2, 256, 0, out)
        plain = list(out)
        emu.emu_grouped_plan_outmask(M, N, 96, split2, 256, 1, out)
        masked = list(out)
        assert masked[0] == 1 and masked[1] == 0 and masked[2:] == plain[2:]
        if split2:
            assert masked == plain
