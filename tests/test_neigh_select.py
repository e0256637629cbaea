"""The tile and the grid rule of the neighbourhood shrinkage (csrc/ndwt_select.h: neigh_tx, neigh_ty, neigh_geometry) without a GPU,
through tests/select/neigh_shim.cpp: both sides of every condition.

  tile           256 positions of axis 0 below 3 filtered axes; 64 x 16 with 3 -- 64 x 8 for elements of 16 bytes, and for elements of 8
                 bytes at radius 3
  tiles          ceil(n0 / TX) x ceil(n1 / TY); one filtered axis or two: no tiles along axis 1
  chunks         the march is split only while the launch has fewer workgroups than kNeighRounds per compute unit; target_blocks > 0
                 stands in for that count; never chunks of fewer than 2r + 1 planes; one filtered axis: one chunk
  cover          the chunks cover the marched axis exactly, the last one may be short
"""
import pytest

from neigh_cases import BIG, geometry, neigh_shim

CUS = 256


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return neigh_shim(tmp_path_factory)


def test_the_tile(shim):
    assert [shim.sel_neigh_tx(nd) for nd in (1, 2, 3)] == [256, 256, 64]
    for eb in (4, 8, 16):
        for r in (1, 2, 3):
            assert shim.sel_neigh_ty(1, eb, r) == 1 and shim.sel_neigh_ty(2, eb, r) == 1
    assert [shim.sel_neigh_ty(3, 4, r) for r in (1, 2, 3)] == [16, 16, 16]
    assert [shim.sel_neigh_ty(3, 8, r) for r in (1, 2, 3)] == [16, 16, 8]      # both sides of r < 3
    assert [shim.sel_neigh_ty(3, 16, r) for r in (1, 2, 3)] == [8, 8, 8]
    assert shim.sel_neigh_rounds() == 8
    # a workgroup's 256 threads cover the tile in whole passes of whole rows
    for nd in (1, 2, 3):
        for eb in (4, 8, 16):
            for r in (1, 2, 3):
                tx, ty = shim.sel_neigh_tx(nd), shim.sel_neigh_ty(nd, eb, r)
                assert 256 % tx == 0 and ty % (256 // tx) == 0
                # the LDS of an instance: the haloed tile of elements and, with 3 axes, the rows of window sums in double -- far below 64 KB
                lds = (2 if nd < 3 else 1) * (tx + 2 * r) * ((ty + 2 * r) if nd == 3 else 1) * eb + ((ty + 2 * r) * tx * 8 if nd == 3 else 0)
                assert lds <= 24 * 1024, (nd, eb, r, lds)


def test_the_tiles_of_an_item(shim):
    g = lambda nd, dims, eb=4, r=1, blocks=1 << 20: geometry(shim, nd, dims, eb, r, blocks, CUS, 0)
    assert g(1, [256])[:2] == (1, 1) and g(1, [257])[:2] == (2, 1) and g(1, [7])[:2] == (1, 1) and g(1, [4096])[:2] == (16, 1)
    assert g(2, [256, 999])[:2] == (1, 1) and g(2, [257, 3])[:2] == (2, 1) and g(2, [511, 3])[:2] == (2, 1) and g(2, [513, 3])[:2] == (3, 1)
    assert g(3, [64, 16, 3])[:2] == (1, 1) and g(3, [65, 16, 3])[:2] == (2, 1) and g(3, [64, 17, 3])[:2] == (1, 2) and g(3, [127, 31, 3])[:2] == (2, 2)
    assert g(3, [64, 16, 7], 16)[:2] == (1, 2) and g(3, [64, 16, 7], 8, 3)[:2] == (1, 2) and g(3, [64, 16, 7], 8, 2)[:2] == (1, 1)   # the tile of 64 x 8
    assert g(3, [512, 512, 512])[:2] == (8, 32)


def test_one_filtered_axis_has_one_chunk(shim):
    for target in (0, 1, BIG):
        for n in (3, 256, 1 << 20):
            assert geometry(shim, 1, [n], 4, 1, 1, CUS, target)[2:] == (1, 1)


def test_the_march_is_split_only_while_the_launch_is_small(shim):
    want = CUS * 8
    # 512^3 float at level 1: 8 x 32 tiles x 8 bands = 2048 workgroups = 8 per compute unit: one chunk; one band fewer: two chunks
    assert geometry(shim, 3, [512, 512, 512], 4, 1, 8, CUS, 0)[2:] == (512, 1)
    assert geometry(shim, 3, [512, 512, 512], 4, 1, 7, CUS, 0)[2:] == (256, 2)
    assert geometry(shim, 3, [512, 512, 512], 4, 1, 8, CUS // 2, 0)[2:] == (512, 1)       # fewer compute units want fewer workgroups
    assert geometry(shim, 3, [512, 512, 512], 4, 1, 8, 2 * CUS, 0)[2:] == (256, 2)
    # 64 images of 512 x 512: 2 tiles x 4 bands x 64 = 512 workgroups: 4 chunks of 128 rows
    assert geometry(shim, 2, [512, 512], 4, 1, 4 * 64, CUS, 0) == (2, 1, 128, 4)
    # exactly enough, and one tile short of it
    assert geometry(shim, 2, [256, 100], 4, 1, want, CUS, 0)[2:] == (100, 1)
    assert geometry(shim, 2, [256, 100], 4, 1, want - 1, CUS, 0)[2:] == (50, 2)
    # more workgroups than wanted already: one chunk
    assert geometry(shim, 2, [256, 100], 4, 1, 10 * want, CUS, 0)[2:] == (100, 1)


def test_a_chunk_never_has_fewer_planes_than_the_window(shim):
    for r in (1, 2, 3):
        w = 2 * r + 1
        for nd in (2, 3):
            dims = lambda nm: [8, nm] if nd == 2 else [8, 8, nm]
            assert geometry(shim, nd, dims(w), 4, r, 1, CUS, BIG)[2:] == (w, 1)              # the axis is one window: one chunk
            assert geometry(shim, nd, dims(2 * w - 1), 4, r, 1, CUS, BIG)[2:] == (2 * w - 1, 1)   # one plane short of two windows
            assert geometry(shim, nd, dims(2 * w), 4, r, 1, CUS, BIG)[2:] == (w, 2)
            assert geometry(shim, nd, dims(3 * w + 2), 4, r, 1, CUS, BIG)[2:] == (w + 1, 3)  # the shape of the GPU tests: chunks of w + 1, w + 1, w
            c = 1000 // w                                         # as many chunks as windows fit
            assert geometry(shim, nd, dims(1000), 4, r, 1, CUS, BIG)[2:] == (-(-1000 // c), -(-1000 // -(-1000 // c)))


def test_target_blocks_stands_in_for_the_count(shim):
    assert geometry(shim, 3, [64, 16, 100], 4, 1, 1, CUS, 1)[2:] == (100, 1)
    assert geometry(shim, 3, [64, 16, 100], 4, 1, 1, CUS, 2)[2:] == (50, 2)
    assert geometry(shim, 3, [64, 16, 100], 4, 1, 1, CUS, 3)[2:] == (34, 3)                  # the last chunk is short: 34 + 34 + 32
    assert geometry(shim, 3, [64, 16, 100], 4, 1, 1, CUS, 0) == geometry(shim, 3, [64, 16, 100], 4, 1, 1, CUS, -5)   # none: the default count
    assert geometry(shim, 3, [64, 16, 100], 4, 1, 4, CUS, 8)[2:] == (50, 2)                  # the count is of all workgroups of the launch
    assert geometry(shim, 3, [64, 16, 100], 4, 1, 1, CUS, 0)[2:] == (4, 25)                  # 2048 wanted, 33 windows fit: ceil(100 / 33) = 4


def test_the_chunks_cover_the_axis_exactly(shim):
    for nm in (3, 4, 5, 6, 7, 11, 17, 23, 100, 101, 511, 512):
        for r in (1, 2, 3):
            if nm < 2 * r + 1:
                continue
            for target in (0, 1, 2, 3, 5, 64, BIG):
                for blocks in (1, 3, 8):
                    _, _, chunk, nchunks = geometry(shim, 3, [70, 20, nm], 4, r, blocks, CUS, target)
                    assert chunk >= 1 and nchunks >= 1 and nchunks * chunk >= nm and (nchunks - 1) * chunk < nm
                    assert chunk >= min(nm, 2 * r + 1)
