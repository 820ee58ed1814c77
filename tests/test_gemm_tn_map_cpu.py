"""The chunk-major workgroup map of the split-K TN GEMM launches, by the
library's own query (dgx_gemm_lds_tn_map: the function the kernel decodes its
block id with, compiled for the host). No GPU."""
import pytest

from _gemm_ref import EINVAL


def _lib():
    from dgx import _native
    return _native.lib()


def _grids(tiles):
    """(row tiles, column tiles) factorisations of a tile count: one row, one
    column, and the most square one (odd row counts end in a 1-row group)."""
    sq = max(d for d in range(1, int(tiles ** 0.5) + 1) if tiles % d == 0)
    return sorted({(tiles, 1), (1, tiles), (sq, tiles // sq), (tiles // sq, sq)})


def test_map_is_a_bijection_and_keeps_chunks_on_one_xcd():
    """For every tiles <= 40 and slabs <= 40: each (chunk, tile) is computed by
    exactly one workgroup; and when the XCDs' ranges are whole chunks (slabs a
    multiple of 8) all workgroups of a chunk have one id % 8, i.e. one XCD."""
    L = _lib()
    for tiles in range(1, 41):
        for ni, nj in _grids(tiles):
            for slabs in range(1, 41):
                n = tiles * slabs
                got = [L.dgx_gemm_lds_tn_map(i, ni, nj, slabs) for i in range(n)]
                assert sorted(got) == list(range(n)), (ni, nj, slabs)
                if n % (8 * tiles) == 0:
                    xcd = {}
                    for i, q in enumerate(got):
                        xcd.setdefault(q // tiles, set()).add(i % 8)
                    assert all(len(v) == 1 for v in xcd.values()), (ni, nj, slabs)
                    # and every XCD takes the same number of chunks
                    assert sorted(list(v)[0] for v in xcd.values()) == sorted(list(range(8)) * (slabs // 8))


def test_map_keeps_the_two_row_tile_groups_inside_a_chunk():
    """conv5's grid (8 x 4 tiles, 16 chunks): consecutive workgroups of an XCD
    walk a chunk in 2 x 2 squares of tiles, chunk after chunk."""
    L = _lib()
    ni, nj, slabs = 8, 4, 16
    seq = [L.dgx_gemm_lds_tn_map(x, ni, nj, slabs) for x in range(0, ni * nj * slabs, 8)]   # XCD 0, in dispatch order
    assert [q // (ni * nj) for q in seq] == [0] * (ni * nj) + [1] * (ni * nj)      # chunk 0, then chunk 1
    tile = [divmod(q % (ni * nj), nj) for q in seq[:4]]
    assert tile == [(0, 0), (1, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("args", [(-1, 1, 1, 1), (1, 1, 1, 1), (0, 0, 1, 1), (0, 1, 0, 1), (0, 1, 1, 0),
                                  (0, 1 << 16, 1 << 16, 1)])
def test_map_rejects_ids_and_grids_out_of_range(args):
    assert _lib().dgx_gemm_lds_tn_map(*args) == EINVAL
