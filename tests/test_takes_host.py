"""CPU: the host queries the non-GEMM entry points decline by (``hsp_*_takes``, ``hsp_gemm_rows_bn_tiles_bf16``; include/hsp.h).
Every row of tests/_takes_cases.py holds -- the last shape taken and the first declined at each limit -- and over the shapes
FaceRecon and the heads reach no query crashes or answers outside its range."""
import pytest

import _takes_cases as tc


def _L():
    from hs_pose_amd._lib import lib
    return lib()


@pytest.mark.parametrize("c", tc.CASES, ids=tc.case_id)
def test_query_answers_its_row(c):
    assert getattr(_L(), c.query)(*c.args) == c.want


@pytest.mark.parametrize("query", tc.QUERIES)
def test_query_over_the_shapes_the_network_reaches(query):
    fn = getattr(_L(), query)
    shapes = tc.sweep(query)
    assert shapes
    for args in shapes:
        got = fn(*args)
        if query == "hsp_gemm_rows_bn_tiles_bf16":
            assert 0 <= got <= 512, f"{query}{args}: {got}"
        else:
            assert got in (0, 1), f"{query}{args}: {got}"


def test_every_takes_query_of_the_header_has_rows():
    """a query declared in include/hsp.h without a row at its limits here would go unchecked"""
    from hs_pose_amd._lib import SIGNATURES
    declared = {n for n in SIGNATURES if n.endswith("_takes") and n != "hsp_gemm_takes"}      # (hsp_gemm_takes: tests/_gemm_cases.py)
    assert declared == set(tc.QUERIES) - {"hsp_gemm_rows_bn_tiles_bf16"}


def test_ops_asks_the_library_once_per_shape():
    """ops._takes keeps its answers: the second question of the same integers does not reach the library"""
    from hs_pose_amd import ops
    ops._takes.cache_clear()
    assert ops._takes("hsp_fps_levels_takes", 12288) and not ops._takes("hsp_fps_levels_takes", 12289)
    assert ops._takes("hsp_fps_levels_takes", 12288)
    info = ops._takes.cache_info()
    assert (info.hits, info.misses) == (1, 2)
