"""CPU: the plan queries of the dense products (hsp_wgrad_plan, hsp_wgrad_pair_plan, hsp_gemm_rows_plan, hsp_gemm_x3_plan,
hsp_gemm_route: host code, the dispatch decides by the same functions).  Every case of tests/_gemm_cases.py enters the plan it was placed for, and the
facts the kernels rely on hold over a sweep of shapes: slices are whole pairs of prefetch groups (16 rows), the
4-slices-per-workgroup form has a multiple of 4 slices, and no plan writes more partial sums than the workspace query of the same
arguments promises -- the pair launch after its shrink loop included.

The workspace sweep found hsp_wgrad_workspace_bytes short for fp32 rows on the x3 form with M an odd multiple of 64 (64 x 512 <-
16448 rows: 65 partials planned, room for 52): the query allowed for the finer cut of the matrix-core forms only where M is a
multiple of 128, and the x3 form takes any M.  test_wgrad_workspace_covers_every_plan holds the corrected rule."""
import ctypes

import pytest

import _gemm_cases as gc


def _L():
    from hs_pose_amd._lib import lib
    return lib()


@pytest.mark.parametrize("c", gc.WGRAD, ids=lambda c: f"{c.entry}-{c.M}x{c.N}x{c.K}-{c.lda}-{c.ldb}-{c.al16}")
def test_wgrad_case_enters_its_plan(c):
    gc.check_wgrad_plan(_L(), c)


@pytest.mark.parametrize("c", gc.WGRAD_DECLINED, ids=lambda c: f"{c.entry}-{c.M}x{c.N}x{c.K}-{c.lda}-{c.ldb}-{c.al16}")
def test_wgrad_case_is_declined_by_its_plan(c):
    assert gc.wgrad_plan(_L(), c)[0] == -2


@pytest.mark.parametrize("p", gc.PAIRS, ids=lambda p: "-".join(str(v) for v in p[:6]))
def test_pair_case_enters_its_plan(p):
    gc.check_pair_plan(_L(), p)


def _gid(c):
    return "-".join(str(v) for v in c[:6]) + f"-a{c.alpha:g}-r{c.rpc}-{c.off}-{int(c.relu)}{c.bn}{c.x3}{c.es}"


@pytest.mark.parametrize("c", gc.ROUTES, ids=_gid)
def test_product_call_goes_to_its_kernel(c):
    """hsp_gemm_route sends every row of ROUTES to the family it names, and that family's own takes function agrees"""
    L, call = _L(), gc.gemm_call(c)
    route = L.hsp_gemm_route(ctypes.byref(call))
    assert route == c.want, f"{c}: route {route}"
    if c.bn and route != gc.X3_BN:                 # the partials declined: the route of the plain call
        call.bn = 0
        assert L.hsp_gemm_route(ctypes.byref(call)) == route
    assert route == gc.NONE or L.hsp_gemm_takes(ctypes.byref(call), route) == 1


def _sweep_K():
    return sorted(set(list(range(1, 20001, 97)) + [k + d for k in range(16, 600, 16) for d in (-1, 0, 1)] + [4112, 16448, 20000]))


def test_wgrad_workspace_covers_every_plan():
    L = _L()
    out = (ctypes.c_int * 4)()
    forms = set()
    for M in range(64, 513, 64):
        for N in range(64, 513, 64):
            unit = (M * N + N) * 4
            for K in _sweep_K():
                ws = L.hsp_wgrad_workspace_bytes(M, N, K)
                # fp32 / bf16 storage; dense and aligned, base pointers off 16 bytes, pitches 2 * odd
                for es, al, lda, ldb in ((4, 1, M, N), (4, 0, M, N), (4, 1, M + 2, N + 2), (2, 1, M, N), (2, 0, M, N), (2, 1, M + 2, N + 2)):
                    assert L.hsp_wgrad_plan(M, N, K, es, al, lda, ldb, 0, out) == 0
                    form, sk, ks, parts = out
                    forms.add(form)
                    assert ks % 16 == 0 and sk * ks >= K, (M, N, K, es, al, lda, list(out))
                    if form == gc.KB4:
                        assert sk % 4 == 0 and sk >= 8 and parts * 4 == sk, (M, N, K, es, al, lda, list(out))
                    else:
                        assert parts == sk and (sk - 1) * ks < K, (M, N, K, es, al, lda, list(out))
                    assert parts * unit <= ws, f"{M} x {N} <- {K} (elem {es}, aligned {al}, lda {lda}): {parts} partials, room for {ws // unit}"
    assert forms == {gc.KB1, gc.KB4, gc.BF16, gc.X3}


def test_ragged_wgrad_workspace_covers_its_plan():
    L = _L()
    out = (ctypes.c_int * 4)()
    for M in (129, 130, 136, 191, 771, 1286, 1289):
        for N in (128, 512, 1024):
            for K in _sweep_K()[::7] + [255, 256, 257]:
                ws = L.hsp_wgrad_workspace_bytes(M, N, K)
                for es, lda, rag, form in ((4, (M + 3) & ~3, 0, gc.X3), (2, (M + 7) & ~7, 1, gc.BF16)):
                    if es == 4 and ((M + 127) // 128) * (N // 128) < 4:
                        assert L.hsp_wgrad_plan(M, N, K, es, 1, lda, N, rag, out) == -2      # ragged fp32 rows: the x3 form or nothing
                        continue
                    assert L.hsp_wgrad_plan(M, N, K, es, 1, lda, N, rag, out) == 0 and out[0] == form
                    assert out[2] % 64 == 0 and out[3] * (M * N + N) * 4 <= ws, (M, N, K, es, list(out))
                assert L.hsp_wgrad_plan(M, N, K, 2, 1, (M + 7) & ~7, N, 0, out) == -2        # hsp_wgrad_bf16 itself declines ragged M
                assert L.hsp_wgrad_plan(M, N, K, 4, 0, (M + 3) & ~3, N, 0, out) == -2        # base pointers off 16 bytes


def test_pair_workspace_covers_the_shrunk_plan():
    L = _L()
    out = (ctypes.c_int * 7)()
    shrunk = one = 0
    shapes = [(64, 64), (128, 128), (128, 256), (256, 128), (128, 384), (256, 256), (64, 512), (512, 512), (320, 832)]
    for M0, N0 in shapes:
        for M1, N1 in shapes:
            for K in (1, 255, 256, 300, 2056, 4112, 8224, 16448, 20000):
                assert L.hsp_wgrad_pair_plan(M0, N0, K, M1, N1, K, out) == 0
                if not out[0]:
                    continue
                one += 1
                alone = (ctypes.c_int * 4)()
                for M, N, sk, ks, b in ((M0, N0, out[1], out[2], out[5]), (M1, N1, out[3], out[4], out[6])):
                    assert sk % 4 == 0 and sk >= 8 and ks % 16 == 0 and sk * ks >= K and b == (M // 64) * (N // 64) * (sk // 4)
                    assert (sk // 4) * (M * N + N) * 4 <= L.hsp_wgrad_workspace_bytes(M, N, K), (M0, N0, M1, N1, K, list(out))
                    assert L.hsp_wgrad_plan(M, N, K, 4, 0, M + 2, N + 2, 0, alone) == 0 and alone[0] == gc.KB4 and sk <= alone[1]
                    shrunk += sk < alone[1]
    assert one > 50 and shrunk > 10
    assert L.hsp_wgrad_pair_plan(128, 100, 256, 128, 128, 256, out) == -2


def test_gemm_rows_workspace_covers_its_plan():
    L = _L()
    out = (ctypes.c_int * 4)()
    split = 0
    for es in (4, 2):
        for M in (1, 63, 64, 65, 129, 512, 1028, 4112, 16448):
            for N in (32, 63, 64, 65, 128, 129, 1024, 1286):
                for K1, K2 in ((1, 0), (33, 0), (256, 0), (257, 0), (4608, 0), (128, 4480), (4480, 128), (1286, 1024), (1024, 1286)):
                    ws = L.hsp_gemm_rows_workspace_bytes(M, N, K1, K2, es)
                    assert L.hsp_gemm_rows_plan(M, N, K1, K2, es, 16, out) == 0
                    tile, mode, ns, TT = out
                    bke = 128 // es
                    assert tile in (64, 128) and mode == 1 and 1 <= ns <= 16 and TT == -(-K1 // bke) + (-(-K2 // bke) if K2 else 0)
                    assert (ns * M * N * 4 if ns > 1 else 0) == ws, (es, M, N, K1, K2, list(out), ws)
                    if ns > 1:
                        assert TT // ns >= 4 and (ns - 1) * -(-TT // ns) < TT                 # >= 4 k-blocks a split, none empty
                    split += ns > 1
                    # the dispatch issues a ("nn", "nt") dual-source call with its sources swapped: the same plan, the same room
                    if K2:
                        swapped = (ctypes.c_int * 4)()
                        assert L.hsp_gemm_rows_plan(M, N, K2, K1, es, 16, swapped) == 0 and list(swapped) == list(out)
                        assert L.hsp_gemm_rows_workspace_bytes(M, N, K2, K1, es) == ws
    assert split > 20
    assert L.hsp_gemm_rows_plan(64, 64, 256, 0, 4, 8, out) == 0 and out[1] == 2
    assert L.hsp_gemm_rows_plan(64, 64, 256, 0, 4, 4, out) == 0 and out[1] == 0
    assert L.hsp_gemm_rows_plan(64, 64, 256, 0, 2, 8, out) == -2


def test_gemm_x3_workspace_covers_its_plan():
    L = _L()
    out = (ctypes.c_int * 4)()
    split = panel = 0
    for M in (1, 63, 64, 65, 129, 1121, 1152, 2305, 4112, 16448):
        for N in (64, 65, 128, 1286, 2048, 4096):
            for K1, K2 in ((1, 0), (128, 0), (511, 0), (512, 0), (1024, 0), (4608, 0), (128, 4480), (4480, 128)):
                ws = L.hsp_gemm_x3_workspace_bytes(M, N, K1, K2)
                for epi in (0, 1, 6):
                    for ldc in (N, N + 1):
                        rc = L.hsp_gemm_x3_plan(M, N, K1, K2, epi, ldc, out)
                        if not L.hsp_gemm_x3_supported(M, N, K1, K2):
                            assert rc == -2 and ws == 0
                            continue
                        assert rc == 0
                        pan, wm, ns, path = out
                        if pan:
                            panel += 1
                            assert K1 == 128 and K2 == 0 and N % 128 == 0 and epi <= 1 and ns == 1 and path == 0
                            continue
                        assert wm in (1, 2) and 1 <= ns <= 16 and (ns == 1 or epi == 0)
                        assert ns * M * N * 4 <= ws or ns == 1, (M, N, K1, K2, epi, list(out), ws)
                        assert path == (0 if ns == 1 else 4 if N % 4 == 0 and ldc % 4 == 0 else 1)
                        split += ns > 1
    assert split > 20 and panel > 4
