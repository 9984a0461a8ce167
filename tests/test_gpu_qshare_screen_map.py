"""The MFMA operand map of the screened shared-row scan (screen_tile,
wvg_qshare.hip), checked with exact integer data through the real kernel.

Row r has a single non-zero element, e = r mod 128, an integer v(r) <= 251;
query j is 32 at the eight elements e with e mod 16 == j and zero elsewhere.
Every bf16 operand, product and sum is exact, so the screen's dot is exactly
32 v(r) where the row's element meets the query and 0 elsewhere: the match moves
a distance by 64 v, forty times the bound's slack (2 c |q| |x| ~ 1.4 v).  In the
first corpus every tile keeps ONE live row (all others deleted), in a lane that
changes from tile to tile, so a (query, tile) pair is folded or skipped on that
lane's bound alone: a wrong lane, query or k map skips tiles that hold results,
and the pipelined call no longer equals the single searches.
"""
import numpy as np
import pytest

from weaviate_amd._lib import METRIC_L2

from test_gpu_qshare_seed import Corp

D, TILES, NQ = 128, 64, 16


def _rows_and_queries():
    r = np.arange(TILES * 64)
    rows = np.zeros((len(r), D), np.float32)
    rows[r, r % D] = (r % 251) + 1
    qs = np.zeros((NQ, D), np.float32)
    for j in range(NQ):
        qs[j, j::16] = 32.0
    return rows, qs


@pytest.mark.gpu
@pytest.mark.parametrize("one_live_row_per_tile", [True, False])
def test_exact_integer_dots_fold_the_right_tiles(ctx, orc, one_live_row_per_tile):
    rows, qs = _rows_and_queries()
    dead = []
    if one_live_row_per_tile:
        live = np.arange(TILES) * 64 + (np.arange(TILES) * 7 + 3) % 64
        dead = np.setdiff1d(np.arange(len(rows)), live)
    cp = Corp(ctx, orc, METRIC_L2, rows, qs, dead)
    try:
        for k in (1, 4, 10):
            for nq in (NQ, 5):
                cp.check(nq, k)
    finally:
        cp.destroy()
