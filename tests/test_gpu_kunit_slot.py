"""Device primitives on their own (tests/kunit/kunit.hip), part 6: the per-slot tile loop of csrc/slot_tiles.h
(geometry, staging predicates, chunk odometer, restart of the product, epilogue) with the plainest hooks: two
row-major panels, a fold that squares the product, optionally a second phase that stages only the rows of one shard.

Every input is an integer of magnitude <= 3 held in a double and 1 / effsamp is a power of two, so every product,
square and sum is exact and the device result must EQUAL NumPy's
    out[a][b] = inv_eff  sum_s ( A0_s B0_s' + [a, b in shard SIG] A1_s B1_s' )_ab ^ 2        (a >= b)
with nothing on the strict upper part of the diagonal tiles or on the rows past p.  p = 130 gives two tile rows,
the second 2 rows high; K = 1 ends a slot inside a k-step, K = 5 starts slot 1 at an offset that is only 8-byte
aligned, K = 16 is one whole chunk, K = 17 a whole chunk and a one-column one.  Columns outside the slots in use
hold NaN, which a load that strays beyond k < K would carry into the sums.  One launch per (K, nph) runs the
slot counts 0, 1 and 3."""
import numpy as np
import pytest

import kunit_ref as R

pytestmark = pytest.mark.gpu

P_ROWS, SHARD = 130, 65          # two shards; the second one spans both tile rows
SIG = 1                          # the shard of phase 1
KH = 64                          # columns of a phase's half of a panel
NS = (0, 1, 3)
INV_EFF = 0.25
TILE = 128


def _unpack(buf, p):
    """A rank's tile-packed lower triangle (dcfm_internal.h: sig_tile_off) as a dense nt*128 square; the strict
    upper tiles, which the layout does not hold, stay zero."""
    nt = (p + TILE - 1) // TILE
    ra, cb = np.meshgrid(np.arange(TILE), np.arange(TILE), indexing="ij")
    rr = ra & 15
    u, v, g, w, lane = (ra >> 4) & 3, (cb >> 4) & 3, rr >> 2, 2 * (ra >> 6) + (cb >> 6), (rr & 3) * 16 + (cb & 15)
    off = ((((w * 4 + u) * 4 + v) * 2 + (g >> 1)) * 64 + lane) * 2 + (g & 1)
    assert np.array_equal(np.sort(off.ravel()), np.arange(TILE * TILE))
    full = np.zeros((nt * TILE, nt * TILE))
    for ti in range(nt):
        for tj in range(ti + 1):
            tile = buf[(ti * (ti + 1) // 2 + tj) * TILE * TILE:][:TILE * TILE]
            full[ti * TILE:(ti + 1) * TILE, tj * TILE:(tj + 1) * TILE] = tile[off]
    return full


@pytest.fixture(scope="module")
def panels():
    rng = np.random.default_rng(20)
    A = rng.integers(-3, 4, size=(P_ROWS, 2 * KH)).astype(np.float64)
    B = rng.integers(-3, 4, size=(P_ROWS, 2 * KH)).astype(np.float64)
    return A, B


def _expected(A, B, K, nslots, nph):
    m = (np.arange(P_ROWS) // SHARD == SIG).astype(np.float64)[:, None]
    acc = np.zeros((P_ROWS, P_ROWS))
    for s in range(nslots):
        t = A[:, s * K:(s + 1) * K] @ B[:, s * K:(s + 1) * K].T
        if nph == 2:
            t = t + (m * A[:, KH + s * K:KH + (s + 1) * K]) @ (m * B[:, KH + s * K:KH + (s + 1) * K]).T
        acc += t * t
    return INV_EFF * np.tril(acc)


@pytest.mark.parametrize("nph", [1, 2])
@pytest.mark.parametrize("K", [1, 5, 16, 17])
def test_slot_loop_equals_numpy(panels, K, nph):
    A, B = (x.copy() for x in panels)
    used = max(NS) * K
    for X in (A, B):                                 # nothing but the slots in use may be read
        X[:, used:KH] = np.nan
        X[:, KH + (used if nph == 2 else 0):] = np.nan
    nt = (P_ROWS + TILE - 1) // TILE
    ntile = nt * (nt + 1) // 2
    out = np.zeros(len(NS) * ntile * TILE * TILE)
    ns = np.array(NS, dtype=np.int32)
    assert R.lib().kunit_slot(R.ptr(A), R.ptr(B), P_ROWS, SHARD, K, KH, R.ptr(ns), len(NS), nph, SIG,
                              R.c_double(INV_EFF), R.ptr(out)) == 0
    for c, nslots in enumerate(NS):
        full = _unpack(out[c * ntile * TILE * TILE:(c + 1) * ntile * TILE * TILE], P_ROWS)
        want = np.zeros_like(full)
        want[:P_ROWS, :P_ROWS] = _expected(panels[0], panels[1], K, nslots, nph)
        bad = np.argwhere(full != want)
        print(f"K={K} nph={nph} nslots={nslots}: {len(bad)} of {full.size} entries differ, max |out| {np.abs(full).max():g}")
        assert len(bad) == 0, f"nslots={nslots}: first differing (row, col) {bad[:5].tolist()}"
