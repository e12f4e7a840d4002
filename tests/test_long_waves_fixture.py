"""CPU checks of the long-wave fixture (tests/long_waves_data.py): its tile counts meet the launch-shape conditions
tests/test_gpu_long_waves.py asserts for grids of 8 workgroups, its neighbouring segments differ in width the way the
filter's counted waits need, the planner has segments to drop, and the sums of d are exact in any order."""
import numpy as np

from oracle import executor
from pinot_amd.query.sql import parse
from tests import long_waves_data as lw

FILTER_WAVES = 8 * 4            # 8 workgroups of 4 waves
AGG_WAVES = (8 * 8, 8 * 16)     # 8 workgroups of 8 / 16 waves


def _meets(tiles):
    return tiles >= 10 * FILTER_WAVES and tiles >= 6 * AGG_WAVES[0] and tiles >= 3 * AGG_WAVES[1]


def test_long_waves_tile_counts_meet_the_shape_conditions():
    raws = lw.raw_segments()
    assert [r.num_docs for r in raws] == [n for n, _, _ in lw.LAYOUT]
    assert {1, 63, 64, 65, 2047, 2048, 2049, 4097, 6144} <= {n for n, _, _ in lw.LAYOUT}
    assert _meets(lw.total_tiles())
    # a predicate on tag above 1 drops the `low` segments (and tag = 7 at most the tiny ones that lack a 7)
    kept = lw.total_tiles(lambda i, n, low: not low)
    assert _meets(kept) and sum(1 for _, _, low in lw.LAYOUT if not low) >= 24
    tiny = sum(lw.tiles(n) for n, _, low in lw.LAYOUT if not low and n < 200)
    assert _meets(kept - tiny)
    # the range on the sorted column: tiles of each kept segment's hull of candidate docs
    work, nseg = 0, 0
    for r in raws:
        ts = np.asarray(executor.OracleSegment(r).values("ts"))
        docs = np.nonzero((ts >= lw.TS_LO) & (ts <= lw.TS_HI))[0]
        if len(docs):
            work += docs[-1] // lw.TILE - docs[0] // lw.TILE + 1
            nseg += 1
    assert _meets(work) and 24 <= nseg < len(raws) and work < lw.total_tiles() - 20  # (tiles cut at both ends)


def test_long_waves_segments_differ_the_way_the_walks_need():
    raws = lw.raw_segments()
    bits = [r.columns["w"].metadata.bits_per_element for r in raws]
    for (n, want, _), b in zip(lw.LAYOUT, bits):
        assert want == 0 or b == want, (n, want, b)
    # 3-, 11- and 17-bit segments within three places of each other, tiny segments between bulk ones
    spots = [i for i, b in enumerate(bits) if b == 17]
    assert len(spots) >= 4
    for i in spots:
        near = set(bits[max(0, i - 3):i + 4])
        assert {3, 11} <= near, (i, near)
    sizes = [n for n, _, _ in lw.LAYOUT]
    between = sum(1 for i in range(1, len(sizes) - 1) if sizes[i] < 2 * lw.TILE and sizes[i - 1] > 10_000 and sizes[i + 1] > 10_000)
    assert between >= 4
    assert all(r.columns["ts"].metadata.is_sorted for r in raws)
    assert all(r.columns["nr"].metadata.bits_per_element <= 12 for r in raws)
    assert max(r.columns["wd"].metadata.bits_per_element for r in raws) > 12
    assert all(not r.columns[c].metadata.has_dictionary for r in raws for c in ("gr", "rl", "rs"))
    assert any(r.columns["nl"].null_vector is None for r in raws) and any(r.columns["nl"].null_vector for r in raws)
    # the dropped segments: no doc with a tag above 1
    qc = parse("SELECT COUNT(*) FROM t WHERE tag >= 2")
    for r, (_, _, low) in zip(raws, lw.LAYOUT):
        assert bool(np.count_nonzero(executor.filter_mask(qc, r))) != low or r.num_docs < 8


def test_long_waves_double_sums_are_exact_in_any_order():
    """d holds multiples of 0.25 below 2^30: the sum over all docs stays below 2^53 quarter units, so every partial sum
    is a double without rounding and the oracle's sum equals the integer sum whatever the order."""
    raws = lw.raw_segments()
    total = 0
    for r in raws:
        d = np.asarray(executor.OracleSegment(r).values("d"))
        q = (d * 4).astype(np.int64)
        assert np.array_equal(q / 4.0, d) and d.max() < 2.0 ** 30 and d.min() >= 0
        total += int(q.sum())
    assert total < 2 ** 53
    oblk, _ = executor.execute(parse("SELECT SUM(d) FROM t WHERE nr < 200"), raws)
    assert oblk.results[0] == total / 4.0
