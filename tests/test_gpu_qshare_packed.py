"""Packed exact rounds of the shadow-fed shared-row scan (scan_f32_qshare_shadow_kernel and its filtered
twin, wvg_qshare.hip, "Packed rounds"): a tile appends its admitted (query, row) pairs to the wave's queue
in LDS, and the exact chain runs in rounds of 64 pairs -- while 64 are pending, and until the queue is
empty after the last tile of a pass.  Results must not change: every call in a default context is compared
bit for bit (ids, distance bits, counts) with one host wvg_search per query in a batch_screen = 0 context,
which never reads the shadow.

The corpora are L2, d = 128, id_base 0, and sized from the device: the scan runs two workgroups of four
waves per CU, and the large corpus has 3 tiles per wave + 37 (so ranges of 3 and 4 tiles) with 17 live
rows in the last tile; a wave's range is [tiles * w / waves, tiles * (w + 1) / waves).  The prologue's sample
is the first 64 tiles.  The tests plant rows into the one large corpus (in both contexts) and take the
reference after planting; planted rows of an earlier test stay and are part of the later references.
A call with one query does not take the shared-row route at all (the host's routing, unchanged); it is
run and compared all the same.
"""
import numpy as np
import pytest

from weaviate_amd._lib import KIND_F32, METRIC_L2
from weaviate_amd.device import Context, Corpus

from test_gpu_parity import bits
from test_gpu_qshare_filter import filtered_search
from test_gpu_qshare_shadow import _captured, _same, _stream

D = 128
SAMPLE_ROWS = 64 * 64  # the prologue's sample: the first 64 tiles
NQ_MAX = 32


class Big:
    """One corpus in the default context (`c`) and the same rows in the exact context (`x`)."""

    def __init__(self, ctx, exact_ctx, n, seed):
        self.n, self.tiles = n, (n + 63) // 64
        rng = np.random.default_rng(seed)
        self.rows = rng.uniform(-1.0, 1.0, (n, D)).astype(np.float32)
        self.qs = rng.uniform(-1.0, 1.0, (NQ_MAX, D)).astype(np.float32)
        self.c = Corpus(ctx, KIND_F32, METRIC_L2, D, n)
        self.x = Corpus(exact_ctx, KIND_F32, METRIC_L2, D, n)
        ids = np.arange(n, dtype=np.uint64)
        for cp in (self.c, self.x):
            cp.upsert(ids, self.rows)

    def plant(self, idx, vecs):
        idx = np.asarray(idx, np.uint64)
        vecs = np.ascontiguousarray(vecs, np.float32)
        assert len(np.unique(idx)) == len(idx) and int(idx.max()) < self.n
        for cp in (self.c, self.x):
            cp.upsert(idx, vecs)

    def want(self, qs, k, words=None):
        """One host wvg_search per query in the exact context, stacked like a stream call's outputs."""
        outs = [self.x.search(qs[[qi]], k, allow=None if words is None else words[qi]) for qi in range(len(qs))]
        return (np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs]),
                np.concatenate([o[2] for o in outs]))

    def shadow(self, nq, k):
        return self.c.search_device_shadow(nq, k)["reads_shadow"]

    def destroy(self):
        self.c.destroy()
        self.x.destroy()


def _waves():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count * 2 * 4


def _range(tiles, waves, w):
    return tiles * w // waves, tiles * (w + 1) // waves


def _near(q, count, seed, scale=1e-3):
    """`count` distinct rows close to q."""
    noise = np.random.default_rng(seed).uniform(-scale, scale, (count, D)).astype(np.float32)
    return q[None, :] + noise


@pytest.fixture(scope="module")
def exact_ctx():
    c = Context(0, batch_screen=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big(ctx, exact_ctx):
    waves = _waves()
    tiles = 3 * waves + 37
    b = Big(ctx, exact_ctx, tiles * 64 - 47, 7101)
    b.waves = waves
    assert min(_range(tiles, waves, w)[1] - _range(tiles, waves, w)[0] for w in range(waves)) >= 3
    yield b
    b.destroy()


def _check_stream(b, qs, k, reps=2):
    want = b.want(qs, k)
    for got in _stream(b.c, qs, k, reps=reps):
        _same(got, want, (len(qs), k))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 5, 16])
def test_pairs_from_several_tiles_in_one_round(big, nq):
    """A near neighbour of query 0 in every tile of four waves' ranges (the first, two inner ones, the last
    with the ragged tile): each of those waves holds a pair from every one of its tiles in one round."""
    plant = []
    for w in (0, 1, big.waves // 2, big.waves - 1):
        t0, t1 = _range(big.tiles, big.waves, w)
        plant += [t * 64 + (t * 7) % 17 for t in range(t0, t1)]  # (row < 17: live in the ragged last tile too)
    big.plant(plant, _near(big.qs[0], len(plant), 7102))
    for k in (1, 10, 64):
        assert big.shadow(nq, k) == (1 if nq > 1 else 0)
        want = _check_stream(big, big.qs[:nq], k)
        assert np.isin(want[0][0][:min(k, len(plant))], np.asarray(plant, np.uint64)).all()


def _words(masks):
    nq, n = masks.shape
    pad = np.zeros((nq, (n + 63) // 64 * 64), np.uint8)
    pad[:, :n] = masks
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("n_open", [0, 1, 2, 16])
def test_drain_thresholds_with_open_queries(big, n_open):
    """The filtered twin.  A list with no row in the prologue's sample leaves its query's tau open, and an
    open query admits every allowed row: 64, 128 and 1,024 entries per tile for 1, 2 and 16 such queries (the
    last fills the queue to its capacity: up to 63 pending + 16 x 64).  n_open = 0: all-ones lists."""
    nq, k = 16, 10
    masks = np.ones((nq, big.n), bool)
    masks[:n_open, :SAMPLE_ROWS] = False
    words = _words(masks)
    assert big.shadow(nq, k) == 1
    want = big.want(big.qs[:nq], k, words)
    for got in filtered_search(big.c, big.qs[:nq], k, [words, words], 0, big.tiles):
        _same(got, want, n_open)
    if n_open:  # the list took effect
        assert (want[0][:n_open] >= SAMPLE_ROWS).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [17, 32])
def test_second_pass_starts_with_an_empty_queue(big, nq):
    """Two passes of 16 queries: query 3's near rows fill one wave's tiles, query 18's another's."""
    wa, wb = 100, big.waves - 5
    pa = [t * 64 + 9 for t in range(*_range(big.tiles, big.waves, wa))]
    pb = [t * 64 + 50 for t in range(*_range(big.tiles, big.waves, wb))]
    big.plant(pa + pb, np.concatenate([_near(big.qs[3], len(pa), 7103), _near(big.qs[18], len(pb), 7104)]))
    k = 10
    assert big.shadow(nq, k) == 1
    want = _check_stream(big, big.qs[:nq], k)
    assert np.isin(want[0][3][:len(pa)], np.asarray(pa, np.uint64)).all()
    if nq == 32:
        assert np.isin(want[0][18][:len(pb)], np.asarray(pb, np.uint64)).all()


@pytest.mark.gpu
def test_special_values(big):
    """NaN, +inf and 1e30 rows in the first, a middle and the last tile of a wave's range (they are admitted
    for every query), and a NaN query (it admits every row)."""
    t0, t1 = _range(big.tiles, big.waves, big.waves // 3)
    idx, vecs = [], []
    for t in (t0, t0 + 1, t1 - 1):
        for off, val in ((3, np.nan), (20, np.inf), (40, 1e30)):
            v = big.rows[t * 64 + off].copy()
            v[17] = val
            if val == 1e30:
                v[:] = 1e30
            idx.append(t * 64 + off)
            vecs.append(v)
    big.plant(idx, np.stack(vecs))
    qs = big.qs[:16].copy()
    qs[4, 9] = np.nan
    for k in (10, 64):
        assert big.shadow(16, k) == 1
        _check_stream(big, qs, k)


@pytest.mark.gpu
def test_ties_are_broken_by_id(big):
    """One row in every tile of eight consecutive waves (>= 24 tiles): equal distances, the smaller ids win."""
    tiles = [t for w in range(40, 48) for t in range(*_range(big.tiles, big.waves, w))]
    assert len(tiles) >= 20
    idx = [t * 64 + 31 for t in tiles]
    v = _near(big.qs[7], 1, 7105, 5e-4)[0]
    big.plant(idx, np.repeat(v[None, :], len(idx), axis=0))
    k = 10
    assert big.shadow(16, k) == 1
    want = _check_stream(big, big.qs[:16], k)
    assert np.array_equal(want[0][7], np.asarray(sorted(idx)[:k], np.uint64))
    assert len(set(bits(want[1][7]).tolist())) == 1


@pytest.mark.gpu
def test_both_directions_and_graph_replays(big):
    """Two consecutive calls (the second walks the ranges in reverse) and a captured call replayed twice
    all equal the first call -- and the exact context's searches."""
    nq, k = 17, 10
    want = big.want(big.qs[:nq], k)
    first, second = _stream(big.c, big.qs[:nq], k, reps=2)
    _same(first, want, "first")
    _same(second, first, "reversed")
    for got in _captured(big.c, big.qs[:nq], k, 1):
        _same(got, first, "replay")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["rows17", "tile_per_wave"])
def test_short_ranges(ctx, exact_ctx, shape):
    """17 live rows (one wave, one ragged tile) and one tile per wave: only the final drain runs."""
    waves = _waves()
    b = Big(ctx, exact_ctx, 17 if shape == "rows17" else waves * 64 - 47, 7106)
    try:
        if shape == "tile_per_wave":
            plant = [t * 64 + 5 for t in (0, 1, waves // 2, waves - 1)]
            b.plant(plant, _near(b.qs[2], len(plant), 7107))
        for nq in (5, 16, 17):
            for k in (1, 10, 64):
                assert b.shadow(nq, k) == 1
                _check_stream(b, b.qs[:nq], k)
    finally:
        b.destroy()
