"""Neighbour records of the device map (srl_device.h, srl_map_kernels.hip: k_nbrec_update) against a brute-force model.

Per voxel (slab order) 32 words: word (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1) = slab << 5 | count of the voxel at key + (dx, dy, dz) with the
16-bit wrap of the probes' keys, 0xFFFFFFFF where the map has no such voxel, words 27 .. 31 zero.  The model is a dictionary built from
srl_map_download; the records must equal it after every kind of map edit, because a pass reads them instead of the table:
  a first insert; a second one that raises counts of old voxels and creates voxels beside old and beside other new ones; an insert that
  fills a voxel to 20; srl_map_upload; a prune followed by an insert (slabs renumbered, an erased key comes back); a growth of the storage.
The maps hold the keys -1, 0 and 1 on every axis and voxels at keys 32 767 and -32 768 of the x axis (neighbours through the wrap)."""
import numpy as np
import pytest

import sr_livo_amd as srl

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF


def _wrap16(v):
    return ((int(v) + 32768) % 65536) - 32768


def _model(keys, counts):
    index = {tuple(int(c) for c in k): v for v, k in enumerate(keys)}
    out = np.zeros((len(keys), 32), np.uint32)
    for v, (kx, ky, kz) in enumerate(keys.astype(np.int64)):
        for d in range(27):
            nk = (_wrap16(kx + d // 9 - 1), _wrap16(ky + (d // 3) % 3 - 1), _wrap16(kz + d % 3 - 1))
            n = index.get(nk)
            out[v, d] = NONE if n is None else (n << 5) | int(counts[n])
    return out


def _check(ctx, what):
    keys, counts, _ = ctx.map_download()
    got = ctx.neighbour_records_download()
    want = _model(keys, counts)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "first differing (voxel, word), got, expected", bad[:6].tolist(), [hex(int(got[v, w])) for v, w in bad[:6]],
                           [hex(int(want[v, w])) for v, w in bad[:6]])
    assert np.all(got[np.arange(len(keys)), 13] == (np.arange(len(keys)) << 5 | counts)), (what, "word 13 is the voxel itself")
    return keys, counts


def _cell(rng, key, n):
    """n points of the voxel with this key (truncation toward zero: key 0 spans (-1, 1)), well apart from one another"""
    key = np.asarray(key, np.float64)
    lo = np.where(key > 0, key, np.where(key < 0, key - 1.0, 0.0))
    grid = np.array([(i, j, k) for i in range(3) for j in range(3) for k in range(3)], np.float64)[rng.permutation(27)[:n]]
    return lo + 0.08 + 0.3 * grid + rng.uniform(0.0, 0.02, (n, 3))


def _first_batch(rng):
    cells = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x + y + z) % 2 == 0]          # a checkerboard round the origin
    cells += [(32767, 3, 3), (-32768, 3, 3), (-32767, 3, 3), (32767, -4, 0), (5, 32767, -32768), (5, -32768, -32768)]
    cells += [(10 + i, 10 + j, 2) for i in range(12) for j in range(12) if (i * 7 + j * 3) % 5 != 0]                  # a slab of ~115 voxels with holes
    return np.concatenate([_cell(rng, c, int(rng.integers(1, 9))) for c in cells])


def _second_batch(rng):
    old = [(0, 0, 0), (1, 1, 0), (32767, 3, 3), (12, 13, 2)]                                    # counts of old voxels rise
    beside_old = [(0, 0, 1), (-1, 0, 0), (-32768, 4, 3), (10, 10, 3), (9, 10, 2)]               # new voxels beside old ones
    beside_new = [(40, 40, 40), (41, 40, 40), (41, 41, 41), (40, 39, 40), (-32768, -4, 0), (-32768, -5, 0)]    # ... and beside each other
    return np.concatenate([_cell(rng, c, int(rng.integers(2, 7))) for c in old + beside_old + beside_new])


@pytest.fixture(scope="module")
def ctx():
    c = srl.Context(0)
    yield c
    c.close()


def test_records_equal_the_model_after_every_kind_of_edit(ctx):
    rng = np.random.default_rng(9101)
    first = _first_batch(rng)
    ctx.map_insert(first)
    keys, counts = _check(ctx, "first insert")
    have = {tuple(k) for k in keys.tolist()}
    for axis in range(3):
        assert {-1, 0, 1} <= set(keys[:, axis].tolist()), axis
    assert {(32767, 3, 3), (-32768, 3, 3), (-32767, 3, 3)} <= have
    v_hi, v_lo = (int(np.flatnonzero((keys == k).all(1))[0]) for k in ((32767, 3, 3), (-32768, 3, 3)))
    rec = ctx.neighbour_records_download()
    assert rec[v_hi, 2 * 9 + 4] >> 5 == v_lo and rec[v_lo, 0 * 9 + 4] >> 5 == v_hi, "32 767 and -32 768 are neighbours through the wrap"

    ctx.map_insert(_second_batch(rng))
    keys2, counts2 = _check(ctx, "second insert")
    assert len(keys2) > len(keys) and np.any(counts2[: len(keys)] > counts), "old counts rose, new voxels came"

    ctx.map_insert(_cell(rng, (0, 0, 0), 27))                                                  # more than a voxel takes
    keys3, counts3 = _check(ctx, "a voxel filled")
    v0 = int(np.flatnonzero((keys3 == (0, 0, 0)).all(1))[0])
    assert counts3[v0] == 20

    # a prune renumbers the slabs; the erased slab of voxels round (10..21, 10..21, 2) comes back in part
    removed, _ = ctx.map_remove_far(np.array([0.0, 0.0, 0.0]), 12.0)
    keys4, _ = _check(ctx, "prune")
    assert removed > 100 and len(keys4) == len(keys3) - removed and (0, 0, 0) in {tuple(k) for k in keys4.tolist()}
    ctx.map_insert(np.concatenate([_cell(rng, (10 + i, 10, 2), 3) for i in range(4)] + [_cell(rng, (0, 1, 0), 2)]))
    keys5, _ = _check(ctx, "insert after the prune")
    assert (11, 10, 2) in {tuple(k) for k in keys5.tolist()} and (11, 10, 2) not in {tuple(k) for k in keys4.tolist()}


def test_records_after_an_upload_and_across_a_growth_of_the_storage(ctx):
    rng = np.random.default_rng(9102)
    src = srl.Context(0)
    try:
        src.map_insert(np.concatenate([_first_batch(rng), _second_batch(rng)]))
        keys, counts, xyz = src.map_download()
    finally:
        src.close()
    ctx.map_upload(keys, counts, xyz)
    k1, c1 = _check(ctx, "upload")
    assert np.array_equal(k1, keys) and np.array_equal(c1, counts)
    # An upload reserves voxels * 3 / 2 + 4 096 slabs; an insertion makes room for one new voxel per point of its batch beforehand.  6 000
    # points in 40 voxels therefore grow slab storage, records and table (rebuilt from the slabs) while the voxels keep their indices.
    assert len(keys) + len(keys) // 2 + 4096 < len(keys) + 6000
    cells = [(0, 0, 0), (1, 1, 0)] + [(60 + i, -7, 1) for i in range(38)]
    batch = np.concatenate([_cell(rng, c, 27) for c in cells] * 6)[:6000]
    ctx.map_insert(batch)
    k2, c2 = _check(ctx, "insert that grows the storage")
    assert np.array_equal(k2[: len(keys)], keys) and len(k2) == len(keys) + 38
    ctx.map_insert(_second_batch(rng))
    _check(ctx, "insert after the growth")
