"""The row sink of infer.py's sampling job: which global rows a rank holds of the launches since the last flush, and how a
flush files the packed rows (series padded to Lmax | latent | encoding) into the three output arrays.  CPU only."""
import numpy as np
import pytest
import torch

import infer as drv
from t2ms_amd import dist as tdist
from t2ms_amd._lib import LAT, LAT_C, LAT_W

CHUNKS = [
    [(0, 3)],                                  # fewer rows than ranks at world 4, 5
    [(0, 5), (5, 12), (12, 13)],               # uneven launches, the last of one row
    [(7, 9)],                                  # one launch, empty for most ranks, not starting at row 0
    [(0, 6), (6, 12), (12, 18)],               # full launches (6 rows: divisible by 1, 2, 3; not by 4, 5)
    [(4, 5), (5, 6), (6, 7), (7, 8)],          # one-row launches: every row goes to rank 0
]


@pytest.mark.parametrize("world", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("chunks", CHUNKS)
def test_rank_rows_partition_the_held_launches(chunks, world):
    rows = [drv.rank_rows(chunks, r, world) for r in range(world)]
    # every row of the launches, each once
    assert sorted(np.concatenate(rows).tolist()) == list(range(chunks[0][0], chunks[-1][1]))
    for r in range(world):
        assert rows[r].dtype.kind == "i"
        # what the rank samples: its contiguous shard_rows slice of every launch, launch after launch
        shards = [tdist.shard_rows(s1 - s0, r, world) for s0, s1 in chunks]
        assert len(rows[r]) == sum(hi - lo for lo, hi in shards)
        at = 0
        for (s0, s1), (lo, hi) in zip(chunks, shards):
            assert rows[r][at:at + hi - lo].tolist() == list(range(s0 + lo, s0 + hi))
            at += hi - lo
    assert len(drv.rank_rows([], 0, world)) == 0


def _rows(row_ids, L, Lmax):
    """Packed rows with known columns: row g holds g + 0.25 in its L series columns (zero padding behind), g + 0.5 + the
    element number in its latent and -(g + the element number) in its encoding."""
    g = torch.tensor(row_ids, dtype=torch.float32)[:, None]
    series = torch.zeros(len(row_ids), Lmax)
    series[:, :L] = g + 0.25
    e = torch.arange(LAT, dtype=torch.float32)[None]
    return drv.RowSink.pack(series, (g + 0.5 + e).reshape(-1, LAT_C, LAT_W), (-(g + e)).reshape(-1, LAT_C, LAT_W))


@pytest.mark.parametrize("flush_rows", [None, 1, 4])
def test_flush_files_the_packed_rows_by_global_row(flush_rows, monkeypatch):
    if flush_rows is None:
        monkeypatch.delenv("T2S_INFER_FLUSH_ROWS", raising=False)
    else:
        monkeypatch.setenv("T2S_INFER_FLUSH_ROWS", str(flush_rows))
    n_rows, L, Lmax = 9, 24, 48
    sink = drv.RowSink(n_rows, Lmax, None, 0, 1, torch.device("cpu"))
    assert sink.out[0].shape == (n_rows, Lmax) and sink.out[1].shape == sink.out[2].shape == (n_rows, LAT_C, LAT_W)
    for o in sink.out:
        o.fill(np.nan)
    packed = _rows(list(range(n_rows)), L, Lmax)
    assert packed.shape == (n_rows, Lmax + 2 * LAT)
    flushed_after = []
    for s0, s1 in [(0, 3), (3, 4), (4, 9)]:
        sink.add(s0, s1, packed[s0:s1])
        flushed_after.append(not sink.held_chunks)
    assert flushed_after == {None: [False, False, False], 1: [True, True, True], 4: [False, True, True]}[flush_rows]
    sink.flush()
    assert not sink.held and not sink.held_chunks
    g = np.arange(n_rows, dtype=np.float32)
    e = np.arange(LAT, dtype=np.float32)
    assert np.array_equal(sink.out[0][:, :L], np.broadcast_to(g[:, None] + 0.25, (n_rows, L)))
    assert np.array_equal(sink.out[0][:, L:], np.zeros((n_rows, Lmax - L), np.float32))
    assert np.array_equal(sink.out[1], (g[:, None] + 0.5 + e[None]).reshape(n_rows, LAT_C, LAT_W))
    assert np.array_equal(sink.out[2], -(g[:, None] + e[None]).reshape(n_rows, LAT_C, LAT_W))
    sink.flush()                                     # nothing held: no-op


def test_a_rank_other_than_zero_keeps_no_arrays_and_a_launch_without_rows_is_still_recorded():
    sink = drv.RowSink(5, 24, None, 1, 2, torch.device("cpu"))
    assert sink.out is None
    sink.add(0, 1, None)                             # one row, two ranks: rank 1 has none of it
    assert sink.held == [] and sink.held_chunks == [(0, 1)]
    assert len(drv.rank_rows(sink.held_chunks, 1, 2)) == 0 and drv.rank_rows(sink.held_chunks, 0, 2).tolist() == [0]
