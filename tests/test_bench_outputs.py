"""bench.py --dump-outputs (CPU only): the files written for the last timed step's blocks -- float64 arrays, one
set per query, the same bytes for the same blocks, group-by values in sorted-key order, within the size budget."""
import os

import numpy as np

import bench
from pinot_amd.engine.results import AggregationResultsBlock, ExecutionStatistics, GroupByResultsBlock


def _blocks():
    agg = AggregationResultsBlock([None, None], [44682136700000, (3.5, 7)], ExecutionStatistics(num_docs_scanned=11920215))
    gb = GroupByResultsBlock([None, None], [None], {("b",): [2, np.arange(4, dtype=np.uint8)],
                                                    ("a",): [1, np.zeros(4, dtype=np.uint8)]},
                             ExecutionStatistics(num_docs_scanned=9))
    return {"Q1.1": agg, "G": gb}


def test_dump_outputs_files(tmp_path):
    d = str(tmp_path / "out")
    bench.dump_outputs(d, _blocks())
    assert sorted(os.listdir(d)) == ["G.num_docs_scanned.npy", "G.num_groups.npy", "G.results.npy",
                                     "Q1.1.num_docs_scanned.npy", "Q1.1.results.npy"]
    got = {f: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert all(a.dtype == np.float64 and a.ndim == 1 for a in got.values())
    assert got["Q1.1.results.npy"].tolist() == [44682136700000.0, 3.5, 7.0]
    assert got["Q1.1.num_docs_scanned.npy"].tolist() == [11920215.0]
    assert got["G.num_groups.npy"].tolist() == [2.0]
    assert got["G.results.npy"].tolist() == [1, 0, 0, 0, 0, 2, 0, 1, 2, 3]  # group ("a",) before ("b",)


def test_dump_outputs_repeatable_and_bounded(tmp_path, monkeypatch):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, _blocks())
    bench.dump_outputs(b, _blocks())
    for f in os.listdir(a):
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read()
    assert bench.DUMP_LIMIT_BYTES <= 64 << 20
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 8)  # room for 8 values in all
    c = str(tmp_path / "c")
    bench.dump_outputs(c, _blocks())
    assert sum(np.load(os.path.join(c, f)).size for f in os.listdir(c)) == 8
