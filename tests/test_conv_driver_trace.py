"""The Conv2D per-channel driver's order of work, pinned on the CPU: which library calls layer.quantize_conv2d queues (channel planes,
patch matrices, the whole-shard entry points, the exact reruns of flagged pairs), which collectives it enters and what it returns -- per
cell of kernel size x kernel family x flagged pairs, in one process and over two and eight gloo ranks -- against
tests/golden/conv_trace.json, recorded from the commit named in tools/gen_conv_trace_golden.py (never from the code under test).  The GPU
tests check the results of these paths against the oracle; they cannot see a second channel_planes pass, an extra sync or a collective
that one rank leaves out.  The values are stamps (every weight holds its own coordinates), so the layout of what comes back is checked
here without the recorded file."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _traces(grid):
    """(grid name, cell name, rank name or None, trace) of every trace of a computed or recorded grid."""
    for gname, cells in grid.items():
        for cname, c in cells.items():
            if gname == "one_process":
                yield gname, cname, None, c
            else:
                for rname, t in c.items():
                    yield gname, cname, rname, t


def _collectives(trace):
    return [(e["ev"], e.get("op"), e["count"]) for e in trace["events"] if e["ev"] in ("all_gather", "all_reduce")]


def test_conv_driver_trace_equals_the_recorded_one(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_conv_trace_golden as gen
    before = [getattr(obj, name) for obj, name in gen.entry_points()]
    got = gen.compute(tmp_path)
    # the binding's entry points and the collectives are back
    assert [getattr(obj, name) for obj, name in gen.entry_points()] == before

    # what came back, against the stamps of W (run_cell's "layout"): independent of the recorded file
    specs = dict(one_process=dict(gen.one_process_cells()), two_ranks=dict(gen.sharded_cells()), eight_ranks=dict(gen.sharded_cells()))
    for gname, cname, rname, t in _traces(got):
        spec = specs[gname][cname]
        assert t["layout"] == dict(idx=True, Q=True, resid=True, contiguous=True), (gname, cname, rname, t["layout"])
        assert t["dtypes"] == dict(Q="torch.float32", idx="torch.int16" if spec["M"] > 64 else "torch.int8", resid="torch.float64"), (gname, cname, rname)
        one_by_one = spec["k"] == 1 and not spec["want_resid"]              # (_quantize_conv1x1 reports no reruns)
        assert t["keys"] == (["Q", "idx", "resid"] if one_by_one else ["Q", "idx", "reruns", "resid"]), (gname, cname, rname)
        if spec["want_resid"]:
            assert t["resid_nan"] == 0, (gname, cname, rname)

    with open(gen.GOLDEN) as f:
        want = json.load(f)
    assert list(got) == list(want) == ["one_process", "two_ranks", "eight_ranks"]
    for grid in want:
        assert list(got[grid]) == list(want[grid]), grid                   # the same cells
        for cell in want[grid]:
            if grid == "one_process":
                assert got[grid][cell] == want[grid][cell], f"{grid}: {cell}"
            else:
                assert list(got[grid][cell]) == list(want[grid][cell]), f"{grid}: {cell}"
                for rank in want[grid][cell]:
                    assert got[grid][cell][rank] == want[grid][cell][rank], f"{grid}: {cell}: {rank}"

    # the grid is the one the golden was recorded for, and it is not vacuous
    assert (len(want["one_process"]), len(want["two_ranks"]), len(want["eight_ranks"])) == (17, 9, 9)
    assert all(len(ranks) == world for g, world in gen.GRIDS.items() for ranks in want[g].values())
    seen = {e["ev"] for _, _, _, t in _traces(want) for e in t["events"]}
    assert seen == set(gen.EVENTS)                                         # every kind of event occurs somewhere
    assert {e["path"] for _, _, _, t in _traces(want) for e in t["events"] if e["ev"] == "quantize_neurons"} == {0, 1, 2}     # auto (the loop), on-chip and streaming reruns
    for grid in gen.GRIDS:
        for cell, ranks in want[grid].items():
            # all ranks enter the same collectives in the same order: kind, op and count
            first = _collectives(ranks["rank0"])
            assert first, (grid, cell)
            for rank, t in ranks.items():
                assert _collectives(t) == first, (grid, cell, rank)
            replicated = cell == "cin1/records"
            assert any(e["ev"] == "all_gather" for e in ranks["rank0"]["events"]) != replicated, (grid, cell)
            # fewer channels than ranks and no residual norms wanted: the ranks agree (MIN) on whether the records are taken
            spec = specs[grid][cell]
            asks = not spec["want_resid"] and spec["Cin"] < gen.GRIDS[grid]
            assert [op for _, op, _ in first if op] == (["MIN", "SUM", "MAX"] if replicated else ["MIN"] if asks else []), (grid, cell)
            # where the records are not taken -- unsupported on one rank, raising on one rank -- every rank walks its filters instead
            if cell in ("cin1/records_one_rank", "cin1/records_raise"):
                assert all(any(e["ev"] == "quantize_conv_channels" for e in t["events"]) == (i < 5) for i, t in enumerate(ranks.values())), (grid, cell)
    assert any(e.get("raises") for e in want["two_ranks"]["cin1/records_raise"]["rank1"]["events"])
    # one exact call per CHANNEL for its flagged pairs
    reruns = [e for e in want["one_process"]["k3/planes/three"]["events"] if e["ev"] == "quantize_neurons"]
    assert [(e["channels"], e["filters"]) for e in reruns] == [([0], [1, 4]), ([2], [2])]
    # the planes of a set of images are formed at most once per activation tensor (the record cells form them of their image shard and
    # then of all images), the NHWC forms need none
    for gname, cname, rname, t in _traces(want):
        spec = specs[gname][cname]
        per_images = {}
        for e in t["events"]:
            if e["ev"] == "channel_planes":
                per_images[e["nimg"]] = per_images.get(e["nimg"], 0) + 1
        assert all(n <= (1 if spec["same"] else 2) for n in per_images.values()), (gname, cname, rname)
        world = dict(gen.GRIDS, one_process=1)[gname]
        assert len(per_images) <= (2 if not spec["want_resid"] and spec["Cin"] < world else 1), (gname, cname, rname)
        if spec["support"] != "planes" and not spec["want_resid"] and spec["Cin"] >= world:
            assert not per_images, (gname, cname, rname)
