"""The Dense layer drivers' order of work, pinned on the CPU: what each entry point launches, which host waits it pays (call_status,
DeviceAlphabet.values()), what it queues before and after them, what it logs and returns -- per cell of entry point x kernel family x
scripted deferred statuses x check, in one process and over two gloo ranks -- against tests/golden/driver_trace.json, recorded from
the commit named in tools/gen_driver_trace_golden.py (never from the code under test).  The GPU failure matrix
(test_failsafe_matrix_gpu.py) checks the results of these paths; it cannot see an extra host wait on a healthy layer or a status read
that moved behind the all-gather."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dense_driver_trace_equals_the_recorded_one(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_driver_trace_golden as gen
    before = [getattr(obj, name) for obj, name in gen.entry_points()]
    got = gen.compute(tmp_path)
    with open(gen.GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want) == ["one_process", "two_ranks"]
    for grid in want:
        assert list(got[grid]) == list(want[grid]), grid                   # the same cells
        for cell in want[grid]:
            assert got[grid][cell] == want[grid][cell], f"{grid}: {cell}"
    # the grid is the one the golden was recorded for, and it is not vacuous
    one = want["one_process"]
    assert len(one) == 132 and len(want["two_ranks"]) == 18
    assert sum(c["raised"] for c in one.values()) == 9 and sum(bool(c["log"]) for c in one.values()) == 37
    for cell, ranks in want["two_ranks"].items():
        # the healthy rank never notices what the other one met: the same trace in every cell of its entry and family, as many collectives
        healthy = want["two_ranks"][cell.rsplit("/", 1)[0] + "/none"]["rank0"]
        assert ranks["rank0"] == healthy, cell
        n_gathers = [sum(e["ev"] == "all_gather" for e in ranks[r]["events"]) for r in ("rank0", "rank1")]
        assert n_gathers[0] == n_gathers[1] == 2, cell
        # ... because the other one reads its status and repairs its shard BEFORE anything of it travels
        ev = [e["ev"] for e in ranks["rank1"]["events"]]
        if "call_status" in ev:
            assert max(i for i, e in enumerate(ev) if e == "call_status") < ev.index("pack_indices") < ev.index("all_gather"), cell
    # the binding's entry points are back
    assert [getattr(obj, name) for obj, name in gen.entry_points()] == before
