"""CPU: the one-GPU median's last-workgroup hand-off, checked in the generated gfx950 code.

gpfq_median2_kernel (csrc/gpfq_misc.hip) merges every workgroup's LDS histogram into the global one with non-returning agent-scope
atomics, then thread 0 takes a ticket (a returning atomic on the control block); the workgroup that draws the last ticket picks the order
statistics from the merged histogram and forms the layer alphabet.  That is only right if every wavefront's merges have been acknowledged
before its workgroup takes the ticket.  No run shows the race reliably, so the property is checked where it lives: in the assembly.  For
each instantiation, after the last merge atomic before the ticket there must be an `s_waitcnt vmcnt(0)` (non-returning atomics count in
vmcnt on gfx9) that an `s_barrier` follows before the ticket: each wavefront waits for its own merges, then the workgroup moves on."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantized_neural_networks_amd", "csrc")


def _hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None


@pytest.fixture(scope="module")
def median_kernels(tmp_path_factory):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("hipcc is not installed")
    from quantized_neural_networks_amd import build
    out = str(tmp_path_factory.mktemp("isa") / "gpfq_misc.s")
    flags = [f for f in build.FLAGS + build.EXTRA_FLAGS.get("gpfq_misc.hip", []) if f != "-fPIC"]
    subprocess.check_call([hipcc] + flags + ["--cuda-device-only", "-S", "-o", out, "gpfq_misc.hip"], cwd=CSRC)
    lines = open(out).read().split("\n")
    kernels = {}
    for i, line in enumerate(lines):
        m = re.match(r"^(_Z\S*gpfq_median2_kernel\S*):", line)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            kernels[m.group(1)] = [l.split(";")[0].strip() for l in lines[i + 1:end]]
    return kernels


def test_both_passes_are_instantiated(median_kernels):
    assert len(median_kernels) == 2, list(median_kernels)


def test_every_wavefront_waits_for_its_merges_before_the_ticket(median_kernels):
    for name, body in median_kernels.items():
        tickets = [i for i, l in enumerate(body) if re.match(r"global_atomic_add\b", l) and re.search(r"\bsc0\b", l)]
        assert len(tickets) == 1, (name, [body[i] for i in tickets])           # the ticket is the kernel's one returning atomic add
        t = tickets[0]
        merges = [i for i in range(t) if re.match(r"global_atomic\w*\b", body[i]) and not re.search(r"\bsc0\b", body[i])]
        assert merges, name
        merge = merges[-1]
        waits = [i for i in range(merge + 1, t) if body[i].startswith("s_waitcnt") and re.search(r"\bvmcnt\(0\)", body[i])]
        ok = any(any(body[j].startswith("s_barrier") for j in range(w + 1, t)) for w in waits)
        span = [l for l in body[merge:t + 1] if l.startswith(("s_waitcnt", "s_barrier", "global_atomic", "buffer_"))]
        assert ok, (name, "no s_waitcnt vmcnt(0) between the last merge atomic and a barrier before the ticket", span)
