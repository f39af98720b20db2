"""The wait counts of the fused kernel's gather pipeline, read from the code objects inside lib/libdvo_amd.so.

The compact-form sweeps of the 256-thread shapes keep each round's gathers two rounds ahead of the arithmetic that consumes them
(rgbd_odometry_amd/csrc/dvo_fused.hip: accumulate_points2, DEPTH == 3).  Whether they really do is decided by the `s_waitcnt vmcnt(N)`
the compiler places, not by the source: a prologue that issued its second round under a condition made the loop head wait vmcnt(0), and
once per trip of three rounds the pipeline was emptied.  CPU test, like tests/test_kernel_registers.py: it disassembles the embedded
gfx950 code object and walks every steady-state point loop of the four instantiations without H around its back edge, with the in-order
queue of outstanding vector-memory operations (tools/hotloop_stats.py: check_waits states the rule and why; `--waits` prints what this
test sees).

What is asserted, for every loop of three rounds per trip (the DEPTH == 3 loops; the two-round loops of the 512-thread shapes and of
the 16-byte texel forms are DEPTH == 2, another pipeline):
  * no vmcnt(0) in the loop;
  * a wait between a round's gathers and the accumulation behind them leaves the gathers of the two youngest rounds in flight, any
    other wait those of the youngest round (it may belong to the next round, which the scheduler lets begin early): 2 resp. 4 loads
    where the two gathers are a round's only loads, 4 resp. 8 loads -- and the 4 resp. 8 stores between them -- in the sweep that also
    writes the final outputs, where a round has four gathers and four stores;
  * in a loop that also fetches the next round's point words or chunk headers, one round less: those words are needed at the start of
    the next issue stage, and the in-order counter completes the gathers of the round before with them.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rgbd_odometry_amd", "lib", "libdvo_amd.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(OBJDUMP)), reason="library or llvm-objdump missing")


def _tool():
    spec = importlib.util.spec_from_file_location("hotloop_stats", os.path.join(ROOT, "tools", "hotloop_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fused_kernels():
    tool = _tool()
    return tool, tool.kernels(tool.disassemble(LIB))


def _instantiation(ks, block, team):
    k = [n for n in ks if "align_fused2_kernelILi%dELb%dELb0E" % (block, team) in n]
    assert len(k) == 1, k
    return ks[k[0]]


@pytest.mark.parametrize("team", [0, 1])
@pytest.mark.parametrize("block", [256, 512])
def test_gathers_stay_two_rounds_ahead(fused_kernels, block, team):
    tool, ks = fused_kernels
    loops = tool.point_loops(_instantiation(ks, block, team))
    assert len(loops) >= 6, [hex(L.head) for L in loops]                     # the point loops were found at all
    deep = [L for L in loops if L.rounds == 3]
    if block == 512:        # DVO_P4_DEPTH: one 512-thread workgroup exposes its serial phases, not its gathers -- no such loop to check
        assert not deep
        return
    # 8-byte, 4-byte direct and 4-byte block-relative points in LDS and the two streamed forms, in the full and in the residual-only
    # sweep, and the latter once more with the final outputs (a team reads 8-byte points only)
    full = [L for L in deep if not L.residual_only]
    res = [L for L in deep if L.residual_only and not L.final]
    fin = [L for L in deep if L.final]
    want = 2 if team else 5
    assert len(full) == want and len(res) == want and len({L.end for L in fin}) >= want, [(hex(L.head), L.kind()) for L in deep]
    assert sum(1 for L in full if L.resident) == (1 if team else 2) and sum(1 for L in res if L.resident) == (1 if team else 2)
    assert any(L.resident for L in fin)
    failed = {}
    for L in deep:
        events, bad = tool.check_waits(L)
        waits = [e for e in events if e[1].startswith("s_waitcnt")]
        assert waits, hex(L.head)
        if bad:
            failed["%x %s" % (L.head, L.kind())] = bad
    assert not failed, failed


def test_resident_loops_wait_for_no_less_than_one_round(fused_kernels):
    """the plain form of the rule for the loops whose only loads are the two gathers of each round: no wait below vmcnt(2)"""
    tool, ks = fused_kernels
    seen = 0
    for team in (0, 1):
        for L in tool.point_loops(_instantiation(ks, 256, team)):
            if L.rounds == 3 and L.resident and not L.final:
                ns = [tool.vmcnt_of(op, args) for a, op, args, t in L.path]
                ns = [n for n in ns if n is not None]
                assert ns and min(ns) >= 2, (hex(L.head), ns)
                seen += 1
    assert seen == 6
