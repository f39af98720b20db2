#!/usr/bin/env python3
"""Instruction mix of the steady-state point loops of align_fused2_kernel<256,false> (the loops that hold 6 = 3 rounds x 2 or 4 = 2 x 2
dwordx3 gathers) out of lib/libdvo_amd.so.  usage: tools/hotloop_stats.py [block] [-v] [--all] [--waits] [--code-object FILE]
`block` is matched as a prefix of the template arguments: `256` takes the first instantiation with 256 threads and no teams, `256ELb0` the
one without H (the headline).  --all lists every loop of 60..1500 instructions with its vector instructions and global loads instead: the
residual-only sweep of a level's last iteration has no dwordx3 gather (its steady-state loops hold 6 = 3 rounds x 2 single-dword gathers,
plus the loads of 4-byte points and chunk headers where the list has that form).

--waits prints, for every steady-state point loop (full and residual-only sweeps), the vector-memory instructions and the `s_waitcnt
vmcnt(N)` of one trip in program order, each wait with what it leaves in flight, and the verdict of check_waits() below:
tests/test_kernel_waits.py asserts that verdict.  --code-object FILE reads a stand-alone gfx950 code object (hipcc --cuda-device-only -c)
instead of the library."""
import os
import re
import struct
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rgbd_odometry_amd", "lib", "libdvo_amd.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def disassemble(path=LIB):
    """disassembly of every embedded gfx950 code object that holds align_fused2_kernel (of the file itself if it is a code object)"""
    data = open(path, "rb").read()
    text = ""
    with tempfile.TemporaryDirectory() as tmp:
        n = 0
        for m in re.finditer(b"\x7fELF\x02\x01\x01", data):
            o = m.start()
            if struct.unpack_from("<H", data, o + 18)[0] != 224:        # EM_AMDGPU
                continue
            shoff = struct.unpack_from("<Q", data, o + 0x28)[0]
            shentsize, shnum = struct.unpack_from("<HH", data, o + 0x3A)
            f = os.path.join(tmp, "co_%d.elf" % n)
            n += 1
            with open(f, "wb") as fh:
                fh.write(data[o:o + shoff + shentsize * shnum])
            out = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f], capture_output=True, text=True, check=True).stdout
            if "align_fused2_kernel" in out:
                text += out
    return text


def kernels(text):
    """{mangled name: [(address, opcode, operands, branch target address or None)]}"""
    out, cur, base = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(2), [])
            base = int(m.group(1), 16)
            continue
        if cur is None:
            continue
        m = re.search(r"^\s+(\S+)\s*(.*?)\s*// ([0-9A-F]+):(.*)$", line)
        if m:
            t = re.search(r"\+0x([0-9a-f]+)>", m.group(4))
            cur.append((int(m.group(3), 16), m.group(1), m.group(2), base + int(t.group(1), 16) if t and m.group(1).startswith("s_") else None))
    return out


def is_load(op):
    return op.startswith("global_load") or op.startswith("buffer_load")


def is_store(op):
    return op.startswith("global_store") or op.startswith("buffer_store") or op.startswith("global_atomic")


def is_fma64(op):
    return op.startswith("v_fma_f64") or op.startswith("v_fmac_f64")


def vmcnt_of(op, args):
    """N of an s_waitcnt that names vmcnt, else None"""
    if op != "s_waitcnt":
        return None
    m = re.search(r"vmcnt\((\d+)\)", args)
    return int(m.group(1)) if m else None


def hot_path(ins, head):
    """One trip of the loop whose head is at `head`, as the list of its instructions in the order a wave executes them when every rare
    block is skipped: every conditional branch to a later place inside the loop is taken.  The forward conditional branches of the point loops guard one thing only, the
    patch of a partial compact form in the compute stage of the residual-only sweep that writes the final outputs (final2_store), and
    the first conditional branch back to the head is the loop's own.  None if the walk does not come back to `head`."""
    idx = {x[0]: i for i, x in enumerate(ins)}
    last = max(a for a, op, args, t in ins if t == head and a >= head)           # the loop's last branch back to its head
    i, path = idx[head], []
    while len(path) < 1500:
        a, op, args, tgt = ins[i]
        path.append(ins[i])
        if op in ("s_endpgm", "s_setpc_b64"):
            return None
        if tgt is not None and (op.startswith("s_cbranch") or op == "s_branch"):
            if tgt == head:
                return path
            if tgt in idx and a < tgt <= last:
                i = idx[tgt]
                continue
            if op == "s_branch":
                return None
        i += 1
        if i >= len(ins):
            return None
    return None


class PointLoop:
    """a steady-state loop of the software pipeline over rounds of points: `rounds` rounds per trip, `per_round` vector-memory loads
    per round; `gathers` of them -- the last ones of a round's issue stage -- are the round's gathers of rank words"""

    def __init__(self, head, path):
        self.head, self.path, self.end = head, path, path[-1][0]
        c = Counter(x[1] for x in path)
        self.x3 = c["global_load_dwordx3"]
        self.loads = sum(n for o, n in c.items() if is_load(o))
        self.stores = sum(n for o, n in c.items() if is_store(o))
        self.fma64 = sum(n for o, n in c.items() if is_fma64(o))
        self.valu = sum(n for o, n in c.items() if o.startswith("v_"))
        # a full round adds two points to 7 double sums (14 v_fma_f64), a residual-only round to one (2)
        self.residual_only = self.x3 == 0
        self.rounds = self.x3 // 2 if self.x3 else self.fma64 // 2
        ok = self.rounds in (2, 3) and self.loads % self.rounds == 0 and self.fma64 == self.rounds * (2 if self.residual_only else 14)
        self.per_round = self.loads // self.rounds if ok else 0
        self.final = self.residual_only and self.stores > 0            # RoundEF: the same points once more at the best-so-far pose
        self.gathers = 4 if self.final else 2
        self.ok = ok and self.per_round >= self.gathers
        # `resident`: the round's gathers are its only loads.  A loop that also loads the next round's points or chunk headers (fetched
        # a round ahead, used at the start of the next issue stage) cannot keep two rounds of gathers in flight: the counter is in order,
        # so the wait for those words also completes every gather issued before them
        self.resident = self.ok and self.per_round == self.gathers

    def kind(self):
        return "%s sweep%s, %d rounds per trip, %d loads per round%s" % (
            "residual-only" if self.residual_only else "full", " with final outputs" if self.final else "", self.rounds, self.per_round,
            "" if self.resident else " (%d of them point words or chunk headers fetched a round ahead)" % (self.per_round - self.gathers))


def point_loops(ins):
    heads = sorted({t for a, op, args, t in ins if (op.startswith("s_cbranch") or op == "s_branch") and t is not None and t <= a})
    out = []
    for h in heads:
        p = hot_path(ins, h)
        if p is None:
            continue
        L = PointLoop(h, p)
        if L.ok:
            out.append(L)
    return out


def check_waits(L):
    """Walks the loop's hot path three times around the back edge (the first two trips fill the queue) with the in-order queue of
    outstanding vector-memory operations: `s_waitcnt vmcnt(N)` leaves the youngest N in flight.  Returns (events, violations).

    The pipeline keeps the gathers of `rounds` rounds in registers: the round that is being computed and `rounds - 1` younger ones.  A
    slot of the loop is `issue round X; compute round X - (rounds - 1)`.  The rule, per wait:
      a. between a round's last load and the first v_fma_f64 behind it -- the accumulation of the round that slot computes -- the wait
         is that compute stage's: it may complete the round it computes and nothing younger, so the loads of the `rounds - 1` youngest
         rounds stay in flight;
      b. any other wait (in front of a round's loads, or behind the accumulation: the scheduler lets the next slot begin early) may
         also complete the next round to be computed, so the loads of the `rounds - 2` youngest rounds stay in flight -- and a round
         whose loads have only begun to issue counts as one more round on top of these, with what it has issued;
      c. never vmcnt(0).
    In a loop that is not `resident` (see PointLoop) only the round's gathers, its last loads, are required to stay in flight, and
    of one round less: its words fetched a round ahead are waited for at the start of the next issue stage, and the in-order
    counter completes the gathers of the round before with them."""
    keep_a, keep_b = L.rounds - 1, L.rounds - 2
    if not L.resident:
        keep_a, keep_b = max(keep_a - 1, 0), max(keep_b - 1, 0)
    queue, events, bad = [], [], []
    n_loads, fma_since_load = 0, True
    for trip in range(3):
        for a, op, args, _ in L.path:
            if is_load(op):
                g, k = divmod(n_loads, L.per_round)
                queue.append(("load", g, k >= L.per_round - L.gathers or L.resident, a))
                n_loads += 1
                fma_since_load = False
                if trip == 2:
                    events.append((a, "%s %s" % (op, args), None))
            elif is_store(op):
                queue.append(("store", -1, False, a))
                if trip == 2:
                    events.append((a, "%s %s" % (op, args), None))
            elif is_fma64(op):
                fma_since_load = True
            else:
                n = vmcnt_of(op, args)
                if n is None or trip < 2:
                    if n is not None:
                        del queue[:max(len(queue) - n, 0)]
                    continue
                left = queue[max(len(queue) - n, 0):] if n else []
                cur, k = divmod(n_loads - 1, L.per_round)
                begun = k + 1 < L.per_round
                stage_a = not fma_since_load and not begun
                keep = keep_a if stage_a else keep_b + (1 if begun else 0)
                need = [q for q in queue if q[0] == "load" and q[2] and q[1] > cur - keep]
                lost = [q for q in need if q not in left]
                why = []
                if n == 0:
                    why.append("vmcnt(0)")
                if lost:
                    why.append("completes %d gather(s) of the %d youngest round(s)" % (len(lost), keep))
                events.append((a, "s_waitcnt vmcnt(%d)" % n, "leaves %d load(s), %d store(s); rule %s%s" % (
                    sum(1 for q in left if q[0] == "load"), sum(1 for q in left if q[0] == "store"), "a" if stage_a else "b",
                    "  <-- " + ", ".join(why) if why else "")))
                if why:
                    bad.append((hex(a), n, ", ".join(why)))
                del queue[:max(len(queue) - n, 0)]
    return events, bad


def main(argv):
    block = argv[1] if len(argv) > 1 and not argv[1].startswith("-") else "256"
    src = argv[argv.index("--code-object") + 1] if "--code-object" in argv else LIB
    ks = kernels(disassemble(src))
    ins = next((v for k, v in ks.items() if ("align_fused2_kernelILi%sELb0E" % block) in k), None)
    if ins is None:
        sys.exit("no align_fused2_kernel<%s..., false> in %s" % (block, src))
    if "--waits" in argv:
        for L in point_loops(ins):
            events, bad = check_waits(L)
            print("loop %x..%x: %s: %s" % (L.head, L.end, L.kind(), "FAILS" if bad else "ok"))
            for a, what, note in events:
                print("   %x  %-60s %s" % (a, what, note or ""))
        return
    idx = {x[0]: i for i, x in enumerate(ins)}
    for i, (a, op, args, tgt) in enumerate(ins):
        if not op.startswith("s_cbranch") or tgt is None: continue
        if tgt > a or tgt not in idx: continue
        body = ins[idx[tgt]:i + 1]
        if "--all" in argv:
            if 60 <= len(body) <= 1500:
                c = Counter(x[1] for x in body)
                print("loop %x..%x: %d instructions, VALU %d, LDS %d, global_load dwordx3 %d, dwordx2 %d, dword %d, scratch %d" % (
                    tgt, a, len(body), sum(n for o, n in c.items() if o.startswith("v_")), sum(n for o, n in c.items() if o.startswith("ds_")),
                    c["global_load_dwordx3"], c["global_load_dwordx2"], c["global_load_dword"], sum(n for o, n in c.items() if o.startswith("scratch"))))
            continue
        ng = sum(1 for x in body if x[1] == "global_load_dwordx3")
        if ng not in (4, 6) or len(body) > 1200: continue
        rounds = ng // 2
        c = Counter(x[1] for x in body)
        valu = sum(n for o, n in c.items() if o.startswith("v_"))
        print("loop %x..%x: %d instructions, %d rounds: VALU %.1f / round, LDS %.1f, SALU %.1f, VMEM %.1f, scratch %d" % (
            tgt, a, len(body), rounds, valu / rounds, sum(n for o, n in c.items() if o.startswith("ds_")) / rounds,
            sum(n for o, n in c.items() if o.startswith("s_") and o != "s_waitcnt") / rounds,
            sum(n for o, n in c.items() if o.startswith("global_") or o.startswith("buffer_")) / rounds, sum(n for o, n in c.items() if o.startswith("scratch"))))
        if "-v" in argv:
            for o, n in c.most_common(60): print("   %4d %s" % (n, o))


if __name__ == "__main__":
    main(sys.argv)
