#!/usr/bin/env python3
"""What every s_waitcnt in gru_split2_kernel's time loop waits for, read from the compiler's device assembly.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 -fno-slp-vectorize --cuda-device-only -S deepgrp_amd/csrc/gru_split2.hip -o dev.s
    python tools/split2_wait_audit.py dev.s [--kernel gru_split2_kernelILi0ELb1E] [--inc deepgrp_amd/csrc/gru_split2_phase.inc]

The time loop is the innermost loop of the kernel that holds 300 MFMAs (two phases of 150).  It is walked in text order, twice, so that
what the back edge carries into a trip (RD0's fragments, a store of the last gaps) is in flight at its head.  LDS operations and scalar
memory reads count on lgkmcnt and return in order; `s_waitcnt lgkmcnt(N)` waits for all but the youngest N.  For every wait the table
names the YOUNGEST operation it still has to wait for -- the one that decides how long it stalls -- and the distance from that
operation's issue to the wait in MFMAs (16 cycles of the matrix pipe each) and in instructions, and the generated gap the wait sits in:
gap g of a phase = the code between the sched_barrier comments g - 1 and g = line g of gru_split2_phase.inc (its macros are printed
when --inc is given).  A wait that finds nothing left to wait for is listed as such.  vmcnt / expcnt fields are printed as they stand.

A report, never a check: the exit status is 0 whenever the loop was found."""
import argparse
import re
import sys

LGKM = re.compile(r"^(ds_|s_load_|s_buffer_load_|s_memtime|s_memrealtime|s_sendmsg)")


def loop_body(path, pattern):
    """instructions (text, is sched_barrier comment) of the innermost loop holding 300 MFMAs in the first kernel matching `pattern`"""
    lines, inside = [], False
    with open(path) as fh:
        for raw in fh:
            if not inside:
                inside = bool(re.match(r"^\S+:", raw)) and pattern in raw.split(":")[0] and not raw.startswith(".")
                continue
            t = raw.strip()
            if t.startswith("s_endpgm"):
                break
            lines.append(t)
    labels = {m.group(1): i for i, t in enumerate(lines) if (m := re.match(r"^(\.L\w+):", t))}
    best = None
    for i, t in enumerate(lines):
        m = re.match(r"^s_cbranch_\w+\s+(\.L\w+)|^s_branch\s+(\.L\w+)", t)
        if not m:
            continue
        head = labels.get(m.group(1) or m.group(2))
        if head is None or head > i:
            continue
        n = sum(1 for x in lines[head:i] if x.startswith("v_mfma"))
        if n == 300 and (best is None or i - head < best[1] - best[0]):
            best = (head, i)
    if best is None:
        return None
    return lines[best[0]:best[1] + 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="gru_split2_kernelILi0ELb1E")
    ap.add_argument("--inc", help="gru_split2_phase.inc: print each gap's macros beside its waits")
    a = ap.parse_args()
    body = loop_body(a.asm, a.kernel)
    if body is None:
        print(f"no loop of 300 MFMAs in a kernel matching {a.kernel!r} in {a.asm}")
        return 2
    gaps = []
    if a.inc:
        with open(a.inc) as fh:
            gaps = [ln.strip() for ln in fh if ln.strip() and not ln.startswith("//")]
    ins = [t.split(";")[0].strip() for t in body]
    kinds = {}
    for t in ins:
        if t and not t.endswith(":") and not t.startswith((".", ";")):
            mn = t.split()[0]
            if mn.startswith(("ds_", "v_mfma", "s_waitcnt", "s_barrier")):
                kinds[mn] = kinds.get(mn, 0) + 1
    print(f"time loop of {a.kernel}: " + ", ".join(f"{n} {mn}" for mn, n in sorted(kinds.items())))
    real = [t.split()[0] for t in ins if t and not t.endswith(":") and not t.startswith((".", ";"))]
    print(f"  {len(real)} instructions a trip: {sum(m.startswith('v_mfma') for m in real)} MFMA, "
          f"{sum(m.startswith('v_') and not m.startswith('v_mfma') for m in real)} other vector ALU, {sum(m.startswith('ds_') for m in real)} LDS, "
          f"{sum(m.startswith('s_') for m in real)} scalar (s_waitcnt, s_nop and branches included)")
    print(f"{'phase':5s} {'gap':>3s} {'mfma':>4s}  {'wait':34s} {'youngest operation waited for':44s} {'issued in':>9s} {'MFMAs':>5s} {'insts':>5s}  gap's macros")
    queue = []                                    # (text, mfma count at issue, instruction count at issue, where)
    nm = ni = 0
    close = []
    for trip in range(2):
        nsb = 0
        trip_m0 = nm
        for raw, t in zip(body, ins):
            if "sched_barrier" in raw:
                nsb += 1
                continue
            if not t or t.endswith(":") or t.startswith((".", ";")):
                continue
            mn = t.split()[0]
            ni += 1
            phase, gap = ("A", nsb) if nsb < 150 else ("B", nsb - 150) if nsb < 300 else ("edge", nsb - 300)
            where = f"{phase}{gap}"
            if mn.startswith("v_mfma"):
                nm += 1
            elif LGKM.match(mn):
                queue.append((t, nm, ni, where))
            elif mn == "s_waitcnt":
                m = re.search(r"lgkmcnt\((\d+)\)", t)
                if m is None:
                    if trip:
                        print(f"{phase:5s} {gap:3d} {nm - trip_m0:4d}  {t:34s} (no lgkmcnt field)")
                    continue
                keep = int(m.group(1))
                waited = queue[:len(queue) - keep] if keep else queue[:]
                queue = queue[len(queue) - keep:] if keep and len(queue) > keep else ([] if not keep else queue)
                if not trip:
                    continue
                macros = gaps[gap] if phase != "edge" and gap < len(gaps) else ""
                if not waited:
                    print(f"{phase:5s} {gap:3d} {nm - trip_m0:4d}  {t:34s} {'(nothing left in flight)':44s} {'':>9s} {'':>5s} {'':>5s}  {macros}")
                    continue
                op, m0, i0, w0 = waited[-1]
                print(f"{phase:5s} {gap:3d} {nm - trip_m0:4d}  {t:34s} {op[:44]:44s} {w0:>9s} {nm - m0:5d} {ni - i0 - 1:5d}  {macros}")
                if nm - m0 < 8:
                    close.append((where, t, op, nm - m0))
    print(f"\n{len(close)} wait(s) with fewer than 8 MFMAs between the operation and the wait:")
    for where, t, op, d in close:
        print(f"  {where:>6s}  {t:30s} <- {op}  ({d} MFMAs)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
