"""Build tools/gff_line_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer and run it over the corpus of
tests/gff_in_cases.py: the line function of dgrp_gff_parse (csrc/gff_line.h) on the CPU, every text in a heap block of exactly its
size.  What the program prints is compared with the expectations of the corpus; exit status 1 when a case differs or the
sanitizers report.  A CPU-only check: nothing here touches a GPU and nothing sanitized is loaded into Python.

    python tools/gff_line_check.py [--cxx g++ | --hipcc hipcc]"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="g++")
    ap.add_argument("--hipcc", default=None, metavar="HIPCC", help="build with this hipcc (-x hip, -Xarch_host sanitizers) instead")
    args = ap.parse_args()
    from gff_in_cases import CASES, UNDECIDED

    from deepgrp_amd import gffin
    failed = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gff_line_check")
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        if args.hipcc:                                               # the file as HIP: the functions are __host__ __device__, the host side sanitized
            san = ["-x", "hip", "--offload-arch=gfx950"] + [x for f in san for x in ("-Xarch_host", f)]
        subprocess.run([args.hipcc or args.cxx, "-std=c++17", "-O1", "-g"] + san +
                       ["-I", os.path.join(ROOT, "deepgrp_amd", "csrc"), os.path.join(ROOT, "tools", "gff_line_check.cpp"), "-o", exe], check=True)
        for name, case in CASES.items():
            text, table = os.path.join(tmp, "text"), os.path.join(tmp, "table")
            with open(text, "wb") as fh:
                fh.write(case.text)
            blob, off, number, count = gffin.names_table(case.names)
            with open(table, "wb") as fh:
                for k in range(count):
                    fh.write(b"%d\t%s\n" % (number[k], blob[off[k]:off[k + 1]].tobytes()))
            r = subprocess.run([exe, text, table] + ([case.key.decode()] if case.key else []), capture_output=True, text=True)
            out = [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
            ok = r.returncode == 0 and not r.stderr and out
            if ok and case.want == UNDECIDED:
                ok = out[0][3] == 1
            elif ok and case.want[0] == "malformed":
                ok = out[0][3] == 0 and out[0][4] == case.want[1]
            elif ok:
                lines, end_at, rows = case.want
                got = [(ln, case.text[pos:pos + size], b, e, n) for ln, b, e, n, pos, size in out[1:]]
                ok = out[0] == [lines, len(rows), end_at, 0, 0] and got == list(rows)
            if not ok:
                failed += 1
                print(f"FAILED {name}: exit {r.returncode}\n{r.stdout[:400]}\n{r.stderr[:2000]}")
    print(f"{len(CASES) - failed} of {len(CASES)} cases agree")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
