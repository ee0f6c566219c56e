"""A deterministic corpus of RepeatMasker listings for the annotation parser: (name, bytes) cases, and the expected rows of a text
from parse_rm's own read_repeatmasker (never from the code under test).  Shared by the host and GPU tests of
deepgrp_amd/annotation.py and by tools/bench_annotation.py (`generated`)."""
import io
import random

from deepgrp_amd._scripts import parse_rm

HEADER = ("   SW   perc perc perc  query     position in query    matching  repeat       position in repeat\n"
          "score   div. del. ins.  sequence  begin end   (left)   repeat    class/family  begin  end    (left)  ID\n"
          "\n")
FAMILIES = parse_rm.REPEATS
OTHER_FAMILIES = ("DNA/hAT-Charlie", "Low_complexity", "LTR/ERVK", "Simple_repeat", "Satellite", "Unknown", "LINE/CR1", "SINE/Alu2",
                  "LINE/L1x", "hsatii")


def out_line(ctg="chr1", begin=1001, end=1300, rep="AluY", fam="SINE/Alu", strand="+", tok0="1234", sep="  ", lead="  ", tail=True):
    toks = [tok0, "10.5", "0.3", "1.2", ctg, str(begin), str(end), "(1000)", strand, rep, fam]
    if tail:
        toks += ["1", "300", "(0)", "7"]
    return lead + sep.join(toks)


def rmsk_line(ctg="chr1", start=1000, end=1300, rep="AluY", cls="SINE", fam="Alu", strand="+", f0="585"):
    return "\t".join([f0, "1504", "13", "4", "13", ctg, str(start), str(end), "-248945422", strand, rep, cls, fam, "1", "300", "-10", "1"])


def text(lines, end="\n", last=True):
    """The lines joined by `end`; last: the final line is ended too."""
    return (end.join(lines) + (end if last and lines else "")).encode("ascii")


def port_rows(data: bytes):
    """[(contig, start, end, number, line from 1)] of parse_rm.read_repeatmasker on the text as the script reads its input
    (UTF-8, universal newlines)."""
    exact, one_off = parse_rm.pentamer_sets()
    at = [0]

    def numbered(fh):
        for k, line in enumerate(fh, 1):
            at[0] = k
            yield line
    fh = io.StringIO(data.decode("utf-8"), newline=None)
    return [(r.ctg, r.start, r.end, r.typ, at[0]) for r in parse_rm.read_repeatmasker(exact, one_off, numbered(fh))]


def grouped(rows):
    """{contig: [(start, end, number, line)]} of port_rows' list, file order within a contig, without the contigs that
    evaluation.read_annotation skips (a first column that opens with '#')."""
    out = {}
    for ctg, start, end, number, line in rows:
        if not ctg.startswith("#"):
            out.setdefault(ctg, []).append((start, end, number, line))
    return out


def one_off_of(word, k=2):
    return word[:k] + ("A" if word[k] != "A" else "C") + word[k + 1:]


def generated(n_lines: int, seed: int = 7, contigs: int = 5, rmsk: bool = True) -> bytes:
    """A listing of about n_lines lines sorted by contig: the header, `.out` lines of numbered and other families, satellite units,
    and (rmsk) some rmsk lines and junk."""
    rnd = random.Random(seed)
    exact = list(parse_rm.pentamer_sets()[0])
    lines = HEADER.rstrip("\n").split("\n") + [""]
    per = max(n_lines // contigs, 1)
    for c in range(contigs):
        ctg = f"chr{c + 1}" if c % 2 == 0 else f"scaffold_{c}_random"
        pos = 1
        for _ in range(per):
            pos += rnd.randrange(1, 5000)
            ln = rnd.randrange(10, 6000)
            kind = rnd.random()
            strand = rnd.choice("+C")
            score = str(rnd.randrange(200, 40000))
            if kind < 0.55:
                fam = rnd.choice(FAMILIES)
                line = out_line(ctg, pos, pos + ln, rnd.choice(("AluY", "L1PA4", "MIRb", "L2a", "MLT1B", "ALR/Alpha")), fam, strand, score,
                                sep=" " * rnd.randrange(1, 5), lead=" " * rnd.randrange(0, 4))
            elif kind < 0.80:
                line = out_line(ctg, pos, pos + ln, rnd.choice(("Charlie1", "(CA)n", "GA-rich", "HSATII", "AluSx")),
                                rnd.choice(OTHER_FAMILIES), strand, score, sep=" " * rnd.randrange(1, 4))
            elif kind < 0.90:
                unit = "".join(rnd.choice([rnd.choice(exact), one_off_of(rnd.choice(exact), rnd.randrange(5)), "ACGTA", "GGA"])
                               for _ in range(rnd.randrange(1, 5)))
                line = out_line(ctg, pos, pos + ln, f"({unit})n", rnd.choice(("Simple_repeat", "Satellite", "Satellite/centr")), strand,
                                score)
            elif kind < 0.97 and rmsk:
                cls, fam = rnd.choice((("SINE", "Alu"), ("LINE", "L1"), ("LTR", "ERVL-MaLR"), ("Satellite", "Satellite"), ("DNA", "hAT"),
                                       ("Simple_repeat", "Simple_repeat")))
                rep = rnd.choice(("AluJb", "L1M5", "(GGAAT)n", "(ATTCCATTCG)n", "HSATII"))
                line = rmsk_line(ctg, pos, pos + ln, rep, cls, fam, rnd.choice("+-"), str(rnd.randrange(585, 700)))
            else:
                line = rnd.choice(("", "# a comment", "   ", "There were no repetitive sequences detected in chrUn", score + " 1 2"))
            pos += ln
            lines.append(line)
    return text(lines)


def small_cases():
    kept = out_line()
    c = [("empty", b""),
         ("one_line", text([kept])),
         ("one_line_no_newline", text([kept], last=False)),
         ("header_only", HEADER.encode()),
         ("skipped_only", text(["", "# nothing", "chr1 10 20 3 AluY SINE/Alu", "1 2 3", out_line(fam="DNA/hAT")])),
         ("crlf", text([HEADER.split("\n")[0], kept, out_line(begin=5, end=9, fam="LINE/L1"), rmsk_line()], end="\r\n")),
         ("crlf_no_last", text([kept, rmsk_line(cls="LINE", fam="L2")], end="\r\n", last=False)),
         ("mixed_forms", text([kept, rmsk_line(), out_line(ctg="chr2", fam="LINE/L2"), rmsk_line(ctg="chr2", cls="LTR", fam="ERV1")])),
         ("blank_lines", b"\n\n\n" + text([kept]) + b"\n\n"),
         ("tabs_between_tokens", text([out_line(sep="\t"), out_line(sep=" \t ", lead="\t")]))]
    return c


def near_misses():
    good = out_line()
    return [
        ("tok0_letter", text([out_line(tok0="12a4"), good])),
        ("tok5_letter", text([out_line(begin="10x1"), good])),
        ("tok6_letter", text([out_line(end="13o0"), good])),
        ("tok8_minus", text([out_line(strand="-"), good])),
        ("tok8_lower_c", text([out_line(strand="c"), good])),
        ("tok8_two_bytes", text([out_line(strand="C+"), good])),
        ("ten_tokens", text([out_line(tail=False).rsplit(None, 1)[0], good])),
        ("eleven_tokens", text([out_line(tail=False), good])),
        ("rmsk_leading_space", text([" " + rmsk_line(), good])),
        ("rmsk_double_tab", text([rmsk_line().replace("\t", "\t\t", 1), rmsk_line().replace("chr1\t", "chr1\t\t"), good])),
        ("rmsk_space_in_field5", text([rmsk_line(ctg="chr 1"), good])),
        ("rmsk_space_in_field10", text([rmsk_line(rep="Alu Y"), good])),
        ("rmsk_field9_C", text([rmsk_line(strand="C"), good])),
        ("rmsk_twelve_fields", text(["\t".join(rmsk_line().split("\t")[:12]), good])),
        ("rmsk_thirteen_fields", text(["\t".join(rmsk_line().split("\t")[:13]), good])),
        ("rmsk_field12_then_space", text(["\t".join(rmsk_line().split("\t")[:13]) + " trailing words", good])),
        ("rmsk_field0_letter", text([rmsk_line(f0="58x"), good])),
        ("rmsk_field6_letter", text([rmsk_line(start="1o00"), good])),
        ("rmsk_class_equals_family", text([rmsk_line(rep="HSATII", cls="Satellite", fam="Satellite"), rmsk_line(cls="HSATII", fam="HSATII")])),
        ("rmsk_class_differs", text([rmsk_line(cls="SINE", fam="Alu"), rmsk_line(cls="SINE", fam="Alu2"), rmsk_line(cls="SINE/Alu", fam="SINE/Alu")])),
    ]


def classification():
    exact = list(parse_rm.pentamer_sets()[0])
    a, b = one_off_of(exact[0], 1), one_off_of(exact[3], 4)
    lines = [out_line(begin=10 * k + 1, end=10 * k + 9, rep="x", fam=f) for k, f in enumerate(FAMILIES)]
    lines += [out_line(begin=10 * k + 1, end=10 * k + 9, rep=f, fam="Other/thing") for k, f in enumerate(FAMILIES)]
    lines += [rmsk_line(rep=f, cls="Other", fam="thing") for f in FAMILIES]
    lines += [out_line(rep=r, fam=f) for r, f in (("HSATII", "Satellite"), ("HSATIIx", "Satellite"), ("xHSATII", "Satellite"),
                                                   ("SINE/Al", "x"), ("SINE/Alux", "x"), ("x", "SINE/alu"), ("x", "LTR/ERVL-MaL"))]
    units = ["GGAAT", "ATTCC", "GAATG", exact[7], "GGAATGGAGT", exact[2] + a, a + b, a, "GGAA", "GGAATG", "GGAATGGAAT" + "GGA", "ACGTA" + "GGAAT",
             "GGAAT" * 3 + a + "GGAAT"]
    for fam in ("Simple_repeat", "Satellite"):
        lines += [out_line(rep=f"({u})n", fam=fam) for u in units]
    lines += [out_line(rep="(GGAAT)n", fam=f) for f in ("Satellite/centr", "Low_complexity", "Simple_repeats", "simple_repeat")]
    lines += [out_line(rep=r, fam="Satellite") for r in ("(GGAAT)", "(GGAAT)m", "GGAAT)n", "(GGAAT", "()n", "(GGAAN)n", "(ggaat)n", "(GGAAT)nx",
                                                        "((GGAAT)n")]
    lines += [rmsk_line(rep="(GGAAT)n", cls="Simple_repeat", fam="Simple_repeat"), rmsk_line(rep="(GGAAT)n", cls="Satellite", fam="centr"),
              rmsk_line(rep="(ATTCCATTCG)n", cls="Satellite", fam="Satellite")]
    long_unit = ("GGAAT" + a) * 500                                  # 5 000 bases
    long_line = out_line(rep="x", fam="LINE/L1") + " " + "x" * 5000
    return [("classes_and_units", text(lines)),
            ("unit_5000", text([out_line(rep=f"({long_unit})n", fam="Satellite"), out_line(rep=f"({long_unit}A)n", fam="Satellite"),
                                out_line(rep=f"({(a + b) * 500})n", fam="Satellite")])),
            ("line_5000", text([long_line, "y" * 5000, out_line(fam="LINE/L2"), long_line]))]


def contig_cases():
    alt = [out_line(ctg=("chrA" if k % 2 == 0 else "chrB"), begin=k + 1, end=k + 50) for k in range(300)]
    return [("run_comes_back", text([out_line(ctg="chr1"), out_line(ctg="chr1", fam="LINE/L1"), out_line(ctg="chr10"),
                                     out_line(ctg="chr1", begin=7, end=8)])),
            ("last_byte_differs", text([out_line(ctg="chr1a"), out_line(ctg="chr1b"), out_line(ctg="chr1b"), out_line(ctg="chr2b")])),
            ("prefix_names", text([out_line(ctg="chr1"), out_line(ctg="chr"), out_line(ctg="chr11")])),
            ("hash_contig", text([out_line(ctg="#chr1"), out_line(ctg="chr#1"), out_line(ctg="#chr1")])),
            ("alternating_300", text(alt))]


def value_cases():
    return [("begin_zero", text([out_line(), out_line(begin=0, end=10)])),
            ("end_below_begin", text([out_line(begin=500, end=100), rmsk_line(start=500, end=100)])),
            ("eighteen_digits", text([out_line(begin="9" * 18, end="9" * 18), rmsk_line(start="1" + "0" * 17, end="9" * 18)])),
            ("leading_zeros", text([out_line(begin="00012", end="0099")]))]


def sized_text(n: int, tail_line: bool = False) -> bytes:
    """A listing of exactly n bytes whose last line is a numbered one that ends at byte n; tail_line: one more numbered line
    follows, so that it STARTS at byte n."""
    last = out_line(ctg="chrZ", begin=77, end=99, fam="LTR/Gypsy") + "\n"
    body, k = [], 0
    while sum(map(len, body)) < n - len(last) - 400:
        body.append(out_line(begin=100 * k + 1, end=100 * k + 60, fam=FAMILIES[k % len(FAMILIES)]) + "\n")
        k += 1
    fill = n - len(last) - sum(map(len, body))
    body.append("#" + "x" * (fill - 2) + "\n")
    data = ("".join(body) + last).encode("ascii")
    assert len(data) == n
    return data + ((out_line(ctg="chrZ", begin=5, end=6) + "\n").encode("ascii") if tail_line else b"")


def size_cases(tile: int):
    return [("generated_40000", generated(40_000)),
            ("tile_minus_1", sized_text(tile - 1)), ("tile", sized_text(tile)), ("tile_plus_1", sized_text(tile + 1)),
            ("line_starts_at_tile", sized_text(tile, tail_line=True)), ("two_tiles_plus_1", sized_text(2 * tile + 1)),
            ("newlines_only", b"\n" * 700 + text([out_line()])),
            ("chunk_edges", text([out_line(lead=" " * k) for k in range(130)]))]


def cases(tile: int):
    """Every case the device decides itself."""
    return small_cases() + near_misses() + classification() + contig_cases() + value_cases() + size_cases(tile)


def fallback_cases():
    """Files the device hands to the host: a byte 0xC3, a carriage return no line feed follows, a coordinate of 19 digits."""
    return [("byte_c3", (out_line() + "\n" + out_line(rep="Alué") + "\n").encode("utf-8")),
            ("lone_cr", (out_line() + "\r" + out_line(fam="LINE/L1") + "\n").encode("ascii")),
            ("cr_at_end", (out_line() + "\n" + out_line(fam="LINE/L1") + "\r").encode("ascii")),
            ("nineteen_digits", text([out_line(), out_line(begin="1" + "0" * 18, end="1" + "0" * 18)]))]
