"""predict --seq_dir on the GPU: dgrp_fasta_extract_batch, repeatseq.write_repeat_fasta and the command line against the statement
of tests/seq_extract_cases.py (Python integers and slices over the file's bytes)."""
import ctypes as C
import functools
import gzip
import logging
import os

import numpy as np
import pytest

import seq_extract_cases as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])
ENTRY = np.dtype([("text_off", "<i8"), ("base_off", "<i8"), ("bases", "<i8")])
GUARD = 0xA5
BITS = sum(1 << c for c in sc.CLASSES)


@functools.lru_cache(maxsize=None)
def _case():
    """The kernel test's buffer and tables, and the sequence of every body by the statement's own walk (made once)."""
    buf, offs, lens, names, rowsets = sc.kernel_case()
    assert len(buf) < 2_000_000
    seqs = []
    for k in range(len(offs)):
        got = sc.sequences(b">n\n" + buf[offs[k]:offs[k] + lens[k]])
        seqs.append((names[k], got[0][1]))
    allrows = np.array([(s, e, lab, k) for k, rows in enumerate(rowsets) for s, e, lab in rows], SEG)
    row_off = np.zeros(len(offs) + 1, np.int64)
    np.cumsum([len(r) for r in rowsets], out=row_off[1:])
    name_off = np.zeros(len(offs) + 1, np.int64)
    np.cumsum([len(n) for n in names], out=name_off[1:])
    return dict(buf=buf, h_off=np.array(offs, np.int64), h_len=np.array(lens, np.int64), rows=allrows, row_off=row_off,
                names=b"".join(names), name_off=name_off, seqs=seqs, rowsets=rowsets)


@functools.lru_cache(maxsize=None)
def _want(flank, width):
    c = _case()
    return sc.brute_extract(b"", c["rowsets"], flank, width, sc.CLASSES, seqs=c["seqs"])


def _run(c, flank, width, cap=None, extra=4096, entries=True, rows=None, row_off=None):
    """One call of the entry on the case's buffer; d_text and d_entries are filled with a guard byte first.
    -> (rc, size, kept, d_text as bytes, d_entries as bytes)"""
    from deepgrp_amd._lib import lib
    L = lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = c["rows"] if rows is None else rows
    row_off = c["row_off"] if row_off is None else row_off
    d_raw = torch.from_numpy(np.frombuffer(c["buf"], np.uint8).copy()).to(dev)
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
    d_names = torch.from_numpy(np.frombuffer(c["names"] + b"\0", np.uint8).copy()).to(dev)
    nrec = len(c["h_off"])
    wb = L.dgrp_fasta_extract_workspace_bytes(nrec, int(c["h_len"].sum()), len(rows))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    cap = len(_want(flank, width)) if cap is None else cap
    d_text = torch.full((cap + extra,), GUARD, dtype=torch.uint8, device=dev)
    d_entries = torch.full((max(len(rows), 1) * ENTRY.itemsize,), GUARD, dtype=torch.uint8, device=dev)
    size, kept = C.c_int64(-1), C.c_int64(-1)
    rc = L.dgrp_fasta_extract_batch(d_raw.data_ptr(), nrec, c["h_off"].ctypes.data, c["h_len"].ctypes.data, d_rows.data_ptr(),
                                    row_off.ctypes.data, d_names.data_ptr(), c["name_off"].ctypes.data, flank, width, BITS,
                                    d_text.data_ptr(), cap, C.byref(size), d_entries.data_ptr() if entries else None, C.byref(kept),
                                    work.data_ptr(), wb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.current_stream().synchronize()
    return rc, size.value, kept.value, d_text.cpu().numpy().tobytes(), d_entries.cpu().numpy().tobytes(), L.dgrp_last_error().decode()


def _check(c, flank, width, out):
    rc, size, kept, text, entries, msg = out
    want = _want(flank, width)
    assert rc == 0, msg
    assert size == len(want)
    got_text = text[:size]
    first_diff = next((i for i in range(len(want)) if got_text[i] != want[i]), None) if got_text != want else None
    assert first_diff is None, (first_diff, got_text[max(first_diff - 40, 0):first_diff + 40], want[max(first_diff - 40, 0):first_diff + 40])
    assert text[size:] == bytes([GUARD]) * (len(text) - size)          # nothing at or beyond the size is written
    ent = sc.brute_entries(want)
    assert kept == len(ent) == sum(1 for rows in c["rowsets"] for r in rows if r[2] in sc.CLASSES)
    got = np.frombuffer(entries, ENTRY)
    assert got[:kept].tolist() == ent
    assert entries[kept * ENTRY.itemsize:] == bytes([GUARD]) * (len(entries) - kept * ENTRY.itemsize)


@pytest.mark.parametrize("width", sc.WIDTHS)
@pytest.mark.parametrize("flank", sc.FLANKS)
def test_extract_batch_kernel_against_the_statement(flank, width):
    """Every body at every alignment, CRLF and LF, with and without the last line end; the whole body, the first and the last base,
    more than 256 one-base rows in one source tile, one row over more than 20 source and output tiles, rows outside the class mask
    between kept ones; the clamp of the flank at both ends, flanks over neighbours, a width larger than any row."""
    c = _case()
    if flank == 0 and width == 60:
        long_row = [r for r in c["rowsets"][sc.LONG] if r[1] - r[0] > 20 * sc.TILE]
        assert long_row and long_row[0][2] in sc.CLASSES
    _check(c, flank, width, _run(c, flank, width))


def test_extract_batch_on_another_stream_and_without_entries():
    c = _case()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = _run(c, 1, 7)
    _check(c, 1, 7, out)
    rc, size, kept, text, entries, msg = _run(c, 0, 60, entries=False)
    assert rc == 0 and text[:size] == _want(0, 60) and entries == bytes([GUARD]) * len(entries)


def test_extract_batch_capacity():
    """text_cap == size succeeds; one byte less is DGRP_ENOMEM with the size reported and nothing written."""
    c = _case()
    want = _want(5000, 7)
    _check(c, 5000, 7, _run(c, 5000, 7, cap=len(want), extra=0))
    rc, size, kept, text, entries, msg = _run(c, 5000, 7, cap=len(want) - 1, extra=4096)
    assert rc == -3 and size == len(want) and kept == len(sc.brute_entries(want)) and "d_text holds" in msg
    assert text == bytes([GUARD]) * len(text) and entries == bytes([GUARD]) * len(entries)


@pytest.mark.parametrize("what", ["beyond", "empty", "order"])
def test_extract_batch_refuses_a_bad_row(what):
    """A row beyond its sequence, an empty row, rows out of order: DGRP_EINVAL naming the row, d_text and d_entries untouched."""
    c = _case()
    rows = c["rows"].copy()
    k = 12                                                               # a random body with rows
    lo, hi = int(c["row_off"][k]), int(c["row_off"][k + 1])
    assert hi - lo >= 2
    n = len(c["seqs"][k][1])
    if what == "beyond":
        bad = hi - 1
        rows[bad]["end"] = n + 1
    elif what == "empty":
        bad = lo + 1
        rows[bad]["end"] = rows[bad]["start"]
    else:
        bad = lo
        rows[lo]["end"] = rows[lo + 1]["start"] + 1
    rc, size, kept, text, entries, msg = _run(c, 1, 60, rows=rows)
    assert rc == -1 and f"row {bad} " in msg and f"of record {k} " in msg and f"sequence of {n} characters" in msg
    assert text == bytes([GUARD]) * len(text) and entries == bytes([GUARD]) * len(entries)


def test_extract_batch_takes_any_sub_range_of_the_rows():
    """h_row_off may select a sub-range of every record's rows: the pieces of a split call are the text of one call."""
    c = _case()
    want = _want(1, 60)
    n = len(c["rows"])
    got = b""
    for lo, hi in ((0, 7), (7, n // 2), (n // 2, n)):
        rc, size, kept, text, entries, msg = _run(c, 1, 60, cap=len(want), row_off=np.clip(c["row_off"], lo, hi).astype(np.int64))
        assert rc == 0, msg
        got += text[:size]
    assert got == want


# ---------------------------------------------------------------- write_repeat_fasta
def _rows_array(per):
    return np.array([(s, e, lab, k) for k, rows in enumerate(per) for s, e, lab in rows], SEG)


@pytest.mark.parametrize("flank,width,classes", [(0, 60, None), (40, 7, (1, 3))])
def test_write_repeat_fasta_mixed_file(tmp_path, monkeypatch, caplog, flank, width, classes):
    """Plain and odd records, CRLF, an empty record: groups and pieces cut at every possible place give the bytes of one call, the
    statement's bytes; the .fai is the statement's and locates every record's bases; the BGZF form inflates to the same bytes."""
    from deepgrp_amd import gz, repeatseq
    data = sc.odd_records_file()
    fa = tmp_path / "in.fa"
    fa.write_bytes(data)
    per = sc.rows_for(data)
    rows = _rows_array(per)
    want = sc.brute_extract(data, per, flank, width, classes)
    assert want.count(b">") > 20
    one = tmp_path / "one.fa"
    with caplog.at_level(logging.WARNING):
        n = repeatseq.write_repeat_fasta(str(fa), str(one), rows, classes=classes, flank=flank, width=width, fai_path=str(one) + ".fai")
    assert n == len(want) and one.read_bytes() == want
    assert caplog.text.count("nonascii") == 1
    fai = (tmp_path / "one.fa.fai").read_bytes()
    assert fai == sc.brute_fai(want)
    for line in fai.split(b"\n")[:-1]:
        name, bases, off, w, w1 = line.split(b"\t")
        bases, off, w = int(bases), int(off), int(w)
        at = want.rindex(b">", 0, off)
        assert want[at + 1:off - 1].split()[0] == name and int(w1) == w + 1 == min(width, bases) + 1
        seq = want[off:off + bases + (bases - 1) // w].replace(b"\n", b"")
        a, b = (int(x) for x in name.rsplit(b":", 1)[1].split(b"-"))
        assert len(seq) == bases == b - a
    monkeypatch.setattr(repeatseq, "SEQ_PIECE", 3000)
    for group_bytes in (1, 700, 6000, 1 << 20):
        cut = tmp_path / f"cut{group_bytes}.fa"
        repeatseq.write_repeat_fasta(str(fa), str(cut), rows, classes=classes, flank=flank, width=width, fai_path=str(cut) + ".fai",
                                     group_bytes=group_bytes)
        assert cut.read_bytes() == want and (tmp_path / f"cut{group_bytes}.fa.fai").read_bytes() == fai
    packed = tmp_path / "one.fa.gz"
    repeatseq.write_repeat_fasta(str(fa), str(packed), rows, classes=classes, flank=flank, width=width, compress=True, group_bytes=6000)
    assert gzip.decompress(packed.read_bytes()) == want and packed.read_bytes().endswith(gz.BGZF_EOF)
    # a row beyond its record: no file, no staged file
    bad = rows.copy()
    bad[-1]["end"] += 5
    for group_bytes in (256 << 20, 700):
        with pytest.raises(Exception, match="beyond"):
            repeatseq.write_repeat_fasta(str(fa), str(tmp_path / "bad.fa"), bad, fai_path=str(tmp_path / "bad.fa.fai"), group_bytes=group_bytes)
    assert sorted(os.listdir(tmp_path)) == sorted(["in.fa", "one.fa", "one.fa.fai", "one.fa.gz"] +
                                                  [f"cut{g}.fa{x}" for g in (1, 700, 6000, 1 << 20) for x in ("", ".fai")])


# ---------------------------------------------------------------- the command line
FLAGS = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]


def _cli_file(rng, T) -> bytes:
    seq = lambda n, alpha="ACGT": "".join(rng.choice(list(alpha), size=n))
    parts = [b"lines before the first header\n"]
    s1 = "NNNNN" + seq(4000, "ACGTacgt") + "NN"
    parts.append(b">chr1 some description\n" + "\n".join(s1[i:i + 60] for i in range(0, len(s1), 60)).encode() + b"\n")
    parts.append(b">short\n" + seq(T - 3).encode() + b"\n")
    s3 = seq(1500, "acgtRY")
    parts.append(b">chr3\r\n" + "\r\n".join(s3[i:i + 70] for i in range(0, len(s3), 70)).encode() + b"\r\n")
    s4 = seq(2500)
    parts.append(b">odd\n" + "\n".join(" " + s4[i:i + 50] + "\t" for i in range(0, len(s4), 50)).encode() + b"\n")
    parts.append(b">\nACGTACGT\n")
    s5 = seq(3000)
    parts.append(b">tail\n" + "\n".join(s5[i:i + 60] for i in range(0, len(s5), 60)).encode())
    return b"".join(parts)


def _tsv_rows(tsv: bytes, data: bytes):
    """The rows of the TSV per record of `data` (by the first word of the header column)."""
    names = [n for n, _p in sc.brute_records(data)]
    assert len(set(names)) == len(names)
    per = [[] for _ in names]
    for line in tsv.split(b"\n")[:-1]:
        _file, header, start, end, label = line.split(b"\t")
        per[names.index(header.split()[0])].append((int(start), int(end), int(label)))
    return per


@pytest.mark.parametrize("model_name,use_mss", [("model_u16_T30_att_vlen.h5", True), ("model_u8_T20.h5", False)])
def test_cli_seq_dir_end_to_end(tmp_path, model_name, use_mss):
    import twobit_corpus as tc
    from deepgrp_amd import gz
    from deepgrp_amd.__main__ import main
    rng = np.random.default_rng(21)
    model_file = os.path.join(GOLDEN, model_name)
    T = 30 if "T30" in model_name else 20
    data = _cli_file(rng, T)
    fa = tmp_path / "in.fa"
    fa.write_bytes(data)
    tail = [] if use_mss else ["-m"]

    def run(inp, tag, *extra):
        d = tmp_path / tag
        main(FLAGS + ["predict", model_file, str(inp), "--output", str(d) + ".tsv", "--seq_dir", str(d)] + list(extra) + tail)
        return (tmp_path / f"{tag}.tsv").read_bytes(), {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}

    plain_tsv = tmp_path / "plain.tsv"
    main(FLAGS + ["predict", model_file, str(fa), "--output", str(plain_tsv)] + tail)
    tsv, files = run(fa, "a", "--seq_fai")
    assert tsv == plain_tsv.read_bytes()
    per = _tsv_rows(tsv, data)
    assert sum(len(r) for r in per) > 3
    want = sc.brute_extract(data, per)
    assert list(files) == ["in.fa.repeats.fa", "in.fa.repeats.fa.fai"]
    assert files["in.fa.repeats.fa"] == want and files["in.fa.repeats.fa.fai"] == sc.brute_fai(want)
    # BGZF output: Python's gzip and the library's own host inflate give the bytes; members of at most 64 KiB, then the EOF member
    _tsv, files = run(fa, "b", "--seq_gzip", "--gzip_level", "1")
    assert list(files) == ["in.fa.repeats.fa.gz"]
    packed = files["in.fa.repeats.fa.gz"]
    assert gzip.decompress(packed) == want and bytes(gz.inflate_host(packed, "b", 1 << 30)) == want
    members = gz.walk_members(packed, "b")
    assert members.kind == "bgzf" and int(members.isize.max()) <= 1 << 16 and packed.endswith(gz.BGZF_EOF)
    # the options reach the file (the README form takes them too)
    seen = sorted({r[2] for rows in per for r in rows})
    classes = tuple(sorted(seen[:1] + [c for c in range(1, seen[-1]) if c not in seen][:1]))   # a label of the TSV, and one that is not in it
    main(["--seq_dir", str(tmp_path / "c"), "--seq_classes", ",".join(map(str, classes)), "--seq_flank", "25", "--seq_width", "50"] + FLAGS +
         [model_file, str(fa), "--output", str(tmp_path / "c.tsv")] + tail)
    assert (tmp_path / "c" / "in.fa.repeats.fa").read_bytes() == sc.brute_extract(data, per, 25, 50, classes)
    assert sc.brute_extract(data, per, 25, 50, classes) not in (want, b"")
    if len(seen) > 1:
        assert sc.brute_extract(data, per, 25, 50, classes) != sc.brute_extract(data, per, 25, 50)
    # the same FASTA as BGZF input gives the same bytes
    bg = tmp_path / "in.fa.gz"
    bg.write_bytes(gz.bgzf_compress(data))
    tsv_bg, files = run(bg, "d")
    assert list(files) == ["in.fa.gz.repeats.fa"] and files["in.fa.gz.repeats.fa"] == sc.brute_extract(data, _tsv_rows(tsv_bg, data)) == want
    # a .2bit file gives what its FASTA text gives (soft-masked bases lower case)
    recs = tc.cli_file()
    (tmp_path / "corpus.2bit").write_bytes(tc.write(recs))
    (tmp_path / "corpus.fa").write_bytes(tc.text(recs))
    _t, from_tb = run(tmp_path / "corpus.2bit", "e", "--seq_flank", "3")
    _t, from_fa = run(tmp_path / "corpus.fa", "f", "--seq_flank", "3")
    assert from_tb["corpus.2bit.repeats.fa"] == from_fa["corpus.fa.repeats.fa"]
    assert from_fa["corpus.fa.repeats.fa"].count(b" core=") > 3
    # an all-N record stops predict: no file, no staged file
    bad = tmp_path / "bad.fa"
    bad.write_bytes(data + b"\n>allN\nNNNNNNNNNN\n")
    with pytest.raises(ValueError, match="negative dimensions"):
        run(bad, "g")
    assert os.listdir(tmp_path / "g") == []
