"""The host side of `predict --seq_dir`: the exported entry and its checks before any device work, the numpy mirror `extract_host`
and `text_bound` against tests/seq_extract_cases.py (an independent statement of the format), the `.fai` statement, and the
command-line refusals.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import seq_extract_cases as sc
from conftest import GOLDEN, ROOT

NAMES = ("dgrp_fasta_extract_workspace_bytes", "dgrp_fasta_extract_batch")
SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])
MODEL = os.path.join(GOLDEN, "model_u8_T20.h5")


def test_symbols_declared_exported_and_bound():
    from deepgrp_amd import _lib, repeatseq
    header = open(os.path.join(ROOT, "include", "deepgrp_hip.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert f" {name}(" in header and name in _lib.exported_symbols() and hasattr(L, name), name
    assert "typedef struct dgrp_extract_entry" in header
    assert repeatseq.ENTRY_DTYPE.itemsize == 24 and repeatseq.SEQ_PIECE == 256 << 20
    assert callable(repeatseq.write_repeat_fasta) and callable(repeatseq.extract_host) and callable(repeatseq.text_bound)
    make = open(os.path.join(ROOT, "deepgrp_amd", "csrc", "Makefile")).read()
    assert "extract_kernels.o: extract_kernels.hip body_tiles.h scan.h" in make


def test_the_workspace_query_is_total_and_monotone():
    from deepgrp_amd import _lib
    q = _lib.lib().dgrp_fasta_extract_workspace_bytes
    assert q(-1, 10, 10) == 0 and q(3, -1, 10) == 0 and q(3, 10, -1) == 0
    assert q(0, 0, 0) >= 0
    base = (7, 100_000, 500)
    for i in range(3):
        prev = q(*base)
        for step in (1, 10, 4096, 1 << 20):
            arg = list(base)
            arg[i] += step
            assert q(*arg) >= prev, (i, step)
            prev = q(*arg)
    # a counter per tile of 4 096 bytes, a size per row and five table entries per record at the least
    assert q(4096, 256 << 20, 100_000) >= 8 * ((256 << 20) // sc.TILE) + 8 * 100_000 + 5 * 8 * 4096


def _call(L, off=(0, 100), ln=(100, 50), row_off=(0, 1, 2), name_off=(0, 2, 4), flank=0, width=60, work=None, nrec=2, d_raw=None,
          d_ptr=None, sizes=True):
    i64 = lambda v: np.array(v, np.int64)
    a = [i64(off), i64(ln), i64(row_off), i64(name_off)]
    need = L.dgrp_fasta_extract_workspace_bytes(2, 150, 2)
    size, kept = C.c_int64(-7), C.c_int64(-7)
    rc = L.dgrp_fasta_extract_batch(d_raw, nrec, a[0].ctypes.data, a[1].ctypes.data, d_ptr, a[2].ctypes.data, d_ptr, a[3].ctypes.data, flank,
                                    width, 2, d_ptr, 1 << 20, C.byref(size) if sizes else None, None, C.byref(kept) if sizes else None, d_ptr,
                                    need if work is None else work, None)
    return rc, L.dgrp_last_error().decode(), size.value, kept.value


def test_the_entry_checks_everything_before_any_device_work():
    """Bad host tables and scalars (DGRP_EINVAL), then a short workspace (DGRP_ENOMEM), then the pointers themselves: every refusal
    carries a message, and the device pointers -- NULL or made up -- are never touched.  nrec == 0 and no rows are nothing to do."""
    from deepgrp_amd import _lib
    L = _lib.lib()
    need = L.dgrp_fasta_extract_workspace_bytes(2, 150, 2)
    fake = 0x10000                                      # 256-byte aligned, not mapped: touching it would crash
    for kw, rc_want, word in ((dict(off=(-1, 100)), -1, "negative range (record 0)"), (dict(ln=(100, -5)), -1, "negative range (record 1)"),
                              (dict(off=(200, 100)), -1, "must ascend and not overlap (record 1)"),
                              (dict(off=(0, 99)), -1, "must ascend and not overlap (record 1)"),
                              (dict(row_off=(0, 2, 1)), -1, "row offsets must ascend (record 1)"),
                              (dict(row_off=(-1, 0, 1)), -1, "negative row offset"),
                              (dict(name_off=(0, 3, 2)), -1, "name offsets must ascend"),
                              (dict(name_off=(-2, 0, 2)), -1, "negative name offset"),
                              (dict(width=0), -1, "width"), (dict(width=-3), -1, "width"), (dict(width=(1 << 30) + 1), -1, "width"),
                              (dict(flank=-1), -1, "negative flank"), (dict(nrec=-1), -1, "bad arguments"),
                              (dict(sizes=False), -1, "h_text_bytes"),
                              (dict(work=need - 1), -3, "workspace"), (dict(work=0), -3, "workspace"),
                              (dict(work=need - 1, d_raw=fake + 1), -3, "workspace"),
                              (dict(), -1, "NULL device pointer"),
                              (dict(d_raw=fake + 1, d_ptr=fake), -1, "16-byte aligned")):
        rc, msg, _size, _kept = _call(L, **kw)
        assert rc == rc_want and word in msg, (kw, rc, msg)
    # nothing to do: no record, or no row at all -- the sizes are 0 and no pointer is needed
    size, kept = C.c_int64(-7), C.c_int64(-7)
    assert L.dgrp_fasta_extract_batch(None, 0, None, None, None, None, None, None, 0, 60, 2, None, 0, C.byref(size), None, C.byref(kept),
                                      None, 0, None) == 0
    assert (size.value, kept.value) == (0, 0)
    rc, _msg, size, kept = _call(L, row_off=(5, 5, 5), work=0)
    assert (rc, size, kept) == (0, 0, 0)


# ---------------------------------------------------------------- extract_host and text_bound
def _host_text(data: bytes, per, flank, width, classes):
    """extract_host over masking.sequence_byte_offsets, record by record, as write_repeat_fasta's host path does."""
    from deepgrp_amd import masking, repeatseq, twobit
    bits = masking.class_bits(classes)
    out, entries = [], []
    buf = np.frombuffer(data, np.uint8)
    for k, (header, offs) in enumerate(masking.sequence_byte_offsets(data)):
        if offs is None:
            continue
        rows = np.array([(s, e, lab, k) for s, e, lab in sorted(per[k])], SEG)
        text, ent = repeatseq.extract_host(buf, offs, twobit.record_name(header), rows, bits, flank, width)
        entries += [(t + sum(len(x) for x in out), b + sum(len(x) for x in out), n) for t, b, n in ent.tolist()]
        out.append(text)
    return b"".join(out), entries


@pytest.mark.parametrize("flank", sc.FLANKS)
@pytest.mark.parametrize("width", sc.WIDTHS)
def test_extract_host_equals_the_statement_on_odd_records(flank, width):
    data = sc.odd_records_file()
    names = [n for n, _p in sc.brute_records(data)]
    assert names == [b"plain", b"crlf", b"padded", b"second", b"nonascii", b"lone", b"empty", b"last"]
    per = sc.rows_for(data)
    for classes in (None, sc.CLASSES):
        want = sc.brute_extract(data, per, flank, width, classes)
        got, entries = _host_text(data, per, flank, width, classes)
        assert got == want
        assert entries == sc.brute_entries(want)
    assert want.count(b">") > 20


def test_extract_host_on_a_headerless_chunk_and_an_empty_name():
    from deepgrp_amd import masking, repeatseq
    assert masking.sequence_byte_offsets(sc.headerless_chunk()) == [] and sc.brute_records(sc.headerless_chunk()) == []
    assert sc.brute_extract(sc.headerless_chunk(), [[(0, 2, 1)]]) == b""
    buf = np.frombuffer(b"xxACGTNNacgt", np.uint8)
    offs = np.arange(2, 12, dtype=np.int64)
    rows = np.array([(0, 4, 1, 0), (5, 7, 2, 0), (8, 10, 3, 0)], SEG)
    text, ent = repeatseq.extract_host(buf, offs, b"", rows, masking.class_bits(None), 1, 3)
    assert text == b">:0-5 class1 core=0-4\nACG\nTN\n>:4-8 class2 core=5-7\nNNa\nc\n>:7-10 class3 core=8-10\ncgt\n"
    assert ent.tolist() == [(0, 22, 5), (29, 51, 4), (57, 81, 3)]
    assert text == sc.row_text(b"", b"ACGTNNacgt", 0, 4, 1, 1, 3) + sc.row_text(b"", b"ACGTNNacgt", 5, 7, 2, 1, 3) + \
        sc.row_text(b"", b"ACGTNNacgt", 8, 10, 3, 1, 3)
    for bad in ([(0, 11, 1, 0)], [(3, 3, 1, 0)], [(4, 6, 1, 0), (5, 7, 1, 0)], [(-1, 2, 1, 0)]):
        with pytest.raises(ValueError, match="empty, out of order or beyond"):
            repeatseq.extract_host(buf, offs, b"n", np.array(bad, SEG), 2, 0, 60)


def test_text_bound_is_a_bound_and_exact_without_flank():
    from deepgrp_amd import repeatseq
    data = sc.odd_records_file()
    per = sc.rows_for(data)
    cases = [(data, per, sc.sequences(data))]
    buf, offs, lens, names, rowsets = sc.kernel_case()
    for k in range(len(offs)):
        text = b">" + (names[k] or b"n") + b"\n" + buf[offs[k]:offs[k] + lens[k]]
        cases.append((text, [rowsets[k]], sc.sequences(text)))
    for flank in sc.FLANKS:
        for width in sc.WIDTHS:
            for text, rowsets_, seqs in cases:
                for k, (name, seq) in enumerate(seqs):
                    if seq is None or not rowsets_[k]:
                        continue
                    rows = np.array([(s, e, lab, k) for s, e, lab in rowsets_[k] if lab > 0], SEG)
                    exact = len(sc.brute_extract(text, [[]] * k + [rowsets_[k]], flank, width, None, seqs=seqs))
                    bound = repeatseq.text_bound(rows, len(name), flank, width)
                    assert bound >= exact, (flank, width, name)
                    if flank == 0:
                        assert bound == exact, (width, name)
    assert repeatseq.text_bound(np.zeros(0, SEG), 3, 5, 60) == 0


def test_brute_fai_of_a_hand_written_text():
    text = b">chr1:0-7 class1\nACG\nTAC\nG\n>chr1:10-12 class3 core=11-12\nNN\n>x:5-11 class2\nAAA\nCCC\n"
    assert sc.brute_fai(text) == b"chr1:0-7\t7\t17\t3\t4\nchr1:10-12\t2\t57\t2\t3\nx:5-11\t6\t75\t3\t4\n"
    assert sc.brute_entries(text) == [(0, 17, 7), (27, 57, 2), (60, 75, 6)]
    for line in sc.brute_fai(text).split(b"\n")[:-1]:
        name, bases, off, w, _w1 = line.split(b"\t")
        assert text[int(off):int(off) + int(w)].isalpha() and text[int(off) - 1:int(off)] == b"\n"


def test_fai_lines_state_what_brute_fai_reads():
    from deepgrp_amd import masking, repeatseq
    seq = b"ACGTNNacgtACGTACGTAC"
    rows = np.array([(2, 9, 1, 0), (12, 13, 3, 0), (15, 20, 2, 0)], SEG)
    for flank, width in ((0, 3), (4, 60), (100, 5)):
        text, ent = repeatseq.extract_host(np.frombuffer(seq, np.uint8), np.arange(len(seq)), b"chrZ", rows, masking.class_bits(None), flank, width)
        got = repeatseq.fai_lines(b"chrZ", rows["start"], ent, flank, width, 1000)
        want = []
        for line, (_t, base_off, _n) in zip(sc.brute_fai(text).split(b"\n")[:-1], ent.tolist()):
            cols = line.split(b"\t")
            cols[2] = b"%d" % (int(cols[2]) + 1000)
            want.append(b"\t".join(cols) + b"\n")
        assert got == b"".join(want)


# ---------------------------------------------------------------- the command line
REFUSALS = [
    # (arguments, environment, words of the message)
    (["predict", "MODEL", "FA", "--seq_gzip"], {}, ["need --seq_dir"]),
    (["predict", "MODEL", "FA", "--seq_fai"], {}, ["need --seq_dir"]),
    (["predict", "MODEL", "FA", "--seq_classes", "1"], {}, ["need --seq_dir"]),
    (["predict", "MODEL", "FA", "--seq_flank", "10"], {}, ["need --seq_dir"]),
    (["--seq_width", "70", "MODEL", "FA"], {}, ["need --seq_dir"]),                                   # the README form
    (["predict", "MODEL", "FA", "--seq_dir", "OUT", "--seq_fai", "--seq_gzip"], {}, ["--seq_fai and --seq_gzip exclude", ".gzi"]),
    (["predict", "MODEL", "-", "--seq_dir", "OUT"], {}, ["--seq_dir: standard input"]),
    (["predict", "MODEL", "x.gz.npz", "--seq_dir", "OUT"], {}, ["--seq_dir: x.gz.npz is a one-hot .npz"]),
    (["predict", "MODEL", "FA", "--seq_dir", "OUT"], {"WORLD_SIZE": "2", "RANK": "0"}, ["--seq_dir", "WORLD_SIZE > 1", "--split_contigs"]),
    (["predict", "MODEL", "FA", "--seq_dir", "OUT", "--split_contigs"], {}, ["--seq_dir", "WORLD_SIZE > 1", "--split_contigs"]),
    (["predict", "MODEL", "FA", "--seq_dir", "OUT", "--seq_width", "0"], {}, ["--seq_width must lie in 1..2^30"]),
    (["predict", "MODEL", "FA", "--seq_dir", "OUT", "--seq_width", str((1 << 30) + 1)], {}, ["--seq_width must lie in 1..2^30"]),
    (["predict", "MODEL", "FA", "--seq_dir", "OUT", "--seq_flank", "-1"], {}, ["--seq_flank must not be negative"]),
    (["predict", "MODEL", "FA", "--seq_dir", "OUT", "--seq_gzip", "--gzip_level", "2"], {}, ["--gzip_level must be 0"]),
    (["predict", "MODEL", "FA", "OTHER/in.fa", "--seq_dir", "OUT"], {}, ["--seq_dir", "in.fa.repeats.fa", "collide"]),
    (["predict", "MODEL", "FA", "SELF", "--seq_dir", "HERE"], {}, ["--seq_dir", "would overwrite the input"]),
    (["--seq_dir", "OUT", "evaluate", "MODEL", "FA", "FA"], {}, ["--seq_dir belongs to predict, not evaluate"]),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_every_refusal_comes_before_the_model_is_read(tmp_path, monkeypatch, k):
    """Each refused command line exits non-zero with its words, with the model reader and the model loader patched to fail: the
    refusal never gets past the flags.  Nothing appears in the output directory."""
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.__main__ import main
    argv, env, words = REFUSALS[k]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    monkeypatch.setattr(dgmodel, "read_keras_hdf5", lambda *a, **kw: pytest.fail("went past the refusal: the model was read"))
    monkeypatch.setattr(dgmodel, "load_model", lambda *a, **kw: pytest.fail("went past the refusal: the model was loaded"))
    monkeypatch.setattr(dgmodel, "device_model", lambda *a, **kw: pytest.fail("went past the refusal: the model was loaded"))
    fa = tmp_path / "in.fa"
    fa.write_bytes(b">x\nACGT\n")
    (tmp_path / "other").mkdir()
    (tmp_path / "other" / "in.fa").write_bytes(b">y\nAC\n")
    (tmp_path / "in.fa.repeats.fa").write_bytes(b">z\nAC\n")
    sub = {"MODEL": MODEL, "FA": str(fa), "OUT": str(tmp_path / "seqs"), "OTHER/in.fa": str(tmp_path / "other" / "in.fa"),
           "SELF": str(tmp_path / "in.fa.repeats.fa"), "HERE": str(tmp_path)}
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit) as e:
        main([sub.get(a, a) for a in argv] + ["--output", str(tmp_path / "o.tsv")] if "evaluate" not in argv else [sub.get(a, a) for a in argv])
    assert e.value.code not in (0, None)
    assert all(w in str(e.value.code) for w in words), e.value.code
    assert sorted(os.listdir(tmp_path)) == before                     # no TSV, no output directory, nothing staged


def test_a_label_outside_the_model_is_refused_once_the_class_count_is_known(tmp_path, monkeypatch):
    """--seq_classes is checked against the class count read from the HDF5 file on the host, before the model is loaded."""
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.__main__ import main
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(dgmodel, "load_model", lambda *a, **kw: pytest.fail("went past the refusal: the model was loaded"))
    monkeypatch.setattr(dgmodel, "device_model", lambda *a, **kw: pytest.fail("went past the refusal: the model was loaded"))
    fa = tmp_path / "in.fa"
    fa.write_bytes(b">x\nACGT\n")
    for labels in ("0", "5", "1,2,9"):
        with pytest.raises(SystemExit) as e:
            main(["predict", MODEL, str(fa), "--seq_dir", str(tmp_path / "seqs"), "--seq_classes", labels, "--output", str(tmp_path / "o.tsv")])
        assert "--seq_classes" in str(e.value.code) and "not a repeat class" in str(e.value.code) and "1..4" in str(e.value.code)
    assert os.listdir(tmp_path / "seqs") == [] and not (tmp_path / "o.tsv").exists()


def test_the_plan_names_the_files(tmp_path, monkeypatch):
    import argparse

    from deepgrp_amd import repeatseq
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    fa, gz = tmp_path / "chr.fa", tmp_path / "hg38.fa.gz"
    fa.write_bytes(b">x\nACGT\n")
    gz.write_bytes(b"\x1f\x8b")
    out = str(tmp_path / "seqs")
    args = argparse.Namespace(seq_dir=out, FASTA=[str(fa), str(gz)])
    plan = repeatseq.plan(args)
    assert plan._asdict() == dict(files={str(fa): os.path.join(out, "chr.fa.repeats.fa"), str(gz): os.path.join(out, "hg38.fa.gz.repeats.fa")},
                        classes=None, flank=0, width=60, gzip=False, fai=False, level=1)
    args = argparse.Namespace(seq_dir=out, FASTA=[str(fa)], seq_gzip=True, seq_flank=7, seq_width=80, seq_classes=(1, 3), gzip_level=0)
    plan = repeatseq.plan(args)
    assert plan._asdict() == dict(files={str(fa): os.path.join(out, "chr.fa.repeats.fa.gz")}, classes=(1, 3), flank=7, width=80, gzip=True, fai=False,
                        level=0)
    assert repeatseq.plan(argparse.Namespace(FASTA=[str(fa)])) is None
