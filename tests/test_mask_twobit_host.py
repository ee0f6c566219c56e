"""The host side of `predict --mask_twobit`: the exported entry and its checks before any device work, the numpy packer and the
file writer against tests/mask_twobit_cases.py (an independent statement of the format), the parser on the written files, the
command-line refusals, the name plan and the warning-and-no-file path.  No GPU."""
import argparse
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

import mask_twobit_cases as mc
import twobit_corpus as tc
from conftest import GOLDEN, ROOT

NAMES = ("dgrp_twobit_pack_workspace_bytes", "dgrp_twobit_pack_batch")


def test_symbols_exported_and_bound():
    from deepgrp_amd import _lib, twobit
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.exported_symbols() and hasattr(L, name), name
    assert callable(twobit.pack_record) and callable(twobit.write_file) and issubclass(twobit.Refused, ValueError)


def test_the_workspace_query_is_total():
    from deepgrp_amd import _lib
    L = _lib.lib()
    assert L.dgrp_twobit_pack_workspace_bytes(-1, 10) == 0 and L.dgrp_twobit_pack_workspace_bytes(3, -1) == 0
    assert L.dgrp_twobit_pack_workspace_bytes(0, 0) >= 0
    small, large = L.dgrp_twobit_pack_workspace_bytes(1, 100), L.dgrp_twobit_pack_workspace_bytes(4096, 256 << 20)
    # two counters per tile of 4 096 bytes and four table entries per record at the least
    assert small > 0 and large >= 2 * 8 * ((256 << 20) // mc.TILE) + 4 * 8 * 4096 and large > small


def test_the_entry_checks_everything_before_any_device_work():
    """Bad host tables (DGRP_EINVAL), a short workspace and an output without room for the records' fixed words (DGRP_ENOMEM) are
    refused with a message and with no device pointer ever touched; nrec == 0 is nothing to do."""
    from deepgrp_amd import _lib
    L = _lib.lib()
    i64 = lambda *v: np.array(v, np.int64)
    assert L.dgrp_twobit_pack_batch(None, 0, None, None, None, 0, 0, None, None, None, 0, None) == 0
    need = L.dgrp_twobit_pack_workspace_bytes(2, 150)

    def call(off=(0, 100), ln=(100, 50), out_off=0, cap=1 << 20, work=need, tables=True, nrec=2):
        a = [i64(*off), i64(*ln), np.zeros(3 * 2, np.int64), np.zeros(3, np.int64)]
        rc = L.dgrp_twobit_pack_batch(None, nrec, a[0].ctypes.data, a[1].ctypes.data, None, out_off, cap, a[2].ctypes.data if tables else None,
                                      a[3].ctypes.data, None, work, None)
        return rc, L.dgrp_last_error().decode()

    for kw, rc_want, word in ((dict(off=(-1, 100)), -1, "negative range (record 0)"), (dict(ln=(100, -5)), -1, "negative range (record 1)"),
                              (dict(ln=(1 << 31, 1 << 31)), -1, "2^32 - 1 bytes"), (dict(nrec=-1), -1, "negative size"),
                              (dict(out_off=-1), -1, "negative size"), (dict(tables=False), -1, "NULL host table"),
                              (dict(work=need - 1), -3, "workspace"), (dict(work=0), -3, "workspace"),
                              (dict(cap=31), -3, "do not fit the output buffer"), (dict(out_off=10, cap=41), -3, "do not fit the output buffer"),
                              (dict(out_off=50, cap=40), -3, "do not fit the output buffer"), (dict(), -1, "NULL device pointer")):
        rc, msg = call(**kw)
        assert rc == rc_want and word in msg, (kw, rc, msg)


CASES = mc.body_cases()


@pytest.mark.parametrize("label", [label for label, _body in CASES])
def test_pack_record_matches_the_statement(label):
    from deepgrp_amd import twobit
    seq = mc.sequence(dict(CASES)[label])
    got = twobit.pack_record(seq)
    assert got == mc.blob(seq)
    assert twobit.pack_record(np.frombuffer(seq, np.uint8)) == got
    n, nb, mb = mc.counts(seq)
    assert len(got) == 16 + 8 * (nb + mb) + (n + 3) // 4


TEXTS = mc.masked_texts()


@pytest.mark.parametrize("label", sorted(TEXTS))
def test_write_file_and_the_parser_close_the_loop(tmp_path, label):
    """write_file over pack_record's blobs is the statement's file byte for byte -- as a list of blobs and as a spool cut anywhere
    -- and open_twobit reads the names, sizes and intervals back."""
    from deepgrp_amd import twobit
    text = TEXTS[label]
    recs = mc.records(text)
    names, blobs = [n for n, _s in recs], [twobit.pack_record(s) for _n, s in recs]
    want = mc.file_of(text)
    out = tmp_path / "x.2bit"
    assert twobit.write_file(names, blobs, out) == len(want)
    assert out.read_bytes() == want
    spool = b"".join(blobs)
    pieces = [spool[o:o + 7] for o in range(0, len(spool), 7)]
    assert twobit.write_file(names, iter(pieces), out, sizes=[len(b) for b in blobs]) == len(want)
    assert out.read_bytes() == want
    tb = twobit.open_twobit(out)
    assert tb.byteorder == "<" and tb.names == names and tb.dna_size.tolist() == [len(s) for _n, s in recs]
    for i, (name, seq) in enumerate(recs):
        r = mc.rec(name, seq)
        assert tb.n_iv[tb.n_off[i]:tb.n_off[i + 1]].tolist() == [[s, s + z] for s, z in r.nblocks], name
        assert tb.m_iv[tb.m_off[i]:tb.m_off[i + 1]].tolist() == [[s, s + z] for s, z in r.mblocks], name
    assert tb.text_size == len(mc.normalised(text))


def test_the_statement_reads_its_own_records():
    assert mc.records(b"x\n>a b\r\nAC\r\ngt\r\n>\nTT\n> c \nN") == [(b"a", b"ACgt"), (b"c", b"N")]
    assert mc.normalised(b">a b\nACRr\n") == b">a\nACNn\n"
    assert mc.counts(b"NNacgtnnACGTn") == [13, 3, 2]


def test_write_file_refuses_what_the_format_cannot_hold(tmp_path):
    from deepgrp_amd import twobit
    out = tmp_path / "r.2bit"
    blob = twobit.pack_record(b"ACGT")
    with pytest.raises(twobit.Refused, match="both named b'chr1'"):
        twobit.write_file([b"chr1", b"chr2", b"chr1"], [blob] * 3, out, what="in.fa")
    with pytest.raises(twobit.Refused, match=r"in.fa: record 1 .*256 bytes"):
        twobit.write_file([b"ok", b"y" * 256], [blob] * 2, out, what="in.fa")
    with pytest.raises(twobit.Refused, match=r"record 2 \(b'c'\): the file reaches 2\^32 bytes"):
        twobit.write_file([b"a", b"b", b"c"], iter(()), out, sizes=[1 << 31, (1 << 31) - 100, 100], what="in.fa")
    assert not out.exists()
    twobit.write_file([b"y" * 255], [blob], out)                       # 255 bytes is a name
    assert twobit.open_twobit(out).names == [b"y" * 255]


def _plan(tmp_path, files, **kw):
    from deepgrp_amd import masking
    args = argparse.Namespace(mask_dir=str(tmp_path / "masked"), mask=None, mask_classes=None, mask_gzip=False, mask_twobit=True,
                              FASTA=[str(f) for f in files])
    for k, v in kw.items():
        setattr(args, k, v)
    return masking.plan(args).files


def test_the_name_plan(tmp_path, monkeypatch):
    import gzip
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    (tmp_path / "a").mkdir()
    fa, gz, tb, sly, notgz = tmp_path / "chr.fa", tmp_path / "hg38.fa.gz", tmp_path / "hg38.2bit", tmp_path / "sly.fa", tmp_path / "odd.gz"
    fa.write_bytes(b">x\nACGT\n")
    gz.write_bytes(gzip.compress(b">x\nACGT\n"))
    rng = np.random.default_rng(3)
    tb.write_bytes(tc.write([tc._rec(rng, b"one", 40)]))
    sly.write_bytes(tc.write([tc._rec(rng, b"one", 40)], ">"))          # a 2bit file whatever its name
    notgz.write_bytes(b">x\nAC\n")                                      # named .gz, not compressed: the name stays
    out = str(tmp_path / "masked")
    join = lambda n: os.path.join(out, n)
    assert _plan(tmp_path, [fa, gz, tb, sly, notgz]) == {str(fa): join("chr.fa.2bit"), str(gz): join("hg38.fa.2bit"), str(tb): join("hg38.2bit"),
                                                         str(sly): join("sly.fa.2bit"), str(notgz): join("odd.gz.2bit")}
    # without the flag nothing changes
    assert _plan(tmp_path, [fa, tb], mask_twobit=False) == {str(fa): join("chr.fa"), str(tb): join("hg38.2bit.fa")}
    # the collision check runs on the new names ...
    plain = tmp_path / "hg38.fa"
    plain.write_bytes(b">y\nAC\n")
    with pytest.raises(SystemExit) as e:
        _plan(tmp_path, [gz, plain])
    assert "collide" in str(e.value) and "hg38.fa.2bit" in str(e.value)
    other = tmp_path / "a" / "hg38.2bit"
    other.write_bytes(tb.read_bytes())
    with pytest.raises(SystemExit) as e:
        _plan(tmp_path, [tb, other])
    assert "collide" in str(e.value)
    # ... and so does the overwrite check: a 2bit input masked into its own directory would land on itself
    with pytest.raises(SystemExit) as e:
        _plan(tmp_path, [tb], mask_dir=str(tmp_path))
    assert "overwrite" in str(e.value) and str(tb) in str(e.value)
    assert _plan(tmp_path, [fa], mask_dir=str(tmp_path)) == {str(fa): str(tmp_path / "chr.fa.2bit")}
    # bare namespaces (no mask_twobit attribute) plan as before
    from deepgrp_amd import masking
    bare = argparse.Namespace(mask_dir=out, mask=None, mask_classes=None, mask_gzip=False, FASTA=[str(fa)])
    assert masking.plan(bare).files == {str(fa): join("chr.fa")}


REFUSALS = [
    # (arguments behind the model, environment, words of the message)
    (["predict", "MODEL", "FA", "--mask_twobit"], {}, ["--mask_twobit needs --mask_dir"]),
    (["--mask_twobit", "MODEL", "FA"], {}, ["--mask_twobit needs --mask_dir"]),                         # the README form
    (["predict", "MODEL", "FA", "--mask_dir", "OUT", "--mask_twobit", "--mask_gzip"], {}, ["--mask_twobit and --mask_gzip exclude"]),
    (["predict", "MODEL", "FA", "--mask_dir", "OUT", "--mask_twobit"], {"WORLD_SIZE": "2", "RANK": "0"},
     ["--mask_twobit", "WORLD_SIZE > 1", "--split_contigs", "byte ranges"]),
    (["predict", "MODEL", "FA", "--mask_dir", "OUT", "--mask_twobit", "--split_contigs"], {},
     ["--mask_twobit", "WORLD_SIZE > 1", "--split_contigs", "byte ranges"]),
    (["--mask_twobit", "evaluate", "MODEL", "FA", "FA"], {}, ["--mask_twobit belongs to predict, not evaluate"]),
    (["predict", "MODEL", "-", "--mask_dir", "OUT", "--mask_twobit"], {}, ["--mask_dir: standard input cannot be masked"]),
    (["predict", "MODEL", "x.gz.npz", "--mask_dir", "OUT", "--mask_twobit"], {}, ["--mask_dir: x.gz.npz is a one-hot .npz"]),
    # the existing messages stay word for word
    (["predict", "MODEL", "FA", "--mask_gzip"], {}, ["--mask, --mask_classes and --mask_gzip need --mask_dir"]),
]


def test_every_refusal_comes_before_anything_is_loaded(tmp_path):
    """One child process runs every refused command line: each exits with its message, and neither torch nor the library was
    loaded by then."""
    fa = tmp_path / "in.fa"
    fa.write_bytes(b">x\nACGT\n")
    sub = {"MODEL": os.path.join(GOLDEN, "model_u8_T20.h5"), "FA": str(fa), "OUT": str(tmp_path / "masked")}
    runs = [([sub.get(a, a) for a in argv] + ([] if "evaluate" in argv else ["--output", str(tmp_path / "o.tsv")]), env)
            for argv, env, _words in REFUSALS]
    (tmp_path / "runs.json").write_text(json.dumps(runs))
    code = ("import json, os, sys\n"
            "from deepgrp_amd.__main__ import main\n"
            "import deepgrp_amd._lib as l\n"
            "base = dict(os.environ)\n"
            "for argv, env in json.load(open(sys.argv[1])):\n"
            "    os.environ.clear(); os.environ.update(base); os.environ.update(env)\n"
            "    try:\n"
            "        main(argv)\n"
            "        msg = 'RAN'\n"
            "    except SystemExit as e:\n"
            "        msg = str(e.code)\n"
            "    print(json.dumps([msg, l._lib is not None or 'torch' in sys.modules]))\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "runs.json")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(got) == len(REFUSALS)
    for (argv, _env, words), (msg, loaded) in zip(REFUSALS, got):
        assert all(w in msg for w in words), (argv, msg)
        assert not loaded, argv
    assert not (tmp_path / "o.tsv").exists() and not (tmp_path / "masked").exists()


@pytest.mark.parametrize("names, word", [([b"chr1 a", b"chr1 b"], "both named b'chr1'"), ([b"z" * 256], "256 bytes")])
def test_a_refused_input_gets_one_warning_and_no_file(tmp_path, monkeypatch, caplog, names, word):
    """masking.write_mask on a writer that stands in for the device work: it spools as mask_fasta does and ends in twobit.write_file.
    Duplicate first words and a 256-byte name: one warning that names the input and the record, no .2bit, no staged file left, and
    the command goes on (no exception)."""
    from deepgrp_amd import masking, twobit
    calls = []

    def fake(fasta_path, out_path, rows, mode="soft", classes=None, **kw):
        calls.append(kw)
        assert os.path.exists(out_path)                                  # the staged file of write_mask
        cut = [twobit.record_name(n.decode()) for n in names]
        twobit.write_file(cut, [twobit.pack_record(b"ACGTnn")] * len(cut), out_path, what=str(fasta_path))

    monkeypatch.setattr(masking, "mask_fasta", fake)
    final = tmp_path / "masked" / "in.fa.2bit"
    final.parent.mkdir()
    plan = masking.MaskPlan({}, "hard", None, twobit=True)
    with caplog.at_level(logging.WARNING, logger="deepgrp_amd.__main__"):
        masking.write_mask("in.fa", str(final), np.zeros(0), plan, logging.getLogger("deepgrp_amd.__main__"))
    assert calls == [dict(twobit=True)]
    assert os.listdir(final.parent) == []
    warnings = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "in.fa" in warnings[0] and word in warnings[0] and str(final) in warnings[0]
    # the same writer with names the format holds leaves the file
    names[:] = [b"chr1 a", b"chr2 b"]
    masking.write_mask("in.fa", str(final), np.zeros(0), plan)
    assert twobit.open_twobit(final).names == [b"chr1", b"chr2"]
