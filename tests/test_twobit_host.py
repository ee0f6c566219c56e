"""The host side of the 2bit input (deepgrp_amd/twobit.py): the parser against the corpus's own statement of the format in both byte
orders, every refusal with the field it names, the signature test, the exported symbols, the names of the masked copies and the
refusal of a sharded run.  No GPU."""
import argparse
import gzip
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import twobit_corpus as tc
from conftest import GOLDEN, ROOT

FILES = {"sizes": tc.sizes_file, "blocks": tc.blocks_file, "odd": tc.odd_file, "batch": lambda: tc.batch_file(300)}


@pytest.mark.parametrize("order", ["<", ">"])
@pytest.mark.parametrize("which", sorted(FILES))
def test_parser_returns_the_corpus(tmp_path, which, order):
    from deepgrp_amd import twobit
    recs = FILES[which]()
    path = tmp_path / "x.2bit"
    path.write_bytes(tc.write(recs, order))
    assert twobit.is_twobit(path)
    tb = twobit.open_twobit(path)
    assert tb.byteorder == order and tb.nrec == len(recs) and tb.size == path.stat().st_size
    assert tb.names == [r.name for r in recs]
    assert tb.dna_size.tolist() == [len(r.codes) for r in recs]
    raw = path.read_bytes()
    for i, r in enumerate(recs):
        assert raw[tb.name_off[i]:tb.name_off[i] + tb.name_len[i]] == r.name
        assert raw[tb.packed_off[i]:tb.packed_off[i] + (len(r.codes) + 3) // 4] == tc.pack_dna(r.codes, r.pad)
        n_iv = tb.n_iv[tb.n_off[i]:tb.n_off[i + 1]]
        m_iv = tb.m_iv[tb.m_off[i]:tb.m_off[i + 1]]
        assert n_iv.dtype == np.int64 and m_iv.dtype == np.int64
        assert np.array_equal(n_iv, tc.intervals(len(r.codes), r.nblocks)), r.name
        assert np.array_equal(m_iv, tc.intervals(len(r.codes), r.mblocks)), r.name
        assert (int(tb.startpos[i]), int(tb.kept[i])) == tc.strip_n(tc.indices(r)), r.name
    assert tb.text_size == len(tc.text(recs))
    assert all(a.dtype == np.int64 for a in (tb.name_off, tb.rec_off, tb.packed_off, tb.dna_size, tb.text_off, tb.startpos, tb.kept))


def test_the_corpus_reaches_every_alignment(tmp_path):
    """packedDna of the corpus starts at every address mod 16 (names of 0..17 bytes, tables of every length)."""
    from deepgrp_amd import twobit
    seen = set()
    for which in ("sizes", "blocks", "batch"):
        path = tmp_path / f"{which}.2bit"
        path.write_bytes(tc.write(FILES[which]()))
        seen |= set((twobit.open_twobit(path).packed_off % 16).tolist())
    assert seen == set(range(16))
    assert sorted({len(r.name) for r in tc.sizes_file()}) == list(range(18))


def test_placed_offsets_align_the_packed_loads():
    """twobit.placed_offsets, for packed bytes and an index buffer at every address mod 16: records do not overlap, fit the buffer
    the docstring sizes, start a multiple of 4 bytes into a 16-byte word, and the second and every later word of a record begins
    with the first base of a packed byte whose address is a multiple of 4 (the condition, worked out here from the word, not from
    the formula)."""
    from deepgrp_amd import twobit
    rng = np.random.default_rng(tc.SEED + 11)
    dna = rng.integers(0, 200, 64).astype(np.int64)
    for idx_addr in range(0x7000_0000_1000, 0x7000_0000_1010):
        packed_addr = (0x7100_0000_0000 + np.arange(64) * 1000 + rng.integers(0, 16, 64)).astype(np.int64)
        assert set((packed_addr % 4).tolist()) == {0, 1, 2, 3}
        off = twobit.placed_offsets(packed_addr, dna, idx_addr)
        assert off.dtype == np.int64 and off[0] >= 0 and (off[1:] >= off[:-1] + dna[:-1]).all()
        assert off[-1] + dna[-1] <= dna.sum() + 32 * dna.size + 16
        for r in range(dna.size):
            o = (idx_addr + int(off[r])) % 16
            assert o % 4 == 0
            for g in (1, 2, 7):
                base = 16 * g - o                                      # first base of word g of the record
                assert base % 4 == 0 and (int(packed_addr[r]) + base // 4) % 4 == 0, (idx_addr % 16, int(packed_addr[r]) % 4, o)


def _small():
    rng = np.random.default_rng(5)
    return [tc._rec(rng, b"one", 40, [(2, 3), (9, 4)], [(1, 5)]), tc._rec(rng, b"two", 21, [(0, 2)], [(4, 4), (10, 2)])]


def _layout(recs):
    """File offsets of the second record's fields."""
    rec2 = 16 + sum(1 + len(r.name) + 4 for r in recs) + 4 + (4 + 8 * 2) + (4 + 8 * 1) + 4 + 10
    nb, mb = len(recs[1].nblocks), len(recs[1].mblocks)
    at = {"dnaSize": rec2, "nBlockCount": rec2 + 4, "nBlockStarts": rec2 + 8, "nBlockSizes": rec2 + 8 + 4 * nb}
    at["maskBlockCount"] = rec2 + 8 + 8 * nb
    at["maskBlockStarts"] = at["maskBlockCount"] + 4
    at["maskBlockSizes"] = at["maskBlockStarts"] + 4 * mb
    at["reserved"] = at["maskBlockStarts"] + 8 * mb
    at["packedDna"] = at["reserved"] + 4
    return at


@pytest.mark.parametrize("order", ["<", ">"])
def test_truncation_names_the_field(tmp_path, order):
    from deepgrp_amd import twobit
    recs = _small()
    raw = tc.write(recs, order)
    at = _layout(recs)
    assert at["packedDna"] + 6 == len(raw)
    path = tmp_path / "t.2bit"

    def refused(nbytes):
        path.write_bytes(raw[:nbytes])
        with pytest.raises(ValueError) as e:
            twobit.open_twobit(path)
        assert str(path) in str(e.value) and "truncated" in str(e.value)
        return str(e.value)

    assert "header" in refused(12)
    assert "index entry 0" in refused(16)
    assert "index entry 1" in refused(16 + 8 + 5)
    for field in ("dnaSize", "nBlockCount", "nBlockStarts", "nBlockSizes", "maskBlockCount", "maskBlockStarts", "maskBlockSizes",
                  "reserved", "packedDna"):
        msg = refused(at[field] + 2)
        assert field in msg and "record 1" in msg and "two" in msg, (field, msg)
    assert "packedDna" in refused(len(raw) - 1)
    path.write_bytes(raw)
    assert twobit.open_twobit(path).nrec == 2


@pytest.mark.parametrize("order", ["<", ">"])
def test_bad_blocks_and_version_are_refused(tmp_path, order):
    from deepgrp_amd import twobit
    rng = np.random.default_rng(6)
    path = tmp_path / "b.2bit"

    def refused(recs, version=0):
        path.write_bytes(tc.write(recs, order, version))
        with pytest.raises(ValueError) as e:
            twobit.open_twobit(path)
        assert str(path) in str(e.value)
        return str(e.value)

    msg = refused([tc._rec(rng, b"u", 50, [(10, 2), (4, 2)])])
    assert "nBlockStarts" in msg and "not ascending" in msg and "record 0" in msg
    msg = refused([tc._rec(rng, b"ok", 9), tc._rec(rng, b"u", 50, [], [(3, 1), (20, 2), (19, 2)])])
    assert "maskBlockStarts" in msg and "not ascending" in msg and "record 1" in msg and "block 2" in msg
    msg = refused([tc._rec(rng, b"p", 50, [(40, 11)])])
    assert "nBlock 0" in msg and "past dnaSize 50" in msg
    msg = refused([tc._rec(rng, b"p", 50, [], [(0, 1), (50, 1)])])
    assert "maskBlock 1" in msg and "past dnaSize 50" in msg
    # equal starts are ascending, a block may end at dnaSize, and a zero-length block at dnaSize reaches nothing
    path.write_bytes(tc.write([tc._rec(rng, b"fine", 50, [(4, 2), (4, 5), (50, 0)], [(49, 1)])], order))
    tb = twobit.open_twobit(path)
    assert tb.n_iv.tolist() == [[4, 9]] and tb.m_iv.tolist() == [[49, 50]]
    msg = refused([tc._rec(rng, b"v", 8)], version=1)
    assert "version 1" in msg


def test_is_twobit_reads_the_signature(tmp_path):
    from deepgrp_amd import gz, twobit
    fa, gzf, empty, short = tmp_path / "a.2bit", tmp_path / "b.2bit", tmp_path / "c.2bit", tmp_path / "d.2bit"
    fa.write_bytes(b">x\nACGT\n")
    gzf.write_bytes(gzip.compress(b">x\nACGT\n"))
    empty.write_bytes(b"")
    short.write_bytes(struct.pack("<I", tc.SIGNATURE)[:3])
    for p in (fa, gzf, empty, short, tmp_path / "missing.2bit", tmp_path):
        assert not twobit.is_twobit(p), p
    for order in "<>":
        real = tmp_path / f"real{ord(order)}.fa"                      # by its bytes, not by its name
        real.write_bytes(tc.write(_small(), order))
        assert twobit.is_twobit(real) and not gz.is_gzip(real)
    assert twobit.twobit_inputs(["-", str(fa), str(real), "x.npz", str(tmp_path / "missing")]) == [str(real)]
    with pytest.raises(ValueError, match="not a 2bit file"):
        twobit.open_twobit(fa)


def test_a_file_above_the_resident_limit_is_refused_before_any_device_work(tmp_path, monkeypatch):
    from deepgrp_amd import fasta
    (tmp_path / "x.2bit").write_bytes(tc.write(tc.odd_file()))
    monkeypatch.setattr(fasta, "RESIDENT_BYTES", 64)
    with pytest.raises(ValueError, match="x.2bit: more than 64 bytes .DGRP_FASTA_RESIDENT_BYTES.*read whole into device memory"):
        list(fasta.read_multi_fasta_device(tmp_path / "x.2bit"))


def test_symbols_exported_and_bound():
    from deepgrp_amd import _lib
    L = _lib.lib()
    for name in ("dgrp_twobit_workspace_bytes", "dgrp_twobit_encode_batch", "dgrp_twobit_text_batch"):
        assert name in _lib.exported_symbols() and hasattr(L, name), name
    assert L.dgrp_twobit_workspace_bytes(0) >= 0 and L.dgrp_twobit_workspace_bytes(-1) == 0
    assert L.dgrp_twobit_workspace_bytes(4096) >= 4096 * 48


def test_entries_check_their_tables_before_any_device_work():
    """Bad host tables are refused (DGRP_EINVAL, a message naming the record) with no device pointer ever touched; nrec == 0 is
    nothing to do."""
    from deepgrp_amd import _lib
    L = _lib.lib()
    i64 = lambda *v: np.array(v, np.int64)
    assert L.dgrp_twobit_encode_batch(None, 0, 0, None, None, None, None, 0, None, None, 0, None, 0, None) == 0
    assert L.dgrp_twobit_text_batch(None, 0, 0, None, None, None, None, None, None, 0, None, None, 0, None, None, 0, None, 0, None) == 0

    def enc(file_bytes=100, poff=10, dna=40, n_off=(0, 0), n_iv=0, out=0, cap=64):
        a = [i64(poff), i64(dna), i64(*n_off), i64(out)]
        rc = L.dgrp_twobit_encode_batch(None, file_bytes, 1, a[0].ctypes.data, a[1].ctypes.data, None, a[2].ctypes.data, n_iv,
                                        a[3].ctypes.data, None, cap, None, 0, None)
        return rc, L.dgrp_last_error().decode()

    for kw, word in ((dict(poff=95), "leave the file"), (dict(dna=1 << 32), "dnaSize"), (dict(cap=39), "leave the buffer"),
                     (dict(out=30), "leave the buffer"), (dict(n_off=(0, 2), n_iv=1), "h_n_iv_off"), (dict(n_off=(2, 1), n_iv=5), "h_n_iv_off"),
                     (dict(n_off=(0, 1), n_iv=1), "without d_n_iv"), (dict(), "NULL device pointer")):
        rc, msg = enc(**kw)
        assert rc == -1 and word in msg, (kw, msg)

    def txt(file_bytes=100, name=(4, 3), poff=10, dna=40, toff=0, cap=46, m_off=(0, 0), m_iv=0):
        a = [i64(name[0]), i64(name[1]), i64(poff), i64(dna), i64(0, 0), i64(*m_off), i64(toff)]
        rc = L.dgrp_twobit_text_batch(None, file_bytes, 1, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, None,
                                      a[4].ctypes.data, 0, None, a[5].ctypes.data, m_iv, a[6].ctypes.data, None, cap, None, 0, None)
        return rc, L.dgrp_last_error().decode()

    for kw, word in ((dict(name=(99, 3)), "name"), (dict(name=(4, 256)), "name"), (dict(poff=91), "leave the file"), (dict(cap=45), "leaves the buffer"),
                     (dict(m_off=(0, 3), m_iv=2), "h_m_iv_off"), (dict(m_off=(0, 1), m_iv=1), "without d_m_iv"), (dict(), "NULL device pointer")):
        rc, msg = txt(**kw)
        assert rc == -1 and word in msg, (kw, msg)


def _plan(tmp_path, files, **kw):
    from deepgrp_amd import masking
    args = argparse.Namespace(mask_dir=str(tmp_path / "masked"), mask=None, mask_classes=None, mask_gzip=False, FASTA=[str(f) for f in files])
    for k, v in kw.items():
        setattr(args, k, v)
    return masking.plan(args).files


def test_mask_plan_names_the_text_of_a_2bit_input(tmp_path, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    (tmp_path / "a").mkdir()
    tb, fa, named_fa = tmp_path / "genome.2bit", tmp_path / "plain.fa", tmp_path / "sly.fa"
    tb.write_bytes(tc.write(_small()))
    named_fa.write_bytes(tc.write(_small(), ">"))                      # a 2bit file whatever its name
    fa.write_bytes(b">x\nACGT\n")
    out = str(tmp_path / "masked")
    assert _plan(tmp_path, [tb, fa, named_fa]) == {str(tb): os.path.join(out, "genome.2bit.fa"), str(fa): os.path.join(out, "plain.fa"),
                                                  str(named_fa): os.path.join(out, "sly.fa.fa")}
    assert _plan(tmp_path, [tb, fa], mask_gzip=True) == {str(tb): os.path.join(out, "genome.2bit.fa.gz"), str(fa): os.path.join(out, "plain.fa.gz")}
    # the appended suffix takes part in the collision check ...
    clash = tmp_path / "genome.2bit.fa"
    clash.write_bytes(b">y\nAC\n")
    with pytest.raises(SystemExit) as e:
        _plan(tmp_path, [tb, clash])
    assert "collide" in str(e.value) and "genome.2bit.fa" in str(e.value)
    other = tmp_path / "a" / "genome.2bit"
    other.write_bytes(tc.write(_small()))
    with pytest.raises(SystemExit) as e:
        _plan(tmp_path, [tb, other], mask_gzip=True)
    assert "collide" in str(e.value) and "genome.2bit.fa.gz" in str(e.value)
    # ... and in the overwrite check: a copy written into the input's directory never lands on the 2bit file, but it does on a
    # FASTA input of that name
    assert _plan(tmp_path, [tb], mask_dir=str(tmp_path)) == {str(tb): str(clash)}
    with pytest.raises(SystemExit) as e:
        _plan(tmp_path, [clash], mask_dir=str(tmp_path))
    assert "overwrite" in str(e.value)


def test_sharded_run_refuses_a_2bit_input_before_anything_is_loaded(tmp_path):
    """WORLD_SIZE=2 without --split_contigs: the command exits with its message; neither torch nor the library was loaded."""
    tb = tmp_path / "genome.2bit"
    tb.write_bytes(tc.write(_small()))
    code = ("import sys\n"
            "from deepgrp_amd.__main__ import main\n"
            "try:\n"
            "    main(sys.argv[1:])\n"
            "except SystemExit as e:\n"
            "    import deepgrp_amd._lib as l\n"
            "    print('LOADED' if (l._lib is not None or 'torch' in sys.modules) else 'CLEAN')\n"
            "    raise\n")
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code, "predict", os.path.join(GOLDEN, "model_u8_T20.h5"), str(tb), "--output", str(tmp_path / "o.tsv")],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stderr
    assert str(tb) in r.stderr and "2bit" in r.stderr and "WORLD_SIZE" in r.stderr and "--split_contigs" in r.stderr
    assert r.stdout.strip() == "CLEAN"
    assert not (tmp_path / "o.tsv").exists()
