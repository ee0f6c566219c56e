"""The batched track entries without a GPU: the four symbols of the ABI, every refusal of dgrp_track_text_batch with its message,
the empty batch, the workspace function, and RecordRunner.work_items / outputs / results with a TrackSpec, with scores and a stand-in pipe."""
import ctypes as C

import numpy as np
import pytest

EINVAL = -1
NEW = ("dgrp_batch_rows", "dgrp_predict_batch_probs", "dgrp_track_batch_workspace_bytes", "dgrp_track_text_batch")


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd import _lib
    return _lib.lib()


def _err(L):
    return L.dgrp_last_error().decode("utf-8", "replace")


def test_the_four_symbols_are_exported_and_bound(L):
    from deepgrp_amd import _lib
    for name in NEW:
        assert name in _lib.exported_symbols(), name
        assert hasattr(L, name), name
    assert L.dgrp_abi_version() == 1


def test_batch_rows_is_the_layout_of_the_batch(L):
    n = np.array([1, 63, 64, 65, 200, 6000], np.int64)
    assert L.dgrp_batch_rows(len(n), n.ctypes.data) == int(((n + 63) // 64 * 64).sum()) == 64 * 3 + 128 + 256 + 6016
    assert L.dgrp_batch_rows(1, n.ctypes.data) == 64
    assert L.dgrp_batch_rows(0, None) == 0


def _call(L, C_=5, nrec=2, row0=(0, 64), n=(10, 20), spos=(0, 3), names=b"abcd", name_off=(0, 2, 4), cls=(1, 2), ncls=None, digits=2,
          bin=1, cap=0, class_off=True):
    """dgrp_track_text_batch with host tables only (every device pointer is a dummy that a refusal never touches)."""
    r0, nn, sp = (np.array(x, np.int64) for x in (row0, n, spos))
    no = np.array(name_off, np.int64)
    cl = np.array(cls, np.int32)
    ncls = len(cls) if ncls is None else ncls
    off = np.full(max(ncls, 0) + 1 + 64, -7, np.int64)
    rc = L.dgrp_track_text_batch(0x1000, C_, nrec, r0.ctypes.data, nn.ctypes.data, sp.ctypes.data, names, no.ctypes.data, cl.ctypes.data, ncls,
                                 digits, bin, None, cap, off.ctypes.data if class_off else None, 0x1000, 1 << 40, None)
    return rc, off


@pytest.mark.parametrize("kw,words", [
    (dict(nrec=-1), ("bad nrec", "-1")),
    (dict(C_=0), ("bad C",)),
    (dict(C_=65), ("bad C",)),
    (dict(cls=(), ncls=0), ("ncls must lie in 1..C",)),
    (dict(cls=(0, 1, 2, 3, 4, 0), ncls=6), ("ncls must lie in 1..C",)),
    (dict(cls=(1, 5)), ("class 5", "0..4")),
    (dict(cls=(-1,)), ("class -1",)),
    (dict(digits=0), ("digits must lie in 1..4", "0")),
    (dict(digits=5), ("digits must lie in 1..4", "5")),
    (dict(bin=0), ("bad bin 0",)),
    (dict(bin=(1 << 40) + 1), ("bad bin",)),
    (dict(cap=-1), ("bad cap",)),
    (dict(n=(10, 0)), ("record 1", "bad n 0")),
    (dict(n=((1 << 40) + 1, 5)), ("record 0", "bad n")),
    (dict(spos=(0, -2)), ("record 1", "bad offset -2")),
    (dict(spos=((1 << 40) + 1, 0)), ("record 0", "bad offset")),
    (dict(row0=(0, -64)), ("record 1", "bad first row")),
    (dict(name_off=(0, 3, 2)), ("record 1", "descending name offsets")),
    (dict(name_off=(-1, 2, 4)), ("record 0", "bad name offset")),
    (dict(class_off=False), ("NULL h_class_off",)),
    (dict(names=None), ("NULL pointer",)),
])
def test_refusals_name_the_entry_and_the_record(L, kw, words):
    rc, _off = _call(L, **kw)
    msg = _err(L)
    assert rc == EINVAL, (kw, rc, msg)
    assert msg.startswith("dgrp_track_text_batch: "), msg
    for w in words:
        assert w in msg, (kw, msg)


def test_null_device_pointers_are_refused(L):
    n, sp, r0, no, cl = np.array([5], np.int64), np.array([0], np.int64), np.array([0], np.int64), np.array([0, 1], np.int64), np.array([1], np.int32)
    off = np.zeros(2, np.int64)
    for probs, work in ((None, 0x1000), (0x1000, None)):
        rc = L.dgrp_track_text_batch(probs, 5, 1, r0.ctypes.data, n.ctypes.data, sp.ctypes.data, b"x", no.ctypes.data, cl.ctypes.data, 1, 2, 1,
                                     None, 0, off.ctypes.data, work, 1 << 30, None)
        assert rc == EINVAL and "dgrp_track_text_batch: NULL pointer" in _err(L)
    # d_text may be NULL only with cap 0
    rc = L.dgrp_track_text_batch(0x1000, 5, 1, r0.ctypes.data, n.ctypes.data, sp.ctypes.data, b"x", no.ctypes.data, cl.ctypes.data, 1, 2, 1,
                                 None, 10, off.ctypes.data, 0x1000, 1 << 30, None)
    assert rc == EINVAL and "NULL pointer" in _err(L)


def test_an_empty_batch_needs_no_device(L):
    rc, off = _call(L, nrec=0, cls=(3, 1, 0))
    assert rc == 0, _err(L)
    assert off[:4].tolist() == [0, 0, 0, 0] and (off[4:] == -7).all()
    # the offsets are filled in full in front of every refusal that comes after the class count
    rc, off = _call(L, cls=(1, 2, 3), n=(10, 0))
    assert rc == EINVAL and off[:4].tolist() == [0, 0, 0, 0]
    h = C.c_int64(-1)
    assert L.dgrp_predict_batch_probs(None, None, 0, None, None, None, None, 50, 256, 50, 50, None, 0, C.byref(h), None, 0, None, None) == EINVAL
    assert "dgrp_predict_batch_probs: bad arguments" in _err(L)


def test_workspace_is_zero_on_bad_input_and_grows(L):
    def wb(n=(1000, 2000), spos=(0, 5), bin=1, ncls=2, names=10, nrec=None):
        nn, sp = np.array(n, np.int64), np.array(spos, np.int64)
        return L.dgrp_track_batch_workspace_bytes(len(n) if nrec is None else nrec, nn.ctypes.data, sp.ctypes.data, bin, ncls, names)
    base = wb()
    assert base > 0
    for bad in (dict(nrec=-1), dict(bin=0), dict(bin=(1 << 40) + 1), dict(ncls=0), dict(ncls=65), dict(names=-1), dict(n=(1000, 0)),
                dict(n=(1000, (1 << 40) + 1)), dict(spos=(0, -1)), dict(spos=((1 << 40) + 1, 0))):
        assert wb(**bad) == 0, bad
    assert L.dgrp_track_batch_workspace_bytes(2, None, None, 1, 2, 0) == 0
    assert L.dgrp_track_batch_workspace_bytes(0, None, None, 1, 2, 0) > 0
    assert wb(n=(1000, 2000) + (1,) * 500, spos=(0, 5) + (0,) * 500) > base          # records
    assert wb(n=(100_000, 2000)) > base                                               # bins
    assert wb(bin=50) < base
    assert wb(ncls=5) > base                                                          # classes
    assert wb(names=100_000) > base + 90_000                                          # names
    # 4 bytes per bin and class at least
    assert wb(n=(1_000_000,), spos=(0,), ncls=3) >= 3 * 4 * 1_000_000


SEG = [("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")]


class FakeModel:
    vecsize, units, classes, attention = 20, 32, 5, False


class FakePipe:
    """Stands in for a ContigPipeline: `seen` lists the methods the runner called, `calls` the (names, chrom0) of every batch's
    texts -- both in the order the pool's threads got there, so they are compared as sets or sorted."""
    model, step = FakeModel(), 4

    def __init__(self):
        self.seen, self.calls = [], []

    def batchable(self):
        return True

    def run_batch(self, base, offsets, lengths, startposes, contigs, who="run_batch"):
        self.seen.append(who)
        out = np.zeros(len(lengths), dtype=SEG)
        out["start"], out["end"], out["label"], out["contig"] = offsets, lengths, 1, contigs
        return out

    def run_idx(self, d_idx, startpos, contig=0):
        self.seen.append("run_idx")
        return np.array([(startpos, startpos + 1, 2, contig)], dtype=SEG)

    def run(self, seq, contig=0):
        self.seen.append("run")
        return np.array([(0, len(seq), 2, contig)], dtype=SEG)

    def run_batch_probs(self, base, offsets, lengths, startposes, contigs):
        rows = self.run_batch(base, offsets, lengths, startposes, contigs, "run_batch_probs")
        return rows, "probs", np.arange(len(lengths)) * 64

    def merged(self, d_idx):
        self.seen.append("merged")
        raise AssertionError("the stand-in has no forward pass")

    def batch_track_texts(self, d_probs, row0, ln, startposes, names, spec, chrom0=0):
        assert d_probs == "probs" and len(row0) == len(ln) == len(startposes) == len(names)
        self.calls.append((tuple(names), chrom0))
        return [b"".join(b"%s:%d;" % (nm.encode(), c) for nm in names) for c in spec.classes]

    def batch_row_offsets(self, rows, contigs):
        from deepgrp_amd.pipeline import ContigPipeline
        return ContigPipeline.batch_row_offsets(rows, contigs)                          # host arithmetic: the real one

    def row_scores_batch(self, d_probs, row0, lengths, startposes, rows, row_off):
        assert d_probs == "probs" and row_off.tolist() == list(range(len(lengths) + 1))     # the stand-in: a row per record
        return [("score", int(n)) for n in lengths]


class Buf:
    def __getitem__(self, _s):
        return self

    def numel(self):
        return 0


def _nine_records():
    from deepgrp_amd import runner as rn
    from deepgrp_amd.fasta import DeviceRecord
    a, b = Buf(), Buf()
    key = lambda h: (h + " description", h)
    return [(key("r0"), DeviceRecord(0, None, 100, a, 0)), (key("r1"), DeviceRecord(2, None, 50, a, 200)),
            (key("r2"), DeviceRecord(0, None, 70, b, 0)),                                  # other buffer: new batch
            (key("r3"), "ACGT"),                                                           # text record: single
            (key("r4"), DeviceRecord(0, None, 30, b, 100)),
            (key("r5"), DeviceRecord(0, None, rn.SMALL_RECORD + 1, b, 200)),               # long: single
            (key("r6"), DeviceRecord(4, None, -4, b, 300)),                                # all-N: single (and raises when run)
            (key("r7"), DeviceRecord(1, None, 10, b, 400)), (key("r8"), DeviceRecord(1, None, 10, b, 500))]


def test_runner_batches_short_records_with_a_track_spec():
    """work_items with a TrackSpec groups exactly as without one; outputs hands batches out as batches, the rest one by one,
    in input order, and an all-N record raises in place."""
    from deepgrp_amd import runner as rn
    from deepgrp_amd.fasta import DeviceRecord
    from deepgrp_amd.tracks import TrackSpec
    spec = TrackSpec((1, 3), 2, 1)
    key = lambda h: (h + " description", h)
    recs = _nine_records()
    pipe = FakePipe()
    with_tracks, without = rn.RecordRunner(pipe, workers=2, tracks=spec), rn.RecordRunner(pipe, workers=2)
    shape = lambda r: [("batch", [kk[1] for kk, _ in v]) if k is rn._BATCH else (k[1], None) for k, v in r.work_items(recs)]
    want = [("batch", ["r0", "r1"]), ("batch", ["r2"]), ("r3", None), ("batch", ["r4"]), ("r5", None), ("r6", None), ("batch", ["r7", "r8"])]
    assert shape(with_tracks) == want == shape(without)
    assert with_tracks._batch_cost(1000) > without._batch_cost(1000)
    # batches come out as batches with the texts of the whole batch; the all-N record stops the run where it stands
    def one(rec, name, chrom):
        if isinstance(rec, DeviceRecord) and rec.length < 0:
            raise ValueError("negative dimensions are not allowed")
        return np.zeros(0, SEG), None, [b"one:" + name.encode()] * 2
    with_tracks.run_record = one
    got = []
    with pytest.raises(ValueError, match="negative dimensions"):
        for kind, k, rows, scores, texts in with_tracks.outputs(recs):
            assert scores is None
            got.append((kind, [kk[1] for kk in k] if kind == "batch" else k[1], len(rows), texts))
    assert [(g[0], g[1]) for g in got] == [("batch", ["r0", "r1"]), ("batch", ["r2"]), ("one", "r3"), ("batch", ["r4"]), ("one", "r5")]
    assert got[0][3] == [b"r0:1;r1:1;", b"r0:3;r1:3;"] and got[0][2] == 2
    assert got[2][3] == [b"one:r3"] * 2
    assert sorted(names for names, _chrom0 in pipe.calls)[:3] == [("r0", "r1"), ("r2",), ("r4",)]
    # records that do not batch (text, long, text) come out record by record, with their keys and their own texts
    lone = [recs[3], recs[5], (key("r9"), "TTGA")]
    assert [(kind, k, texts) for kind, k, _rows, _scores, texts in with_tracks.outputs(lone)] == \
        [("one", key(h), [b"one:" + h.encode()] * 2) for h in ("r3", "r5", "r9")]


def test_one_path_for_rows_tracks_and_scores():
    """The four runners (tracks or not, scores or not) group the same records into the same work items; outputs yields None for
    what was not asked for and a batch's scores and texts together; the plain runner's results are 3-tuples from the fused calls
    alone; the record ordinals count the input's records without a gap or a repeat."""
    from deepgrp_amd import runner as rn
    from deepgrp_amd.fasta import DeviceRecord
    from deepgrp_amd.tracks import TrackSpec
    recs = _nine_records()
    spec = TrackSpec((1, 3), 2, 1, None, False, True)                                       # bigWig: the ordinals reach the pipe
    runners = {(t, sc): rn.RecordRunner(FakePipe(), workers=2, tracks=spec if t else None, scores=sc)
               for t in (False, True) for sc in (False, True)}
    shape = lambda r: [("batch", [kk[1] for kk, _ in v]) if k is rn._BATCH else (k[1], None) for k, v in r.work_items(recs)]
    shapes = [shape(r) for r in runners.values()]
    assert all(sh == shapes[0] for sh in shapes) and len(shapes[0]) == 7 and sum(len(v or [0]) for _k, v in shapes[0]) == 9

    singles = []                                                                            # (name, chrom) of every lone record

    def one(r):
        def run(rec, name, chrom):
            singles.append((name, chrom))
            if isinstance(rec, DeviceRecord) and rec.length < 0:
                raise ValueError("negative dimensions are not allowed")
            return np.zeros(0, SEG), [] if r.scores else None, [b"one"] if r.tracks is not None else None
        return run
    for (t, sc), r in runners.items():
        if t or sc:
            r.run_record = one(r)
        del singles[:]
        got = []
        with pytest.raises(ValueError, match="negative dimensions"):
            for out in (r.outputs(recs) if t or sc else r.outputs([(k[0], rec) for k, rec in recs])):
                got.append(out)
        assert [len(out) for out in got] == [5] * 5 and [out[0] for out in got] == ["batch", "batch", "one", "batch", "one"], (t, sc)
        for kind, _key, rows, scores, texts in got:
            assert (scores is not None) == sc and (texts is not None) == t, (t, sc, kind)
        # a batch's scores and texts come together, from one run_batch_probs call
        if t and sc:
            assert got[0][3] == [("score", 100), ("score", 50)] and got[0][4] == [b"r0:1;r1:1;", b"r0:3;r1:3;"]
            assert set(r.pipe.seen) == {"run_batch_probs"}
        if t:
            # ordinals: the chrom0 of the batches and the chrom of the singles count the records, the all-N record included (the
            # batch behind it, records 7 and 8, may have run on the pool before the all-N record raised)
            before = {(("r0", "r1"), 0), (("r2",), 2), (("r4",), 4)}
            assert before <= set(r.pipe.calls) <= before | {(("r7", "r8"), 7)} and len(r.pipe.calls) == len(set(r.pipe.calls)), r.pipe.calls
            assert sorted(singles) == [("r3", 3), ("r5", 5), ("r6", 6)], (sc, singles)
    # the plain runner: 3-tuples with arbitrary keys, and only the fused calls
    plain = rn.RecordRunner(FakePipe(), workers=2)
    ok = [(k[0], rec) for k, rec in recs if not (isinstance(rec, DeviceRecord) and rec.length < 0)]
    res = list(plain.results(ok))
    assert [len(x) for x in res] == [3] * 6
    assert [(x[0], x[1]) for x in res][:3] == [("batch", ["r0 description", "r1 description"]), ("batch", ["r2 description"]),
                                               ("one", "r3 description")]
    assert set(plain.pipe.seen) == {"run_batch", "run_idx", "run"} and len(plain.pipe.seen) == 6
    assert [x[3:] for x in plain.outputs(ok)] == [(None, None)] * 6
