"""Probability tracks of batches of short records on the GPU: dgrp_track_text_batch against the numpy statement of the format
(tracks.reference_text) per record and class, concatenated, byte for byte; its retry protocol, its one-record form against
dgrp_track_text, rows beyond 2^32 elements; dgrp_predict_batch_probs against dgrp_predict_batch and ContigPipeline.merged bit for
bit; the command line on a file of hundreds of short records (tracks, --track_gzip, TSV and masks untouched, which path ran); and
the stream contract of the two new device entries."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from stream_harness import FILLS, SEG, Harness, c_i64, dev_of, i64ptr       # noqa: E402
from test_gpu_tracks import NAMES, _column, _kernel_text, _trained_model, _write_fasta      # noqa: E402


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


def _batch_text(L, d_probs, row0, n, spos, names, cls, digits, bin, cap=None, fill=None):
    """dgrp_track_text_batch -> (rc, text buffer as numpy [cap], class offsets).  cap None: first with cap 0, then with exactly the
    room reported."""
    from deepgrp_amd.pipeline import stream_ptr
    r0, nn, sp = (np.ascontiguousarray(x, np.int64) for x in (row0, n, spos))
    cl = np.ascontiguousarray(cls, np.int32)
    noff = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(x) for x in names], out=noff[1:])
    blob = b"".join(names)
    wb = L.dgrp_track_batch_workspace_bytes(len(nn), nn.ctypes.data, sp.ctypes.data, bin, len(cl), len(blob))
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device=d_probs.device)
    off = np.full(len(cl) + 1, -1, np.int64)

    def call(text, room):
        return L.dgrp_track_text_batch(d_probs.data_ptr(), d_probs.shape[1], len(nn), r0.ctypes.data, nn.ctypes.data, sp.ctypes.data, blob,
                                       noff.ctypes.data, cl.ctypes.data, len(cl), digits, bin, text.data_ptr(), room, off.ctypes.data,
                                       work.data_ptr(), wb, stream_ptr())
    if cap is None:
        probe = torch.empty(1, dtype=torch.uint8, device=d_probs.device)
        assert call(probe, 0) == 0
        cap = int(off[-1])
    text = torch.full((max(cap, 1),), 0 if fill is None else fill, dtype=torch.uint8, device=d_probs.device)
    rc = call(text, cap)
    return rc, text.cpu().numpy(), off


# ---------------------------------------------------------------- 1. the statement
SWEEP_C, SWEEP_DIGITS, SWEEP_BINS, SWEEP_NREC = (2, 5, 16), (1, 2, 3, 4), (1, 7, 50, 200), (1, 2, 37, 1500)
SWEEP_CASES = len(SWEEP_C) * len(SWEEP_DIGITS) * len(SWEEP_BINS) * len(SWEEP_NREC)
# lines of the whole sweep by tracks.reference_text on a CPU with these seeds: 19_276_434 (see _sweep_case); the floor keeps the
# sweep from going empty without pinning numpy's random streams to the last line
SWEEP_MIN_LINES = 19_000_000


def _sweep_case(case, Cn, digits, bin, nrec):
    """One case, all on the host: (array [rows, C], row0, n, startpos, names, classes).  Records sit in the array with gaps of
    0.97 between them (rows no record owns), neighbours end and start with a bin of 1.0 in every selected class -- equal non-zero
    quantised values on both sides of every record boundary."""
    rng = np.random.default_rng(1000 + case)
    must = [1, max(bin - 1, 1), 63, 64, 65]
    n = [int(6000 ** rng.random()) for _ in range(nrec)]                       # 1..6000, most of them short
    if nrec >= 37:
        for i, v in enumerate(must):
            n[i * 7] = v
        n[-1] = 6000
    else:
        for i in range(nrec):
            n[i] = must[(case // 4 + i) % len(must)]
    gaps = rng.integers(0, 3, nrec) * 64
    row0, pos = [], 0
    for k in range(nrec):
        pos += int(gaps[k])
        row0.append(pos)
        pos += (n[k] + 63) // 64 * 64 if case % 2 else n[k]                     # the batch layout, or records back to back
    arr = rng.random((pos + 1, Cn)).astype(np.float32)
    k = int(rng.integers(1, min(Cn, 3) + 1))
    cls = [int(c) for c in rng.permutation(Cn)[:k]]
    if case % 2 == 0 and 0 not in cls:
        cls[int(rng.integers(0, k))] = 0
    spos = [int(rng.choice([0, bin * 3 + bin // 2, 10 ** 11 + 3])) for _ in range(nrec)]
    names = [NAMES[int(rng.integers(0, len(NAMES)))] if nrec < 1500 or rng.random() < 0.02 else NAMES[int(rng.integers(0, 2))]
             for _ in range(nrec)]
    owned = np.zeros(pos + 1, bool)
    for r in range(nrec):
        a, b = row0[r], row0[r] + n[r]
        owned[a:b] = True
        for c in cls:
            arr[a:b, c] = _column(rng, ("runs", "noise", "edges")[(case + r) % 3], n[r], digits)
            arr[a:min(a + bin, b), c] = 1.0
            arr[max(b - bin, a):b, c] = 1.0
    arr[~owned] = 0.97
    return arr, row0, n, spos, names, cls


def _sweep():
    case = 0
    for Cn in SWEEP_C:
        for digits in SWEEP_DIGITS:
            for bin in SWEEP_BINS:
                for nrec in SWEEP_NREC:
                    yield case, Cn, digits, bin, nrec
                    case += 1


def _want(arr, row0, n, spos, names, cls, digits, bin):
    from deepgrp_amd.tracks import reference_text
    return [b"".join(reference_text(arr[row0[r]:row0[r] + n[r], c], spos[r], names[r], digits, bin) for r in range(len(n))) for c in cls]


def test_track_batch_against_the_statement(L):
    dev = torch.device("cuda", 0)
    checked = lines = crossing = 0
    for case, Cn, digits, bin, nrec in _sweep():
        arr, row0, n, spos, names, cls = _sweep_case(case, Cn, digits, bin, nrec)
        want = _want(arr, row0, n, spos, names, cls, digits, bin)
        rc, text, off = _batch_text(L, torch.from_numpy(arr).to(dev), row0, n, spos, names, cls, digits, bin)
        assert rc == 0
        assert off.tolist() == np.r_[0, np.cumsum([len(w) for w in want])].tolist(), (case, Cn, digits, bin, nrec)
        for k, w in enumerate(want):
            assert text[off[k]:off[k + 1]].tobytes() == w, (case, Cn, digits, bin, nrec, cls[k])
        checked += 1
        lines += sum(w.count(b"\n") for w in want)
        crossing += (nrec - 1) * len(cls)
    print(f"sweep: {checked} cases, {lines} lines, {crossing} record boundaries with equal values on both sides")
    assert checked == SWEEP_CASES == 192
    assert lines >= SWEEP_MIN_LINES
    assert crossing > 50_000


# ---------------------------------------------------------------- 2. retry
def test_a_cap_one_byte_short_writes_nothing(L):
    arr, row0, n, spos, names, cls = _sweep_case(7, 5, 2, 7, 37)
    want = _want(arr, row0, n, spos, names, cls, 2, 7)
    total = sum(len(w) for w in want)
    d = torch.from_numpy(arr).cuda()
    rc, text, off = _batch_text(L, d, row0, n, spos, names, cls, 2, 7, cap=total - 1, fill=0x5A)
    assert rc == 0 and (text == 0x5A).all(), "a too-small buffer was written"
    assert off.tolist() == np.r_[0, np.cumsum([len(w) for w in want])].tolist()
    rc, text, off = _batch_text(L, d, row0, n, spos, names, cls, 2, 7, cap=total + 100, fill=0x5A)
    assert rc == 0 and text[:total].tobytes() == b"".join(want) and (text[total:] == 0x5A).all()


# ---------------------------------------------------------------- 3. one record
def test_one_record_is_dgrp_track_text(L):
    rng = np.random.default_rng(3)
    for Cn, digits, bin, n, startpos in ((5, 2, 1, 5000, 0), (16, 4, 7, 4097, 10 ** 11 + 3), (2, 1, 200, 70_001, 451), (5, 3, 50, 49, 26)):
        arr = rng.random((n, Cn)).astype(np.float32)
        cls = int(rng.integers(0, Cn))
        arr[:, cls] = _column(rng, "runs", n, digits)
        d = torch.from_numpy(arr).cuda()
        for name in NAMES:
            one = _kernel_text(d, startpos, name, cls, digits, bin)
            rc, text, off = _batch_text(L, d, [0], [n], [startpos], [name], [cls], digits, bin)
            assert rc == 0 and off.tolist() == [0, len(one)] and text[:len(one)].tobytes() == one and one


# ---------------------------------------------------------------- 4. 64-bit offsets
def test_rows_beyond_2_to_32_elements(L):
    from deepgrp_amd.tracks import reference_text
    total, Cn = 280_000_000, 16
    d = torch.zeros((total, Cn), dtype=torch.float32, device="cuda")
    a = (1 << 32) // Cn - 300                                   # record 1 straddles element 2^32
    row0, n, spos, names, cls = [5, a, total - 700], [100, 1000, 700], [3, 10 ** 11 + 3, 0], [b"lo", b"mid", b"hi"], [15, 0]
    cols = {c: [np.zeros(k, np.float32) for k in n] for c in cls}
    cols[15][0][7:9] = 0.25
    cols[15][1][250:600] = 0.5                                  # across the 2^32 mark
    cols[15][1][999] = 1.0
    cols[15][2][0] = 1.0                                        # equal to the end of record 1: still two lines
    cols[15][2][699] = 0.75
    cols[0][1][310:320] = 0.125
    cols[0][2][650:] = 0.0625
    for c in cls:
        for r in range(3):
            d[row0[r]:row0[r] + n[r], c] = torch.from_numpy(cols[c][r]).cuda()
    for bin in (1, 200):
        want = [b"".join(reference_text(cols[c][r], spos[r], names[r], 3, bin) for r in range(3)) for c in cls]
        rc, text, off = _batch_text(L, d, row0, n, spos, names, cls, 3, bin)
        assert rc == 0 and off.tolist() == [0, len(want[0]), len(want[0]) + len(want[1])]
        assert text[:off[1]].tobytes() == want[0] and text[off[1]:off[2]].tobytes() == want[1]
        assert want[0].count(b"\n") >= 4 and want[1].count(b"\n") == 2
    del d
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 5. dgrp_predict_batch_probs
def _models(orc, tmp_path):
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.pipeline import DeviceModel
    yield "gru", dgmodel.load_model(os.path.join(GOLDEN, "model_u8_T20.h5")), 4
    yield "attention", dgmodel.load_model(os.path.join(GOLDEN, "model_u60_T342_att.h5")), 50
    w = orc.LSTMWeights.random(48, 5, 40, seed=48, gain=2.0)
    yield "lstm", DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, None, vecsize=40, rnn="LSTM"), 7


def test_predict_batch_probs_is_predict_batch_and_merged(L, orc, tmp_path):
    from deepgrp_amd.pipeline import ContigPipeline
    dev = torch.device("cuda", 0)
    checked = 0
    for label, m, s in _models(orc, tmp_path):
        T, Cn = m.vecsize, m.classes
        rng = np.random.default_rng(len(label))
        lens = [1, 2, T - 1, T, T + 1, 63, 64, 65, T + s, T + 16 * s, 3 * T + 7, 4097] + [int(x) for x in rng.integers(1, 6000, 20)]
        offs, pos = [], 0
        for n in lens:
            pos += int(rng.integers(0, 37))
            offs.append(pos)
            pos += n
        d_base = torch.from_numpy(rng.choice(5, size=pos + 5, p=[.24, .25, .25, .24, .02]).astype(np.uint8)).to(dev)
        sp = [int(x) for x in rng.integers(0, 1000, len(lens))]
        ln = np.array(lens, np.int64)
        rows_total = L.dgrp_batch_rows(len(lens), ln.ctypes.data)
        assert rows_total == int(((ln + 63) // 64 * 64).sum())
        for fast in (False, True):
            pipe = ContigPipeline(m, s, 256, 4, 6, fast=fast)
            assert pipe.batchable()
            d_probs = torch.full((rows_total, Cn), 7.0, dtype=torch.float32, device=dev)
            got = pipe.run_batch(d_base, offs, lens, sp, list(range(len(lens))), d_probs=d_probs)
            np.testing.assert_array_equal(got, pipe.run_batch(d_base, offs, lens, sp, list(range(len(lens)))), err_msg=f"{label} fast={fast}")
            probs = d_probs.cpu().numpy()
            row = 0
            for o, n in zip(offs, lens):
                merged = pipe.merged(d_base[o:o + n].clone()).cpu().numpy()
                np.testing.assert_array_equal(probs[row:row + n].view(np.uint32), merged.view(np.uint32), err_msg=f"{label} fast={fast} n={n}")
                pad = (n + 63) // 64 * 64
                assert not probs[row + n:row + pad].view(np.uint32).any(), (label, fast, n)
                row += pad
                checked += 1
            assert row == rows_total
            pipe.close()
        m.close()
    assert checked == 3 * 2 * 32


# ---------------------------------------------------------------- 6. / 7. the command line
def _assembly(rng, T):
    from deepgrp_amd import synthetic
    raw = synthetic.synthetic_chromosome(1_200_000, contig=2, flank=1000)[2000:-2000]
    recs, p = [], 0
    for k in range(300):
        n = int(rng.integers(2000, 20_001))
        recs.append((b"ctg%d len=%d" % (k, n), raw[p:p + n]))
        p = (p + n) % (len(raw) - 20_000)
        if k == 100:
            recs.append((b"long one", raw[:300_000]))                                     # beyond SMALL_RECORD: on its own
        if k == 200:
            recs.append(("textα loop".encode(), b"NNN" + raw[5000:9000] + b"NN"))      # non-ASCII header: the line loop
        if k == 250:
            recs.append((b"tiny", raw[100:100 + T - 5]))                                   # below the window length
    return recs


def _expected_tracks(model_file, recs, classes, digits, bin):
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.pipeline import ContigPipeline, upload_sequence
    from deepgrp_amd.tracks import reference_text
    pipe = ContigPipeline(dgmodel.load_model(model_file), 50, 256, 50, 50, use_mss=True)
    out = {c: [] for c in classes}
    for header, seq in recs:
        st, d_idx = upload_sequence(seq)
        merged = pipe.merged(d_idx).cpu().numpy()
        for c in classes:
            out[c].append(reference_text(merged[:, c], st, header.split()[0], digits, bin))
    return {c: b"".join(v) for c, v in out.items()}


def test_cli_tracks_run_short_records_as_batches(tmp_path, monkeypatch):
    from deepgrp_amd.__main__ import main
    from deepgrp_amd.gz import BGZF_EOF
    from deepgrp_amd.pipeline import ContigPipeline
    model_file, T = _trained_model(tmp_path)
    recs = _assembly(np.random.default_rng(23), T)
    fa = tmp_path / "asm.fa"
    _write_fasta(fa, recs)
    batches, singles = [], []
    run_batch_probs, track_text_device = ContigPipeline.run_batch_probs, ContigPipeline.track_text_device

    def counted_batch(self, d_base, offsets, lengths, *a, **k):
        batches.append(len(lengths))
        return run_batch_probs(self, d_base, offsets, lengths, *a, **k)

    def counted_single(self, merged, startpos, name, *a, **k):
        singles.append(name)
        return track_text_device(self, merged, startpos, name, *a, **k)
    monkeypatch.setattr(ContigPipeline, "run_batch_probs", counted_batch)
    monkeypatch.setattr(ContigPipeline, "track_text_device", counted_single)
    main(["predict", model_file, str(fa), "--output", str(tmp_path / "p.tsv"), "--mask_dir", str(tmp_path / "mp")])
    assert not batches and not singles
    plain_tsv, plain_mask = (tmp_path / "p.tsv").read_bytes(), (tmp_path / "mp" / "asm.fa").read_bytes()
    assert plain_tsv.count(b"\n") > 300
    classes = (1, 2, 3, 4)
    for bin, flags in ((1, []), (50, []), (1, ["--track_gzip", "--gzip_level", "0"]), (50, ["--track_gzip", "--gzip_level", "1"])):
        del batches[:], singles[:]
        tdir = tmp_path / f"T{bin}{len(flags)}"
        main(["predict", model_file, str(fa), "--output", str(tmp_path / "t.tsv"), "--mask_dir", str(tmp_path / "mt"),
              "--track_dir", str(tdir), "--track_bin", str(bin)] + flags)
        assert (tmp_path / "t.tsv").read_bytes() == plain_tsv, (bin, flags)
        assert (tmp_path / "mt" / "asm.fa").read_bytes() == plain_mask, (bin, flags)
        want = _expected_tracks(model_file, recs, classes, 2, bin)
        ext = ".gz" if flags else ""
        assert sorted(os.listdir(tdir)) == sorted(f"asm.fa.class{c}.bedGraph{ext}" for c in classes)
        for c in classes:
            got = (tdir / f"asm.fa.class{c}.bedGraph{ext}").read_bytes()
            if flags:
                assert got.endswith(BGZF_EOF), "no BGZF EOF member"
                got = gzip.decompress(got)
            assert got == want[c], (bin, flags, c)
        assert sum(len(v) for v in want.values()) > 100_000
        # which path ran: the 301 short device records as batches, the long and the text-loop record one by one
        assert sum(batches) == 301 and max(batches) > 1, batches
        per_single = len(classes)
        assert len(singles) == 2 * per_single, singles                 # the long record and the text-loop record
        assert {s if isinstance(s, bytes) else s.encode("utf-8", "surrogateescape") for s in singles} == {b"long", "textα".encode()}


def test_cli_batched_tracks_failure_leaves_only_finished_inputs(tmp_path):
    """An all-N record in the second input stops predict as before: the first input's files are in place, nothing of the second."""
    from deepgrp_amd.__main__ import main
    model_file = os.path.join(GOLDEN, "model_u8_T20.h5")
    rng = np.random.default_rng(2)
    r = lambda k: rng.choice(list(b"ACGT"), size=k).astype(np.uint8).tobytes()
    good, bad = tmp_path / "good.fa", tmp_path / "bad.fa"
    _write_fasta(good, [(b"g%d" % k, r(300 + 17 * k)) for k in range(40)])
    _write_fasta(bad, [(b"b%d" % k, r(700)) for k in range(10)] + [(b"allN", b"N" * 40)] + [(b"c%d" % k, r(500)) for k in range(10)])
    for flags in ([], ["--track_gzip"]):
        tdir = tmp_path / f"T{len(flags)}"
        with pytest.raises(ValueError, match="negative dimensions"):
            main(["predict", model_file, str(good), str(bad), "--output", str(tmp_path / "o.tsv"), "--track_dir", str(tdir)] + flags)
        ext = ".gz" if flags else ""
        assert sorted(os.listdir(tdir)) == [f"good.fa.class{c}.bedGraph{ext}" for c in (1, 2, 3, 4)], flags
        tsv = (tmp_path / "o.tsv").read_bytes()
        assert b"allN" not in tsv and b"\tc0\t" not in tsv


# ---------------------------------------------------------------- 8. the stream contract
@pytest.fixture(scope="module")
def H(L):
    from deepgrp_amd.pipeline import require_gpu
    h = Harness(require_gpu())
    h.choose_side(L)
    return h


def _probs(seed, n, c):
    p = np.random.default_rng(seed).random((n, c)).astype(np.float32) ** 3
    return (p / p.sum(axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("fill", FILLS, ids=[f"fill{f:02X}" for f in FILLS])
def test_sync_track_text_batch(H, L, fill):
    from deepgrp_amd.tracks import reference_text
    c, digits, bin_ = 5, 2, 7
    n = np.array([1, 700, 64, 2500, 333], np.int64)
    row0 = np.r_[0, np.cumsum((n[:-1] + 63) // 64 * 64)].astype(np.int64)
    rows = int(row0[-1] + n[-1])
    spos = np.array([0, 123, 10 ** 11 + 3, 5, 77], np.int64)
    names = [b"chr\xce\xb1 1", NAMES[2], b"a", b"", b"scaffold_5"]
    noff = np.r_[0, np.cumsum([len(x) for x in names])].astype(np.int64)
    blob = b"".join(names)
    cls = np.array([3, 0, 2], np.int32)
    real, poison = _probs(13, rows, c), _probs(130, rows, c)
    real[row0[3] + 1000:row0[3] + 1500, 2] = 0.0
    real[row0[3] + 2000:row0[3] + 2500, 3] = 0.5
    want = [b"".join(reference_text(real[row0[r]:row0[r] + n[r], k], int(spos[r]), names[r], digits, bin_) for r in range(len(n))) for k in cls]
    total = sum(len(w) for w in want)
    cap = total + 64
    wb = L.dgrp_track_batch_workspace_bytes(len(n), n.ctypes.data, spos.ctypes.data, bin_, len(cls), len(blob))

    def call(b, wk, st, t):
        off = np.full(len(cls) + 1, -1, np.int64)
        nm = C.create_string_buffer(blob, len(blob))
        rc = L.dgrp_track_text_batch(b["p"].data_ptr(), c, len(n), i64ptr(t["row0"]), i64ptr(t["n"]), i64ptr(t["spos"]), nm, i64ptr(t["noff"]),
                                     t["cls"].ctypes.data, len(cls), digits, bin_, b["text"].data_ptr(), cap, off.ctypes.data, wk.data_ptr(), wb, st)
        C.memset(nm, ord("#"), len(blob))                                      # the names are a host table too
        return rc, off.tolist()
    late, off, _, off_idle = H.run(call, {"p": (real, poison)}, {"text": np.full(cap, 0x5A, np.uint8)}, work_bytes=wb, fill=fill, sync=True,
                                   tables={"row0": row0, "n": n.copy(), "spos": spos, "noff": noff, "cls": cls})
    assert off == off_idle == np.r_[0, np.cumsum([len(w) for w in want])].tolist()
    assert late["text"][:total].tobytes() == b"".join(want) and (late["text"][total:] == 0x5A).all()
    assert total > 5000


def test_sync_predict_batch_probs(H, L, orc):
    from test_gpu_streams import BATCH, MODELS, _batch_tables, _idx, _make_model
    for m, fill in [(MODELS[0], f) for f in FILLS] + [(MODELS[1], FILLS[0]), (MODELS[9], FILLS[0])]:
        fam, cell, u, T, att, c, s, level = m
        w, dm, view = _make_model(orc, m, gain=3.0)
        try:
            rng = np.random.default_rng(15)
            lens = np.array([1, T - 1, T, T + 1, 64, T + 16 * s, 1500, 333], np.int64)
            offs, size = _batch_tables(rng, lens)
            real, poison = _idx(rng, size), np.full(size, 4, np.uint8)
            spos = rng.integers(0, 1000, len(lens)).astype(np.int64)
            contig = np.arange(10, 10 + len(lens), dtype=np.int32)
            cap = 1024
            wb = L.dgrp_batch_workspace_bytes(view, len(lens), lens.ctypes.data, s)
            rows_total = L.dgrp_batch_rows(len(lens), lens.ctypes.data)

            def call(b, wk, st, t, probs=True):
                cnt = c_i64()
                args = (view, b["idx"].data_ptr(), len(lens), i64ptr(t["off"]), i64ptr(t["n"]), i64ptr(t["spos"]), t["contig"].ctypes.data, s,
                        BATCH, 4, 6, b["rec"].data_ptr(), cap, C.byref(cnt), wk.data_ptr(), wb, st)
                rc = L.dgrp_predict_batch_probs(*args, b["probs"].data_ptr()) if probs else L.dgrp_predict_batch(*args)
                return rc, cnt.value
            outs = {"rec": np.full(cap * SEG.itemsize, 0xAB, np.uint8), "probs": np.full((rows_total, c), 7.0, np.float32)}
            tables = {"off": offs, "n": lens.copy(), "spos": spos, "contig": contig}
            late, cnt, _, cnt_idle = H.run(call, {"idx": (real, poison)}, outs, work_bytes=wb, fill=fill, sync=True, tables=tables)
            plain, cnt_plain, _, _ = H.run(lambda b, wk, st, t: call(b, wk, st, t, probs=False), {"idx": (real, poison)}, outs, work_bytes=wb,
                                           fill=fill, sync=True, tables=tables)
            assert cnt == cnt_idle == cnt_plain > len(lens)
            np.testing.assert_array_equal(late["rec"], plain["rec"])
            assert (plain["probs"] == 7.0).all(), "dgrp_predict_batch wrote to a buffer it was not given"
            row = 0
            for r, n in enumerate(lens):
                out = torch.zeros((int(n), c), dtype=torch.float32, device=H.dev)
                wk = torch.empty(max(L.dgrp_forward_merge_record_workspace_bytes(view, int(n), s), 256), dtype=torch.uint8, device=H.dev)
                d_idx = dev_of(real[offs[r]:offs[r] + n], H.dev)
                assert L.dgrp_forward_merge_record(view, d_idx.data_ptr(), int(n), s, BATCH, out.data_ptr(), wk.data_ptr(), wk.numel(), None) == 0
                torch.cuda.synchronize()
                np.testing.assert_array_equal(late["probs"][row:row + n].view(np.uint32), out.cpu().numpy().view(np.uint32), err_msg=f"{fam} record {r}")
                pad = (int(n) + 63) // 64 * 64
                assert not late["probs"][row + n:row + pad].any()
                row += pad
        finally:
            L.dgrp_model_destroy(view)
            dm.close()
