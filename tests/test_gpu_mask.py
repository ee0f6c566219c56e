"""predict --mask_dir on the GPU: dgrp_fasta_mask_batch, masking.mask_fasta and the command line against a brute-force statement of
the masked file written here -- a per-line Python loop over the file's bytes (the reference's line loop: every line stripped, '>'
lines open a record, a record without a name is dropped) that rewrites the sequence bytes covered by the expected TSV rows."""
import ctypes as C
import logging
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])
WS = b" \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"


def brute_records(data: bytes):
    """[(header, [byte positions of its sequence characters] or None if a sequence line is not ASCII)] in file order."""
    recs, cur, pos = [], None, 0
    while pos < len(data):
        e = pos
        while e < len(data) and data[e] not in (10, 13):
            e += 1
        term = 2 if data[e:e + 2] == b"\r\n" else (1 if e < len(data) else 0)
        line, s0 = data[pos:e], pos
        pos = e + term
        a, b = 0, len(line)
        while a < b and line[a] in WS:
            a += 1
        while b > a and line[b - 1] in WS:
            b -= 1
        if a == b:
            raise IndexError("blank line")
        if line[a] == 62:
            cur = None
            name = line[a + 1:b]
            if name:
                cur = [name.decode("utf-8", "replace"), []]
                recs.append(cur)
        elif cur is not None and cur[1] is not None:
            if not line.isascii():
                cur[1] = None
            else:
                cur[1] += list(range(s0 + a, s0 + b))
    return [(h, p) for h, p in recs]


def brute_mask(data: bytes, rows_per_record, mode: str, classes=None) -> bytes:
    """rows_per_record[k] = [(start, end, label), ...] of the k-th record brute_records finds."""
    out = bytearray(data)
    for k, (_h, positions) in enumerate(brute_records(data)):
        if positions is None:
            continue
        rows = sorted(rows_per_record[k]) if k < len(rows_per_record) else []
        j = 0
        for p, at in enumerate(positions):
            while j < len(rows) and rows[j][1] <= p:                    # (rows are disjoint)
                j += 1
            inside = j < len(rows) and rows[j][0] <= p and (rows[j][2] in classes if classes is not None else rows[j][2] > 0)
            c = out[at]
            if mode == "hard":
                out[at] = 78 if inside else c
            elif 65 <= c <= 90 or 97 <= c <= 122:
                out[at] = c | 0x20 if inside else c & 0xDF
    return bytes(out)


# ---------------------------------------------------------------- the kernel
def _random_rows(rng, n, dense=False):
    rows, p = [], 0
    while n and p < n:
        p += int(rng.integers(0, 3 if dense else 400))
        if p >= n:
            break
        ln = 1 if dense else int(rng.integers(1, 300))
        rows.append((p, min(p + ln, n), int(rng.integers(0, 5))))
        p = min(p + ln, n)
    return rows


def _body(rng, n, width, crlf, final_nl=True):
    seq = rng.choice(list(b"ACGTNacgtnRY*"), size=n).astype(np.uint8).tobytes()
    nl = b"\r\n" if crlf else b"\n"
    body = nl.join(seq[i:i + width] for i in range(0, n, width))
    return body + (nl if final_nl else b"")


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("mode", ["soft", "hard"])
def test_mask_batch_kernel_against_brute_force(inplace, mode):
    from deepgrp_amd._lib import check, lib
    L = lib()
    rng = np.random.default_rng(11 + inplace + 2 * (mode == "hard"))
    specs = [(1, 60, False), (5, 1, False), (200, 60, True), (3000, 60, False), (70_000, 70_000, False), (150_000, 66_000, True),
             (9000, 1, True), (1_100_000, 60, False), (4097, 61, False), (0, 60, False), (777, 60, False), (12_000, 60, True)]
    for _ in range(40):
        specs.append((int(rng.integers(1, 5000)), int(rng.integers(1, 100)), bool(rng.integers(0, 2))))
    buf, offs, lens, rowsets, bodies = bytearray(), [], [], [], []
    for k, (n, w, crlf) in enumerate(specs):
        buf += b">h%d x\n" % k
        buf += b"x" * int(rng.integers(0, 17))                      # any alignment of the body
        body = _body(rng, n, w, crlf, final_nl=k % 3 != 1) if n else b""
        offs.append(len(buf))
        lens.append(len(body))
        bodies.append(body)
        buf += body + b"\n"
        nseq = n
        if k == 1:
            rows = [(0, nseq, 2)]                                      # the whole body, first and last base
        elif k == 9 or k == 10:
            rows = []                                                  # zero rows
        elif k == 6:
            rows = _random_rows(rng, nseq, dense=True)                 # > 256 rows per tile
        else:
            rows = _random_rows(rng, nseq)
            if nseq > 2 and rng.random() < 0.5:
                rows = [(0, 1, 1)] + [r for r in rows if r[0] >= 2]
        rowsets.append(rows)
    classes = (1, 3)
    bits = sum(1 << c for c in classes)
    h_off, h_len = np.array(offs, np.int64), np.array(lens, np.int64)
    allrows = np.zeros(sum(len(r) for r in rowsets), SEG)
    row_off = np.zeros(len(specs) + 1, np.int64)
    i = 0
    for k, rows in enumerate(rowsets):
        for st, en, lab in rows:
            allrows[i] = (st, en, lab, k)
            i += 1
        row_off[k + 1] = i
    dev = torch.device("cuda", 0)
    d_raw = torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(dev)
    d_out = d_raw if inplace else torch.full_like(d_raw, 7)
    d_rows = torch.from_numpy(allrows.view(np.uint8)).to(dev)
    wb = L.dgrp_fasta_mask_workspace_bytes(len(specs), int(h_len.sum()), len(allrows))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    check(L.dgrp_fasta_mask_batch(d_raw.data_ptr(), len(specs), h_off.ctypes.data, h_len.ctypes.data, d_rows.data_ptr(),
                                  row_off.ctypes.data, 1 if mode == "hard" else 0, bits, d_out.data_ptr(), work.data_ptr(), wb,
                                  torch.cuda.current_stream().cuda_stream), "mask")
    got = d_out.cpu().numpy().tobytes()
    for k, body in enumerate(bodies):
        want = brute_mask(b">h\n" + body, [rowsets[k]], mode, classes)[3:]
        assert got[offs[k]:offs[k] + lens[k]] == want, f"body {k} {specs[k]}"
    if not inplace:                                                    # nothing outside the bodies is written
        outside = np.ones(len(buf), bool)
        for o, n in zip(offs, lens):
            outside[o:o + n] = False
        assert (np.frombuffer(got, np.uint8)[outside] == 7).all()


def test_mask_batch_refuses_a_row_beyond_the_body():
    from deepgrp_amd._lib import DgrpError, check, lib
    L = lib()
    dev = torch.device("cuda", 0)
    buf = b"ACGT\nAC\n"                                                # 6 sequence characters
    d_raw = torch.from_numpy(np.frombuffer(buf, np.uint8).copy()).to(dev)
    rows = np.array([(0, 2, 1, 0), (4, 7, 1, 0)], SEG)
    d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
    h_off, h_len, row_off = np.array([0], np.int64), np.array([len(buf)], np.int64), np.array([0, 2], np.int64)
    wb = L.dgrp_fasta_mask_workspace_bytes(1, len(buf), 2)
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    rc = L.dgrp_fasta_mask_batch(d_raw.data_ptr(), 1, h_off.ctypes.data, h_len.ctypes.data, d_rows.data_ptr(), row_off.ctypes.data,
                                 0, 2, d_raw.data_ptr(), work.data_ptr(), wb, torch.cuda.current_stream().cuda_stream)
    assert rc == -1                                                    # DGRP_EINVAL
    assert b"beyond" in L.dgrp_last_error()
    assert d_raw.cpu().numpy().tobytes() == buf                        # nothing written
    with pytest.raises(DgrpError):
        check(rc, "mask")


# ---------------------------------------------------------------- mask_fasta
def _mixed_file(rng) -> bytes:
    parts = [b"text before the first header\n"]
    parts.append(b">plain one\n" + _body(rng, 5000, 60, False))
    parts.append(b">crlf\r\n" + _body(rng, 3000, 70, True))
    parts.append(b">spaces\n" + b"\n".join(b"  " + _body(rng, 50, 50, False, False) + b" \t" for _ in range(30)) + b"\n")
    parts.append(b">\n" + _body(rng, 300, 60, False))                 # empty header: copied
    parts.append(b">nonascii\nACGT\xc3\xa9ACGT\nACGT\n")
    parts.append(b">lone cr\rACGTACGT\rACGT\n")
    parts.append(b">last\n" + _body(rng, 20_000, 80, False, False))
    return b"".join(parts)


def test_mask_fasta_mixed_file_and_ranges(tmp_path, caplog):
    from deepgrp_amd import fasta
    from deepgrp_amd.masking import mask_fasta
    rng = np.random.default_rng(3)
    data = _mixed_file(rng)
    fa = tmp_path / "in.fa"
    fa.write_bytes(data)
    recs = brute_records(data)
    assert [h for h, _p in recs] == ["plain one", "crlf", "spaces", "nonascii", "lone cr", "last"]
    per = [_random_rows(rng, len(p) if p is not None else 10) for _h, p in recs]
    rows = np.array([(st, en, lab, k) for k, rr in enumerate(per) for st, en, lab in rr], SEG)
    for mode, classes in (("soft", None), ("hard", (2, 4))):
        out = tmp_path / f"whole_{mode}.fa"
        with caplog.at_level(logging.WARNING):
            n = mask_fasta(str(fa), str(out), rows, mode=mode, classes=classes)
        assert n == 6
        assert "nonascii" in caplog.text
        want = brute_mask(data, per, mode, classes)
        assert out.read_bytes() == want
        # the same by parts: every range of whole chunks with its own record ordinals
        starts = fasta.chunk_starts_host(str(fa)).tolist() + [len(data)]
        cuts = [0, starts[2], starts[5], len(data)]
        parts = tmp_path / f"parts_{mode}.fa"
        with open(parts, "wb") as fh:
            fh.truncate(len(data))
        k0 = 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            nrec = len(brute_records(data[a:b]))
            sub = rows[(rows["contig"] >= k0) & (rows["contig"] < k0 + nrec)].copy()
            sub["contig"] -= k0
            mask_fasta(str(fa), str(parts), sub, mode=mode, classes=classes, ranges=[(a, b)])
            k0 += nrec
        assert parts.read_bytes() == want


# ---------------------------------------------------------------- the command line
def _expected_rows(orc, fasta_path, model_file, step, B, ml, xd, use_mss):
    """The reference CLI's rows per record (oracle, from the GPU's own probabilities), in file order."""
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.pipeline import upload_sequence
    model = dgmodel.load_model(model_file)
    T, Cn = model.input_shape[1], model.output_shape[2]
    out = []
    with open(fasta_path) as fh:
        for _header, seq in orc.read_multi_fasta(fh):
            st, d_idx = upload_sequence(seq.encode())
            nwin = orc.window_count(d_idx.numel(), T, step)
            probs = model.forward_windows(d_idx, step, 0, nwin).cpu().numpy() if nwin else np.zeros((0, T, Cn), np.float32)
            out.append([tuple(int(v) for v in r) for r in orc.predict_contig(seq, lambda _i: (lambda a, b: probs[a:a + b]), T, Cn,
                                                                                step, B, ml, xd, use_mss)])
    return out


def _cli_file(rng, T) -> bytes:
    seq = lambda n, alpha="ACGT": rng.choice(list(alpha), size=n).astype("U1")
    parts = [b"lines before the first header\n"]
    s1 = "NNNNN" + "".join(seq(4000)) + "NN"
    parts.append(b">chr1 some description\n" + "\n".join(s1[i:i + 60] for i in range(0, len(s1), 60)).encode() + b"\n")
    parts.append(b">short\n" + "".join(seq(T - 3)).encode() + b"\n")
    s3 = "".join(rng.choice(list("acgtn"), size=1500, p=[.23, .23, .23, .23, .08])).strip("n")
    parts.append(b">chr3\r\n" + "\r\n".join(s3[i:i + 70] for i in range(0, len(s3), 70)).encode() + b"\r\n")
    s4 = "".join(seq(2500))
    parts.append(b">odd\n" + "\n".join(" " + s4[i:i + 50] + "\t" for i in range(0, len(s4), 50)).encode() + b"\n")
    parts.append(b">\nACGTACGT\n")
    s5 = "".join(seq(3000))
    parts.append(b">tail\n" + "\n".join(s5[i:i + 60] for i in range(0, len(s5), 60)).encode())
    return b"".join(parts)


@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("model_name,use_mss", [("model_u16_T30_att_vlen.h5", True), ("model_u8_T20.h5", False)])
def test_cli_mask_dir_end_to_end(orc, tmp_path, mode, model_name, use_mss):
    from deepgrp_amd.__main__ import main
    from deepgrp_amd.fasta import LineLoop  # noqa: F401 -- the loop the rows are about
    rng = np.random.default_rng(21)
    model_file = os.path.join(GOLDEN, model_name)
    T = 30 if "T30" in model_name else 20
    data = _cli_file(rng, T)
    fa = tmp_path / "in.fa"
    fa.write_bytes(data)
    flags = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
    tail = [] if use_mss else ["-m"]
    plain_tsv = tmp_path / "plain.tsv"
    main(flags + ["predict", model_file, str(fa), "--output", str(plain_tsv)] + tail)
    mdir = tmp_path / "masked"
    tsv = tmp_path / "masked.tsv"
    main(["--mask_dir", str(mdir), "--mask", mode] + flags + [model_file, str(fa), "--output", str(tsv)] + tail)   # README form
    assert tsv.read_bytes() == plain_tsv.read_bytes()
    per = _expected_rows(orc, str(fa), model_file, 4, 7, 3, 5, use_mss)
    assert sum(len(r) for r in per) > 3
    got = (mdir / "in.fa").read_bytes()
    assert len(got) == len(data)
    assert got == brute_mask(data, per, mode)
    assert os.listdir(mdir) == ["in.fa"]
    if mode == "soft":
        # lower-case runs of the masked file, record by record, are exactly the rows (labels > 0; touching rows merge)
        for (_h, pos), rows in zip(brute_records(got), per):
            lower = np.array([97 <= got[p] <= 122 for p in pos], bool)
            want = np.zeros(len(pos), bool)
            for st, en, lab in rows:
                want[st:en] |= lab > 0
            assert (lower == want).all()
    # -vv: the staged path gives the same bytes
    mdir2 = tmp_path / "masked_vv"
    main(["-vv"] + flags + ["predict", model_file, str(fa), "--output", str(tmp_path / "vv.tsv"), "--mask_dir", str(mdir2),
                            "--mask", mode] + tail)
    main(["predict", model_file, str(fa), "--output", str(tmp_path / "reset.tsv")])    # (logging back to the default level)
    assert (mdir2 / "in.fa").read_bytes() == got
    # an all-N record stops predict: no masked file
    bad = tmp_path / "bad.fa"
    bad.write_bytes(data + b"\n>allN\nNNNNNNNNNN\n")
    mdir3 = tmp_path / "masked_bad"
    with pytest.raises(ValueError, match="negative dimensions"):
        main(flags + ["predict", model_file, str(bad), "--output", str(tmp_path / "bad.tsv"), "--mask_dir", str(mdir3)] + tail)
    assert os.listdir(mdir3) == []


def _rank_worker(rank, world, port, argv):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      DGRP_DIST_BACKEND="gloo")
    from deepgrp_amd.__main__ import main
    main(argv)


@pytest.mark.parametrize("split", [False, True])
def test_cli_mask_two_ranks(tmp_path, split):
    """Two ranks on GPU 0 over gloo, records sharded (each rank masks its own byte ranges of one temporary file) or every record
    split (rank 0 masks): the masked files equal the single-process ones."""
    import torch.multiprocessing as mp
    from deepgrp_amd import model as dgmodel, synthetic
    from deepgrp_amd.__main__ import main
    w = synthetic.trained_weights()
    mpath = str(tmp_path / "m.hdf5")
    dgmodel.save_keras_hdf5(mpath, w["kernel"], w["recurrent_kernel"], w["bias"], w["ff_kernel"], w["ff_bias"], None, vecsize=200)
    raw = synthetic.synthetic_chromosome(600_000, contig=3, flank=1000)[5000:-5000]
    rng = np.random.default_rng(4)
    fa, odd = tmp_path / "many.fa", tmp_path / "odd.fa"
    pos = 0
    with open(fa, "wb") as fh:
        for k in range(60):
            n = 150_000 if k in (7, 40) else int(rng.integers(1, 3000))
            seq = raw[pos:pos + n]
            pos += n
            fh.write(b">r%d\n" % k + b"\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + b"\n")
    body = raw[pos:pos + 30_000]
    with open(odd, "wb") as fh:
        fh.write(b"headerless\n>crlf\r\n" + b"\r\n".join(body[i:i + 60] for i in range(0, 9000, 60)) + b"\r\n")
        fh.write(b">spaces\n" + b"\n".join(body[i:i + 50] + b"  " for i in range(9000, 15000, 50)) + b"\n")
        fh.write(b">lower\n" + body[15000:].lower() + b"\n>\nACGT\n")
    common = ["-b", "7", "predict", mpath, str(fa), str(odd), "--mask", "soft"]
    main(common + ["--output", str(tmp_path / "single.tsv"), "--mask_dir", str(tmp_path / "single")])
    argv = common + ["--output", str(tmp_path / "ranks.tsv"), "--mask_dir", str(tmp_path / "ranks")] + (["--split_contigs"] if split else [])
    ctx = mp.get_context("spawn")
    port = 29400 + os.getpid() % 150 + (7 if split else 0)
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, argv)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    for name in ("many.fa", "odd.fa"):
        single = (tmp_path / "single" / name).read_bytes()
        assert (tmp_path / "ranks" / name).read_bytes() == single
        assert single != (tmp_path / name).read_bytes()
    assert sorted(os.listdir(tmp_path / "ranks")) == ["many.fa", "odd.fa"]
