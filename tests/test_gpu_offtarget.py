"""The five device entries of `evaluate --offtarget`, each against its Python statement and the entry it stands beside:
dgrp_rm_parse_all (the host statement of annotation.read_listing(all_rows=True); dgrp_rm_parse_fields byte for byte on the numbered
rows), dgrp_token_ids (annotation.family_ranks), dgrp_paint_keys_batch (offtarget.reference_keys; dgrp_paint_rows_batch below key
64), dgrp_key_crosstab_batch (offtarget.reference_crosstab; dgrp_confusion_matrix) and dgrp_row_key_classes_batch
(offtarget.reference_row_classes; dgrp_row_hits_batch).  Every count is an integer: equal means equal."""
import ctypes as C

import numpy as np
import pytest

import rm_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from deepgrp_amd import annotation, offtarget, strata                   # noqa: E402
from stream_harness import SEG, Harness, i64ptr, last_error             # noqa: E402

EINVAL, ENOMEM = -1, -3
NONE = 0xFFFFFFFF
ROW_KEYS = ("begin", "end", "number", "name_pos", "name_len", "line", "millidiv")
FAM_KEYS = ("fam_pos", "fam_len", "fam2_pos", "fam2_len")


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


@pytest.fixture(scope="module")
def H(L, dev):
    h = Harness(dev)
    h.choose_side(L)
    return h


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


# ================================================================================================ the parser
def _straddle(edge, back, fam, rmsk=False):
    """A listing whose last line's family token starts `back` bytes in front of byte `edge` (and ends behind it)."""
    if rmsk:
        probe = rm_cases.rmsk_line(ctg="chrS", start=5, end=60, cls=fam.split("/")[0], fam=fam.split("/")[1])
        token = fam.replace("/", "\t")
    else:
        probe = rm_cases.out_line(ctg="chrS", begin=5, end=60, fam=fam)
        token = fam
    at = probe.index(token)
    data = rm_cases.sized_text(edge - back - at) + (probe + "\n").encode("ascii")
    start = edge - back
    assert data[start:start + len(token)] == token.encode() and start < edge < start + len(token)
    return data


PARSER_CASES = (rm_cases.cases(annotation.TILE_BYTES) + [("generated_4000", rm_cases.generated(4000))]
                + [(f"chunk_edge_back{b}", _straddle(128 * 301, b, "DNA/hAT-Charlie")) for b in (1, 4, 14)]
                + [(f"tile_edge_back{b}", _straddle(annotation.TILE_BYTES, b, "DNA/hAT-Charlie")) for b in (1, 4, 14)]
                + [("tile_edge_rmsk", _straddle(2 * annotation.TILE_BYTES, 3, "LTR/ERVK", rmsk=True)),
                   ("chunk_edge_rmsk", _straddle(128 * 9, 5, "LTR/ERVK", rmsk=True))])


def _device_text(data):
    buf = torch.empty(max(len(data), 1), dtype=torch.uint8, device="cuda")
    if data:
        buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf[:len(data)]


def _host(out, counts, keys):
    return {k: out[k][:counts[1]].cpu().numpy() for k in keys}


def _tokens_of(data, rows):
    a = [data[int(p):int(p) + int(n)] for p, n in zip(rows["fam_pos"], rows["fam_len"])]
    b = [data[int(p):int(p) + int(n)] for p, n in zip(rows["fam2_pos"], rows["fam2_len"])]
    return [(x + b"/" + y if len(y) else x).decode("ascii") for x, y in zip(a, b)]


@pytest.mark.parametrize("name,data", PARSER_CASES, ids=[c[0] for c in PARSER_CASES])
def test_all_rows_entry_against_the_fields_entry_and_the_host_statement(tmp_path, name, data):
    d_text = _device_text(data)
    c_f, o_f, rc_f = annotation.parse_device(d_text, len(data), fields=True)
    c_a, o_a, rc_a = annotation.parse_device(d_text, len(data), all_rows=True)
    assert rc_f == rc_a == 0 and c_a[0] == c_f[0] and c_a[3] == c_f[3] == 0 and c_a[1] >= c_f[1]
    old, new = _host(o_f, c_f, ROW_KEYS), _host(o_a, c_a, ROW_KEYS + FAM_KEYS)
    numbered = new["number"] > 0
    for k in ROW_KEYS:
        assert new[k][numbered].tobytes() == old[k].tobytes(), k
    path = tmp_path / "case.out"
    path.write_bytes(data)
    want = annotation.read_listing(str(path), device=False, all_rows=True)
    assert want.route == "host" and len(want) == c_a[1]
    for k in ("begin", "end", "number", "line", "millidiv"):
        np.testing.assert_array_equal(new[k], getattr(want, k), err_msg=k)
    tokens = _tokens_of(data, new)
    assert tokens == [want.families[i] for i in want.family_id]
    assert all(n2 == 0 or p2 > p for p, p2, n2 in zip(new["fam_pos"], new["fam2_pos"], new["fam2_len"]))
    if name.startswith(("chunk_edge_", "tile_edge_")):
        assert tokens[-1] in ("DNA/hAT-Charlie", "LTR/ERVK") and new["number"][-1] == 0
        assert (new["fam2_len"][-1] > 0) == name.endswith("rmsk")
    if name == "rmsk_class_equals_family":
        assert tokens == ["Satellite", "HSATII"] and new["fam2_len"].tolist() == [0, 0]
    got = annotation.listing_of_device_text(str(path), d_text, len(data), all_rows=True) if len(data) else want
    assert got.families == want.families and got.family_id.tobytes() == want.family_id.tobytes()
    assert got.run_names == want.run_names and got.run_first.tolist() == want.run_first.tolist()


def test_all_rows_twice_the_same_bytes_and_the_flags():
    data = dict(PARSER_CASES)["generated_4000"]
    d_text = _device_text(data)
    a = annotation.parse_device(d_text, len(data), all_rows=True)
    b = annotation.parse_device(d_text, len(data), all_rows=True)
    assert a[0] == b[0] and a[0][1] > annotation.parse_device(d_text, len(data))[0][1]
    for k in ROW_KEYS + FAM_KEYS:
        assert a[1][k][:a[0][1]].cpu().numpy().tobytes() == b[1][k][:a[0][1]].cpu().numpy().tobytes(), k
    for _name, bad in rm_cases.fallback_cases():
        c, _o, rc = annotation.parse_device(_device_text(bad), len(bad), all_rows=True)
        assert rc == 0 and c[3] == 1
    short = annotation.parse_device(d_text, len(data), cap=a[0][1] - 1, all_rows=True)
    assert short[2] == ENOMEM and short[0][1] == a[0][1] and "dgrp_rm_parse_all" in last_error()


# ================================================================================================ the token ids
def _spell(tokens):
    """tokens: str (one span) or (a, b) (two spans, the logical string a/b) -> (text, pos, len, pos2, len2, the logical strings)"""
    text, pos, ln, pos2, ln2, logical = bytearray(b"#"), [], [], [], [], []
    for t in tokens:
        a, b = (t, "") if isinstance(t, str) else t
        pos.append(len(text))
        text += a.encode() + b"\t"
        ln.append(len(a))
        pos2.append(len(text) if b else pos[-1])
        text += b.encode() + b" "
        ln2.append(len(b))
        logical.append(a + "/" + b if b else a)
    return (bytes(text), np.array(pos, np.int64), np.array(ln, np.int32), np.array(pos2, np.int64), np.array(ln2, np.int32), logical)


def _ids(tokens):
    text, pos, ln, pos2, ln2, logical = _spell(tokens)
    d_text = _device_text(text)
    got = annotation.token_ids_device(d_text, len(text), len(tokens), _dev(pos), _dev(ln), _dev(pos2), _dev(ln2))
    return got, logical


TOKEN_CASES = {
    "one_row": ["LINE/L2"],
    "one_token": ["SINE/Alu"] * 700,
    "last_byte": [f"LTR/ERV{c}" for c in "KL1KL1KKL"] * 50,
    "one_byte": list("zAb/AzbZ?") * 30,
    "two_spans_one_spelling": ["LINE/L2", ("LINE", "L2"), "LINE", ("LINE", "L"), "LINE/L", "L2", ("LINE/L2", "x"), ("LINE", "L2/x")] * 9,
    "prefixes": ["LTR", "LTR/", "LTR/ERV", "LT", "LTR/ERV1", "L", "LTR0"] * 3,
    "distinct_16384": [f"fam{(k * 7919) % 16384}" for k in range(16384)] + ["fam5", "fam16383"],
}


@pytest.mark.parametrize("name", list(TOKEN_CASES))
def test_token_ids_equal_the_host_ranks(name):
    got, logical = _ids(TOKEN_CASES[name])
    want_ids, want_names = annotation.family_ranks(logical)
    assert got is not None
    fid, names = got
    assert fid.dtype == torch.int32 and fid.cpu().numpy().tolist() == want_ids.tolist()
    assert [t.decode() for t in names] == want_names
    again, _ = _ids(TOKEN_CASES[name])
    assert again[0].cpu().numpy().tobytes() == fid.cpu().numpy().tobytes() and again[1] == names
    if name == "two_spans_one_spelling":
        ids = fid.cpu().numpy()[:8]
        assert ids[0] == ids[1] and ids[3] == ids[4] and ids[6] == ids[7] and len(set(ids.tolist())) == 5
    if name == "prefixes":
        assert want_names == ["L", "LT", "LTR", "LTR/", "LTR/ERV", "LTR/ERV1", "LTR0"]


def test_token_ids_overflow_writes_nothing_and_refusals(L):
    tokens = [f"fam{k}" for k in range(16385)]
    text, pos, ln, pos2, ln2, _logical = _spell(tokens)
    d_text = _device_text(text)
    d = [_dev(x) for x in (pos, ln, pos2, ln2)]
    d_fid = torch.full((len(tokens),), -77, dtype=torch.int32, device="cuda")
    cap = 1 << 20
    wb = int(L.dgrp_token_ids_workspace_bytes(len(tokens), cap))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    names, off, counts = np.full(cap, 0x5A, np.uint8), np.full(16385, -5, np.int64), (C.c_int64 * 3)()
    call = lambda rows, wb_, cap_=cap: L.dgrp_token_ids(d_text.data_ptr(), len(text), rows, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                        d[3].data_ptr(), d_fid.data_ptr(), names.ctypes.data, cap_, off.ctypes.data, counts,
                                                        work.data_ptr(), wb_, _stream())
    assert call(len(tokens), wb) == 0, last_error()
    torch.cuda.synchronize()
    assert counts[0] == 16385 and counts[1] == 1
    assert bool((d_fid == -77).all()) and (names == 0x5A).all() and (off[1:] == -5).all()
    assert annotation.token_ids_device(d_text, len(text), len(tokens), *d) is None
    assert call(100, int(L.dgrp_token_ids_workspace_bytes(100, cap)) - 1) == ENOMEM and "workspace" in last_error()
    assert call(100, wb, 10) == ENOMEM and counts[2] > 10 and "names" in last_error()
    d[0][7] = len(text) - 2                                             # a span that leaves the text: refused, not read
    assert call(100, wb) == EINVAL and "leaves the text" in last_error()
    torch.cuda.synchronize()
    assert bool((d_fid == -77).all())
    assert call(0, 0) == 0 and counts[0] == 0 and counts[1] == 0


# ================================================================================================ the paint
def _rows_for(o, n, rng, families=9, extra=6, cover=True):
    """Rows around a record of n bases from coordinate o: nested, overlapping, equal, sticking out, wholly outside and empty ones, a
    modelled row over an un-modelled one -> (SEG rows, keys uint32, modelled mask).  A modelled row's label is its key; an
    un-modelled row's label is 0 or a number the model does not take -- the paint does not read it."""
    fam = lambda k: 64 + k % families
    q = [(max(o - 5, 0), o + n + 5, fam(8)),                                 # an un-modelled family under everything
         (o + n // 4, o + n // 2, 2), (o + n // 3, o + n // 3 + max(n // 8, 1), fam(3)),      # a modelled row over an un-modelled one
         (o + n // 2, o + n, fam(1)), (o + n // 2, o + n, fam(0)), (o + n // 2, o + n, fam(5)),   # equal rows of three families
         (o + n // 2 + n // 4, o + n, 4), (o + n // 2 + n // 4, o + n, 3),  # two modelled rows over them, the smaller label wins
         (o + n + 10, o + n + 20, 1), (0, max(o - 1, 0), fam(2)),           # wholly outside
         (o + 1, o + 1, 1), (o + n, o + n, fam(4)), (o, o, 1)]              # empty
    if not cover:
        q = q[1:]                                                            # without the family under everything: bare stretches
    for _ in range(extra):
        a = int(rng.integers(max(o - 3, 0), o + n + 3))
        q.append((a, a + int(rng.integers(0, (n + 4) if cover else max(n // 6, 2))),
                  int(rng.integers(1, 64)) if rng.random() < 0.4 else fam(int(rng.integers(0, families)))))
    order = rng.permutation(len(q))
    rows, keys = np.zeros(len(q), SEG), np.zeros(len(q), np.uint32)
    for i, k in enumerate(order):
        key = q[k][2]
        rows[i] = (q[k][0], q[k][1], key if key < 64 else (0, 9)[i % 2], 0)
        keys[i] = key
    return rows, keys, keys < 64


def _layout(lengths):
    ln = np.asarray(lengths, np.int64)
    off = np.zeros(len(ln) + 1, np.int64)
    np.cumsum(ln, out=off[1:])
    return ln, off


def _row_off(rows):
    ro = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ro[1:])
    return ro


def _paint_keys(L, lengths, origins, rows, keys, fill=0x01010101):
    ln, off = _layout(lengths)
    org, ro = np.asarray(origins, np.int64), _row_off(rows)
    flat = np.concatenate(rows) if ro[-1] else np.zeros(0, SEG)
    d_rows = _dev(flat.view(np.uint8)) if flat.size else None
    d_rk = _dev(np.concatenate(keys).view(np.int32)) if flat.size else None
    wb = int(L.dgrp_eval_workspace_bytes(len(ln), int(ro[-1])))
    work = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
    guard = 16
    track = torch.full((int(off[-1]) + 2 * guard,), fill, dtype=torch.int32, device="cuda")
    rc = L.dgrp_paint_keys_batch(track[guard:].data_ptr(), len(ln), i64ptr(off), i64ptr(ln), i64ptr(org), _ptr(d_rows), i64ptr(ro), _ptr(d_rk),
                                 work.data_ptr(), wb, _stream())
    torch.cuda.synchronize()
    whole = track.cpu().numpy()
    assert (whole[:guard] == fill).all() and (whole[-guard:] == fill).all()
    return rc, whole[guard:-guard].view(np.uint32).copy(), (ln, off, org, ro, d_rows, work, wb)


@pytest.mark.parametrize("lengths", [[1], [8192], [8193], [65, 8193], [64, 1, 8193]], ids=str)
def test_paint_keys_equals_the_statement_and_the_label_paint_below_64(L, lengths):
    rng = np.random.default_rng(sum(lengths))
    origins = [int(rng.integers(0, 5000)) for _ in lengths]
    trip = [_rows_for(o, n, rng) for o, n in zip(origins, lengths)]
    rows, keys = [t[0] for t in trip], [t[1] for t in trip]
    rc, got, (ln, off, org, _ro, _d, work, wb) = _paint_keys(L, lengths, origins, rows, keys)
    assert rc == 0, last_error()
    want = np.concatenate(offtarget.reference_keys(origins, lengths, rows, keys))
    np.testing.assert_array_equal(got, want)
    assert (got != NONE).any() and ((got[got != NONE] >= 64).any() or lengths == [1])
    # key < 64 is the label dgrp_paint_rows_batch paints from the modelled rows alone
    modelled = [t[0][t[2]] for t in trip]
    mo = _row_off(modelled)
    d_m = _dev(np.concatenate(modelled).view(np.uint8))
    d_lab = torch.zeros(int(off[-1]), dtype=torch.int8, device="cuda")
    assert L.dgrp_paint_rows_batch(d_lab.data_ptr(), len(ln), i64ptr(off), i64ptr(ln), i64ptr(org), d_m.data_ptr(), i64ptr(mo), work.data_ptr(), wb,
                                   _stream()) == 0, last_error()
    labels = d_lab.cpu().numpy()
    np.testing.assert_array_equal(np.where(got < 64, got, 0).astype(np.int8), labels)
    # and the strata paint, which shares the body, still states what it stated
    sof = [rng.integers(0, 256, len(m)).astype(np.uint8) for m in modelled]
    d_st = _dev(np.concatenate(sof))
    d_sk = torch.empty(int(off[-1]), dtype=torch.int32, device="cuda")
    assert L.dgrp_paint_strata_batch(d_sk.data_ptr(), len(ln), i64ptr(off), i64ptr(ln), i64ptr(org), d_m.data_ptr(), i64ptr(mo), d_st.data_ptr(),
                                     work.data_ptr(), wb, _stream()) == 0, last_error()
    np.testing.assert_array_equal(d_sk.cpu().numpy().view(np.uint32), np.concatenate(strata.reference_keys(origins, lengths, modelled, sof)))


def test_paint_keys_without_rows_and_a_key_of_any_size(L):
    empty = np.zeros(0, SEG)
    rc, got, _ = _paint_keys(L, [70, 3], [0, 9], [empty, empty], [np.zeros(0, np.uint32)] * 2)
    assert rc == 0 and (got == NONE).all()
    row = np.zeros(2, SEG)
    row[0], row[1] = (5, 60, -3, 0), (20, 30, 1 << 30, 0)                  # labels no other entry would take: they are not read
    rc, got, _ = _paint_keys(L, [70], [0], [row], [np.array([0xFFFFFFFE, 0], np.uint32)])
    assert rc == 0, last_error()
    assert (got[5:20] == 0xFFFFFFFE).all() and (got[20:30] == 0).all() and (got[:5] == NONE).all() and (got[60:] == NONE).all()


@pytest.mark.parametrize("bad", [(5, 9, NONE), (-1, 9, 70), (9, 5, 70)], ids=str)
def test_paint_keys_refuses_a_bad_row_and_leaves_the_track(L, bad):
    rows, keys, _m = _rows_for(0, 500, np.random.default_rng(3))
    rows[len(rows) // 2] = (bad[0], bad[1], 1, 0)
    keys[len(rows) // 2] = bad[2]
    rc, got, _ = _paint_keys(L, [500], [0], [rows], [keys])
    assert rc == EINVAL and "dgrp_paint_keys_batch" in last_error() and "key below 0xFFFFFFFF" in last_error()
    assert (got == 0x01010101).all()


# ================================================================================================ the cross-tabulation
def _runs(rng, n, draw, mean=40):
    """n values in runs (neighbouring bases share their value, as on a genome), some single ones between them"""
    out = np.zeros(n, np.int64)
    i = 0
    while i < n:
        k = 1 if rng.random() < 0.2 else int(rng.integers(1, 2 * mean))
        out[i:i + k] = draw()
        i += k
    return out


def _world(C_, F, n, seed):
    rng = np.random.default_rng(seed)
    pred = _runs(rng, n, lambda: int(rng.integers(0, C_))).astype(np.int8)

    def key():
        u = rng.random()
        if u < 0.3:
            return int(rng.integers(1, C_))
        if u < 0.5:
            return NONE
        return 64 + (int(rng.integers(0, F)) if u < 0.9 else (0, F - 1)[int(rng.integers(0, 2))])
    keys = _runs(rng, n, key).astype(np.uint32)
    return pred, keys


def _crosstab(L, pred, keys, C_, K, stream=None):
    d_pred, d_keys = _dev(pred), _dev(keys.view(np.int32))
    d_hist = torch.full((C_ * K + 2,), -3, dtype=torch.int64, device="cuda")
    d_bad = torch.full((3,), 7, dtype=torch.int32, device="cuda")
    rc = L.dgrp_key_crosstab_batch(d_pred.data_ptr(), d_keys.data_ptr(), len(pred), C_, K, d_hist[1:].data_ptr(), d_bad[1:].data_ptr(),
                                   _stream() if stream is None else stream)
    torch.cuda.synchronize()
    h, b = d_hist.cpu().numpy(), d_bad.cpu().numpy()
    assert h[0] == -3 and h[-1] == -3 and b[0] == 7 and b[2] == 7
    return rc, h[1:-1].reshape(C_, K), int(b[1])


@pytest.mark.parametrize("F", [1, 60, 16384])
@pytest.mark.parametrize("C_", [2, 5, 17])
def test_crosstab_equals_the_statement_and_the_confusion_matrix(L, C_, F):
    n, K = 20_011, 64 + F + 1
    pred, keys = _world(C_, F, n, 100 * C_ + F % 97)
    rc, got, flag = _crosstab(L, pred, keys, C_, K)
    assert rc == 0, last_error()
    want, want_flag = offtarget.reference_crosstab(pred, keys, C_, K)
    np.testing.assert_array_equal(got, want)
    assert flag == want_flag == 0 and got.sum() == n and got[:, 64:-1].sum() > 0 and got[:, -1].sum() > 0
    if F == 16384:
        assert (C_ * K * 4 > 160 * 1024) == (C_ >= 5) and got[:, 64 + F - 1].sum() > 0   # several groups of cells (C >= 5), the last family among them
    truth = np.where(keys < 64, keys, 0).astype(np.int8)
    d_cnf, d_bad = torch.empty((C_, C_), dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    assert L.dgrp_confusion_matrix(_dev(truth).data_ptr(), _dev(pred).data_ptr(), n, C_, d_cnf.data_ptr(), d_bad.data_ptr(), _stream()) == 0
    cnf = d_cnf.cpu().numpy()
    for lab in range(1, C_):
        np.testing.assert_array_equal(got[:, lab], cnf[lab])
    np.testing.assert_array_equal(got[:, 64:].sum(axis=1), cnf[0])
    again = _crosstab(L, pred, keys, C_, K)
    assert again[1].tobytes() == got.tobytes()


def test_crosstab_flags_a_bad_key_or_label_and_does_not_count_it(L):
    C_, F = 5, 60
    K = 64 + F + 1
    pred, keys = _world(C_, F, 9001, 5)
    for spoil in ("key_is_the_none_column", "key_beyond", "label_C", "label_negative"):
        p, k = pred.copy(), keys.copy()
        if spoil == "key_is_the_none_column":
            k[4000] = K - 1
        elif spoil == "key_beyond":
            k[8999] = 0x7FFFFFFF
        elif spoil == "label_C":
            p[17] = C_
        else:
            p[0] = -1
        rc, got, flag = _crosstab(L, p, k, C_, K)
        want, want_flag = offtarget.reference_crosstab(p, k, C_, K)
        assert rc == 0 and flag == want_flag == 1 and got.sum() == 9000, spoil
        np.testing.assert_array_equal(got, want)
    d1 = torch.zeros(1, dtype=torch.int64, device="cuda")
    for C_, K_, n in ((0, K, 5), (65, K, 5), (5, 64, 5), (5, 64 + 16384 + 2, 5), (5, K, -1)):
        assert L.dgrp_key_crosstab_batch(d1.data_ptr(), d1.data_ptr(), n, C_, K_, d1.data_ptr(), d1.data_ptr(), _stream()) == EINVAL
    rc, got, flag = _crosstab(L, pred[:0], keys[:0], 5, K)
    assert rc == 0 and not got.any() and flag == 0


# ================================================================================================ the counts per row
def _pred_rows(o, n, rng, count):
    rows = np.zeros(count + 3, SEG)
    for i in range(count):
        a = int(rng.integers(max(o - 20, 0), o + n))
        rows[i] = (a, a + int(rng.integers(1, max(n // 3, 2))), int(rng.integers(1, 5)), 0)
    rows[count], rows[count + 1], rows[count + 2] = (max(o - 5, 0), o + n + 5, 2, 0), (o + n + 1, o + n + 9, 1, 0), (o, o, 3, 0)
    return rows


@pytest.mark.parametrize("lengths,count", [([1], 2), ([8193], 40), ([65, 8193, 300], 5000)], ids=str)
def test_row_key_classes_against_numpy_and_the_hits(L, lengths, count):
    rng = np.random.default_rng(len(lengths) + count)
    origins = [int(rng.integers(0, 5000)) for _ in lengths]
    trip = [_rows_for(o, n, rng, extra=4, cover=False) for o, n in zip(origins, lengths)]
    rc, track, (ln, off, org, _ro, _d, _w, _wb) = _paint_keys(L, lengths, origins, [t[0] for t in trip], [t[1] for t in trip])
    assert rc == 0, last_error()
    pr = [_pred_rows(o, n, rng, count) for o, n in zip(origins, lengths)]
    po = _row_off(pr)
    flat = np.concatenate(pr)
    d_rows, d_keys = _dev(flat.view(np.uint8)), _dev(track.view(np.int32))
    wb = int(L.dgrp_eval_workspace_bytes(len(ln), len(flat)))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    d_cls = torch.full((len(flat) + 2, 4), -9, dtype=torch.int64, device="cuda")
    assert L.dgrp_row_key_classes_batch(d_keys.data_ptr(), len(ln), i64ptr(off), i64ptr(ln), i64ptr(org), d_rows.data_ptr(), i64ptr(po),
                                        d_cls[1:].data_ptr(), work.data_ptr(), wb, _stream()) == 0, last_error()
    torch.cuda.synchronize()
    whole = d_cls.cpu().numpy()
    assert (whole[0] == -9).all() and (whole[-1] == -9).all()
    got = whole[1:-1]
    want = np.zeros_like(got)
    clen = np.zeros(len(flat), np.int64)
    for r in range(len(ln)):
        for i in range(int(po[r]), int(po[r + 1])):
            a = min(max(int(flat[i]["start"]) - origins[r], 0), lengths[r])
            e = min(max(int(flat[i]["end"]) - origins[r], 0), lengths[r])
            clen[i] = max(e - a, 0)
            want[i] = offtarget.reference_row_classes(track[off[r] + a:off[r] + max(e, a)], int(flat[i]["label"]))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got.sum(axis=1), clen)
    assert (got > 0).any(axis=0).all() or lengths == [1]
    d_lab = _dev(np.where(track < 64, track, 0).astype(np.int8))
    d_hits = torch.zeros(len(flat), dtype=torch.int64, device="cuda")
    assert L.dgrp_row_hits_batch(d_lab.data_ptr(), len(ln), i64ptr(off), i64ptr(ln), i64ptr(org), d_rows.data_ptr(), i64ptr(po), d_hits.data_ptr(),
                                 work.data_ptr(), wb, _stream()) == 0, last_error()
    np.testing.assert_array_equal(got[:, 0], d_hits.cpu().numpy())
    bad = flat.copy()
    bad[1]["label"] = 64
    assert L.dgrp_row_key_classes_batch(d_keys.data_ptr(), len(ln), i64ptr(off), i64ptr(ln), i64ptr(org), _dev(bad.view(np.uint8)).data_ptr(),
                                        i64ptr(po), d_cls[1:].data_ptr(), work.data_ptr(), wb, _stream()) == EINVAL


# ================================================================================================ stream order
@pytest.mark.parametrize("fill", [0xA5, 0x00, 0xFF], ids=lambda f: f"fill{f:02X}")
def test_paint_keys_synchronises_once_and_is_stream_ordered_behind_it(H, L, fill):
    lengths, origins = [65, 8193], [100, 0]
    rng = np.random.default_rng(4)
    trip = [_rows_for(o, n, rng) for o, n in zip(origins, lengths)]
    flat, keys = np.concatenate([t[0] for t in trip]), np.concatenate([t[1] for t in trip])
    p_flat = flat.copy()
    p_flat["start"], p_flat["end"] = 0, 10 ** 6
    ln, off = _layout(lengths)
    org, ro = np.asarray(origins, np.int64), _row_off([t[0] for t in trip])
    wb = int(L.dgrp_eval_workspace_bytes(2, len(flat)))
    call = lambda b, w, s, t: (L.dgrp_paint_keys_batch(b["keys"].data_ptr(), 2, i64ptr(t["off"]), i64ptr(t["ln"]), i64ptr(t["org"]), b["rows"].data_ptr(),
                                                       i64ptr(t["ro"]), b["rk"].data_ptr(), w.data_ptr(), wb, s), None)
    late, *_ = H.run(call, {"rows": (flat.view(np.uint8), p_flat.view(np.uint8)), "rk": (keys.view(np.int32), np.full(len(keys), 77, np.int32) + (keys == 77))},
                     {"keys": np.full(int(off[-1]), 0x01010101, np.int32)}, work_bytes=wb, fill=fill, sync=True, drained=False,
                     tables={"off": off, "ln": ln, "org": org, "ro": ro})
    want = np.concatenate(offtarget.reference_keys(origins, lengths, [t[0] for t in trip], [t[1] for t in trip]))
    np.testing.assert_array_equal(late["keys"].view(np.uint32), want)


def test_crosstab_is_stream_ordered(H, L):
    C_, F = 5, 60
    K = 64 + F + 1
    pred, keys = _world(C_, F, 20_011, 9)
    call = lambda b, w, s, t: (L.dgrp_key_crosstab_batch(b["pred"].data_ptr(), b["keys"].data_ptr(), len(pred), C_, K, b["hist"].data_ptr(),
                                                         b["bad"].data_ptr(), s), None)
    late, *_ = H.run(call, {"pred": (pred, np.where(pred == 1, 2, 1).astype(np.int8)), "keys": (keys.view(np.int32), np.full(len(keys), 64, np.int32) + (keys == 64))},
                     {"hist": np.full((C_, K), -3, np.int64), "bad": np.full(1, 7, np.int32)})
    want, _flag = offtarget.reference_crosstab(pred, keys, C_, K)
    np.testing.assert_array_equal(late["hist"], want)
    assert late["bad"][0] == 0


@pytest.mark.parametrize("fill", [0xA5, 0xFF], ids=lambda f: f"fill{f:02X}")
def test_row_key_classes_synchronises_once_and_is_stream_ordered_behind_it(H, L, fill):
    lengths, origins = [65, 8193], [100, 0]
    rng = np.random.default_rng(6)
    trip = [_rows_for(o, n, rng) for o, n in zip(origins, lengths)]
    track = np.concatenate(offtarget.reference_keys(origins, lengths, [t[0] for t in trip], [t[1] for t in trip]))
    pr = [_pred_rows(o, n, rng, 30) for o, n in zip(origins, lengths)]
    flat = np.concatenate(pr)
    p_flat = flat.copy()
    p_flat["start"], p_flat["end"], p_flat["label"] = 0, 10 ** 6, 1
    ln, off = _layout(lengths)
    org, po = np.asarray(origins, np.int64), _row_off(pr)
    wb = int(L.dgrp_eval_workspace_bytes(2, len(flat)))
    call = lambda b, w, s, t: (L.dgrp_row_key_classes_batch(b["keys"].data_ptr(), 2, i64ptr(t["off"]), i64ptr(t["ln"]), i64ptr(t["org"]), b["rows"].data_ptr(),
                                                            i64ptr(t["po"]), b["cls"].data_ptr(), w.data_ptr(), wb, s), None)
    late, *_ = H.run(call, {"rows": (flat.view(np.uint8), p_flat.view(np.uint8)), "keys": (track.view(np.int32), np.full(len(track), 1, np.int32) + (track == 1))},
                     {"cls": np.full((len(flat), 4), -9, np.int64)}, work_bytes=wb, fill=fill, sync=True, drained=False,
                     tables={"off": off, "ln": ln, "org": org, "po": po})
    assert (late["cls"].sum(axis=1) > 0).any() and (late["cls"][:, 0] > 0).any() and (late["cls"] >= 0).all()
