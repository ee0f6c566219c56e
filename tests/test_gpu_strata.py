"""The three device entries of `evaluate --strata`, each against its Python statement and the entry it stands beside:
dgrp_rm_parse_fields (annotation.millidiv_of_line; dgrp_rm_parse byte for byte), dgrp_paint_strata_batch (strata.reference_keys;
dgrp_paint_rows_batch on every covered base) and dgrp_prob_hist_strata_batch (strata.reference_strata_hist; dgrp_prob_hist_batch
summed over strata).  Every count is an integer: equal means equal."""
import ctypes as C
import io

import numpy as np
import pytest

import rm_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from bed_device import Arena                                           # noqa: E402
from deepgrp_amd import annotation, strata                              # noqa: E402
from stream_harness import SEG, Harness, i64ptr, last_error             # noqa: E402

EINVAL, ENOMEM = -1, -3
NONE = 0xFFFFFFFF
PAD = np.float32(0.75)
ROW_KEYS = ("begin", "end", "number", "name_pos", "name_len", "line", "run_first")


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


# ================================================================================================ the parser
TOKENS = ["10.5", "0.0", "7", "7.", "12.34", ".5", "-1.0", "1e1", "1234567.0", "999999.9", "123456", "0", "00.09", "1..2", "1.2.3", "12.3x",
          "x", "+5", "5%", "1,5", ".", "30.", "000001.999"]


def _token_text():
    lines = rm_cases.HEADER.rstrip("\n").split("\n") + [""]
    for k, tok in enumerate(TOKENS):
        lines.append(rm_cases.out_line(begin=100 * k + 1, end=100 * k + 60, fam=rm_cases.FAMILIES[k % 10], lead=" " * (k % 5)).replace("10.5", tok, 1))
        f = rm_cases.rmsk_line(start=100 * k, end=100 * k + 60).split("\t")
        f[2] = ("1" * (k % 9 + 1))                                      # 1 .. 9 digits: 8 and 9 are too many
        lines.append("\t".join(f))
    return rm_cases.text(lines)


def _straddle(edge, back, token):
    """A listing whose last line's divergence token starts `back` bytes in front of byte `edge` (and ends behind it)."""
    probe = rm_cases.out_line(ctg="chrS", begin=5, end=60).replace("10.5", token, 1)
    at = probe.index(token)
    data = rm_cases.sized_text(edge - back - at) + (probe + "\n").encode("ascii")
    start = edge - back
    assert data[start:start + len(token)] == token.encode() and start < edge < start + len(token)
    return data


PARSER_CASES = (rm_cases.cases(annotation.TILE_BYTES) + [("generated_4000", rm_cases.generated(4000)), ("tokens", _token_text())]
                + [(f"chunk_edge_back{b}", _straddle(128 * 301, b, "123.45")) for b in (1, 3, 5)]
                + [(f"tile_edge_back{b}", _straddle(annotation.TILE_BYTES, b, "123.45")) for b in (1, 3, 5)]
                + [("tile_edge_point", _straddle(2 * annotation.TILE_BYTES, 2, "17.9")), ("chunk_edge_bad", _straddle(128 * 7, 2, "1e+01"))])


def _device_text(data):
    buf = torch.empty(max(len(data), 1), dtype=torch.uint8, device="cuda")
    if data:
        buf[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf[:len(data)]


def _host(out, counts):
    kept, runs = counts[1], counts[2]
    return {k: v[:runs if k == "run_first" else kept].cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name,data", PARSER_CASES, ids=[c[0] for c in PARSER_CASES])
def test_fields_entry_equals_the_old_entry_and_the_python_rule(name, data):
    d_text = _device_text(data)
    c_old, o_old, rc_old = annotation.parse_device(d_text, len(data))
    c_new, o_new, rc_new = annotation.parse_device(d_text, len(data), fields=True)
    assert rc_old == rc_new == 0 and c_old == c_new and c_new[3] == 0
    old, new = _host(o_old, c_old), _host(o_new, c_new)
    for k in ROW_KEYS:
        assert old[k].tobytes() == new[k].tobytes(), k
    lines = io.StringIO(data.decode("ascii"), newline=None).read().split("\n")
    want = [annotation.millidiv_of_line(lines[int(ln) - 1]) for ln in new["line"]]
    assert new["millidiv"].dtype == np.int32 and new["millidiv"].tolist() == want
    assert len(want) == len(rm_cases.port_rows(data))
    if name == "tokens":
        assert want[0::2] == [105, 0, 70, 70, 123, -1, -1, -1, -1, 9999999, 1234560, 0, 0, -1, -1, -1, -1, -1, -1, -1, -1, 300, 19]
        assert want[1::2] == [int("1" * (k % 9 + 1)) if k % 9 + 1 <= 7 else -1 for k in range(len(TOKENS))]
    if name.startswith(("chunk_edge_", "tile_edge_")):
        assert want[-1] == {"123.45": 1234, "17.9": 179, "1e+01": -1}[lines[int(new["line"][-1]) - 1].split()[1]]


def test_the_same_call_gives_the_same_bytes_and_listings_carry_millidiv():
    data = dict(PARSER_CASES)["generated_4000"]
    d_text = _device_text(data)
    a = annotation.parse_device(d_text, len(data), fields=True)
    b = annotation.parse_device(d_text, len(data), fields=True)
    assert a[0] == b[0] and all(x.tobytes() == y.tobytes() for x, y in zip(_host(a[1], a[0]).values(), _host(b[1], b[0]).values()))
    listing = annotation.listing_of_device_text("<case>", d_text, len(data))
    assert listing.route == "device" and listing.millidiv.tobytes() == _host(a[1], a[0])["millidiv"].tobytes()
    assert set(listing.millidiv.tolist()) == {105, 13}
    rows, lines, div = listing.grouped_fields(listing.table_mask())
    assert sorted(div) == sorted(rows) and all(len(div[k]) == len(rows[k]) == len(lines[k]) for k in rows)


@pytest.mark.parametrize("name,data", rm_cases.fallback_cases(), ids=[c[0] for c in rm_cases.fallback_cases()])
def test_the_not_plain_flag_as_in_the_old_entry(tmp_path, name, data):
    d_text = _device_text(data)
    c_old, _o, rc_old = annotation.parse_device(d_text, len(data))
    c_new, _o, rc_new = annotation.parse_device(d_text, len(data), fields=True)
    assert rc_old == rc_new == 0 and c_old == c_new and c_new[3] == 1
    p = tmp_path / "l.out"
    p.write_bytes(data)
    got = annotation.read_listing(str(p))
    assert got.route == "host" and got.millidiv.tolist() == [105] * len(got)


def test_a_capacity_one_below_the_need_writes_nothing_and_reports_the_need(L):
    data = dict(PARSER_CASES)["alternating_300"]
    d_text = _device_text(data)
    d_names, d_off, d_pent, nnames, unit = annotation._device_tables(d_text.device)
    guard, cap = 64, 299
    arrs = {k: torch.full((cap + guard,), -77, dtype=(torch.int32 if k in ("number", "name_len", "millidiv") else torch.int64), device="cuda")
            for k in ROW_KEYS + ("millidiv",)}
    wb = int(L.dgrp_rm_parse_workspace_bytes(len(data)))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    c4 = (C.c_int64 * 4)()
    args = lambda cap_, wb_, div: (d_text.data_ptr(), len(data), d_names.data_ptr(), d_off.data_ptr(), nnames, d_pent.data_ptr(), unit,
                                   *(arrs[k].data_ptr() for k in ROW_KEYS), div, cap_, c4, work.data_ptr(), wb_, _stream())
    rc = L.dgrp_rm_parse_fields(*args(cap, wb, arrs["millidiv"].data_ptr()))
    torch.cuda.synchronize()
    assert rc == ENOMEM and c4[1] == 300 and c4[3] == 0
    assert "300 rows for a capacity of 299" in last_error() and "dgrp_rm_parse_fields" in last_error()
    assert L.dgrp_rm_parse_fields(*args(300, wb - 1, arrs["millidiv"].data_ptr())) == ENOMEM and "workspace" in last_error()
    assert L.dgrp_rm_parse_fields(*args(300, wb, None)) == EINVAL and "NULL output" in last_error()
    torch.cuda.synchronize()
    for k, a in arrs.items():
        assert bool((a == -77).all()), k


# ================================================================================================ the paint
def _rows_for(o, n, rng, extra=6):
    """Rows around a record of n bases from coordinate o: nested, overlapping, equal, sticking out at both ends, wholly outside and
    empty ones, then `extra` random ones -> (SEG rows, strata)."""
    q = [(max(o - 5, 0), o + n + 5, 5, 9),                                 # sticks out at both ends
         (o + n // 4, o + n // 2, 2, 7), (o + n // 3, o + n // 3 + max(n // 8, 1), 2, 3),      # nested in the first, overlapping each other
         (o + n // 2, o + n, 4, 1), (o + n // 2, o + n, 4, 0), (o + n // 2, o + n, 4, 200),   # equal rows of one label, three strata
         (o + n // 2, o + n, 3, 255),                                      # and a smaller label over them
         (o + n + 10, o + n + 20, 1, 0), (0, max(o - 1, 0), 1, 0),         # wholly outside
         (o + 1, o + 1, 1, 0), (o + n, o + n, 1, 0), (o, o, 1, 0)]         # empty
    for _ in range(extra):
        a = int(rng.integers(max(o - 3, 0), o + n + 3))
        q.append((a, a + int(rng.integers(0, n + 4)), int(rng.integers(1, 64)), int(rng.integers(0, 256))))
    order = rng.permutation(len(q))
    rows = np.zeros(len(q), SEG)
    for i, k in enumerate(order):
        rows[i] = (q[k][0], q[k][1], q[k][2], 0)
    return rows, np.array([q[k][3] for k in order], np.uint8)


def _paint(L, lengths, origins, rows, sof, lead=7, gap=3, short_work=0, stream=None):
    """One dgrp_paint_strata_batch on records laid out with `lead` foreign keys in front and `gap` between them.
    -> (rc, the whole track uint32, off [nrec + 1], the arenas, the label track of dgrp_paint_rows_batch)."""
    ln, org = np.asarray(lengths, np.int64), np.asarray(origins, np.int64)
    nrec = len(ln)
    off = np.zeros(nrec + 1, np.int64)
    off[:nrec] = lead + np.cumsum(np.r_[0, ln[:-1] + gap]) if nrec else 0
    off[nrec] = (off[nrec - 1] + ln[-1] + gap) if nrec else lead
    ro = np.zeros(nrec + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ro[1:])
    flat = np.concatenate(rows) if ro[-1] else np.zeros(0, SEG)
    st = np.concatenate(sof) if ro[-1] else np.zeros(0, np.uint8)
    d_rows = torch.from_numpy(flat.view(np.uint8).copy()).cuda() if flat.size else None
    d_st = torch.from_numpy(st.copy()).cuda() if st.size else None
    wb = int(L.dgrp_eval_workspace_bytes(nrec, int(ro[-1]))) - short_work
    track, work = Arena(int(off[nrec]) * 4), Arena(max(wb, 1))
    ptr = lambda t: None if t is None else t.data_ptr()
    s = _stream() if stream is None else stream
    rc = L.dgrp_paint_strata_batch(track.ptr, nrec, i64ptr(off), i64ptr(ln), i64ptr(org), ptr(d_rows), i64ptr(ro), ptr(d_st), work.ptr, wb, s)
    torch.cuda.synchronize()
    labels = None
    if rc == 0 and nrec:
        d_lab = torch.zeros(int(off[nrec]), dtype=torch.int8, device="cuda")
        wk = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
        assert L.dgrp_paint_rows_batch(d_lab.data_ptr(), nrec, i64ptr(off), i64ptr(ln), i64ptr(org), ptr(d_rows), i64ptr(ro), wk.data_ptr(),
                                       wb, s) == 0, last_error()
        torch.cuda.synchronize()
        labels = d_lab.cpu().numpy()
    return rc, track.body().cpu().numpy().view(np.uint32).copy(), off, (track, work), labels


def _check_paint(L, lengths, origins, rows, sof):
    rc, got, off, arenas, labels = _paint(L, lengths, origins, rows, sof)
    assert rc == 0, last_error()
    want = np.full(int(off[-1]), NONE, np.uint32)                        # every element is written: the gaps are "no row" too
    for r, key in enumerate(strata.reference_keys(origins, lengths, rows, sof)):
        want[off[r]:off[r] + lengths[r]] = key
    np.testing.assert_array_equal(got, want)
    covered = got != NONE
    np.testing.assert_array_equal((got[covered] >> 8).astype(np.int8), labels[covered])
    assert not labels[~covered].any()
    assert all(a.guards_intact() for a in arenas)
    return got


@pytest.mark.parametrize("lengths", [[1], [63], [64], [65], [8193], [65, 8193], [64, 1, 8193]], ids=str)
def test_paint_equals_the_statement(L, lengths):
    rng = np.random.default_rng(sum(lengths))
    origins = [int(rng.integers(0, 5000)) for _ in lengths]
    pairs = [_rows_for(o, n, rng) for o, n in zip(origins, lengths)]
    got = _check_paint(L, lengths, origins, [p[0] for p in pairs], [p[1] for p in pairs])
    assert (got != NONE).any()


def test_paint_one_long_row_and_the_lowest_stratum_of_a_label(L):
    n = 100_000
    rows = np.zeros(1, SEG)
    rows[0] = (0, n, 63, 0)
    got = _check_paint(L, [n], [0], [rows], [np.array([255], np.uint8)])
    assert (got[7:7 + n] == (63 << 8 | 255)).all()
    two = np.zeros(3, SEG)
    two[0], two[1], two[2] = (10, 90, 2, 0), (10, 90, 2, 0), (40, 60, 3, 0)
    got = _check_paint(L, [100], [0], [two], [np.array([9, 4, 0], np.uint8)])
    assert (got[7 + 10:7 + 90] == (2 << 8 | 4)).all() and (got[7:7 + 10] == NONE).all()


def test_paint_without_rows_gives_no_row_everywhere(L):
    empty = np.zeros(0, SEG)
    for lengths, rows in (([70], [empty]), ([5, 300], [empty, empty]), ([5, 300], [empty, _rows_for(0, 300, np.random.default_rng(1))[0]])):
        sof = [np.zeros(len(r), np.uint8) for r in rows]
        got = _check_paint(L, lengths, [0] * len(lengths), rows, sof)
        assert (got[7:7 + lengths[0]] == NONE).all()
    only_outside = np.zeros(1, SEG)
    only_outside[0] = (500, 600, 1, 0)
    assert (_check_paint(L, [100], [0], [only_outside], [np.zeros(1, np.uint8)]) == NONE).all()


@pytest.mark.parametrize("bad", [(5, 9, 0), (5, 9, 64), (5, 9, -1), (-1, 9, 1), (9, 5, 1)], ids=str)
def test_paint_refuses_a_bad_row_and_leaves_the_track(L, bad):
    rows, sof = _rows_for(0, 500, np.random.default_rng(3))
    rows[len(rows) // 2] = (bad[0], bad[1], bad[2], 0)
    rc, _got, _off, arenas, _lab = _paint(L, [500], [0], [rows], [sof])
    assert rc == EINVAL and "dgrp_paint_strata_batch" in last_error() and "1 <= label <= 63" in last_error()
    assert arenas[0].untouched()


def test_paint_refusals_before_device_work(L):
    rows, sof = _rows_for(0, 500, np.random.default_rng(3))
    rc, _got, _off, arenas, _lab = _paint(L, [500], [0], [rows], [sof], short_work=1)
    assert rc == ENOMEM and arenas[0].untouched() and arenas[1].untouched()
    ln, org, ro = np.array([500], np.int64), np.zeros(1, np.int64), np.array([0, len(rows)], np.int64)
    track = Arena(400 * 4)
    for off in (np.array([0, 400], np.int64), np.array([-1, 600], np.int64), np.array([200, 100], np.int64)):     # the record does not lie in the track
        assert L.dgrp_paint_strata_batch(track.ptr, 1, i64ptr(off), i64ptr(ln), i64ptr(org), 0x10000, i64ptr(ro), 0x10000, 0x10000, 1 << 30,
                                         _stream()) == EINVAL, off
    torch.cuda.synchronize()
    assert track.untouched()


# ================================================================================================ the histogram
HIST_LENGTHS = [4097, 0, 63, 1000]


def _tenths():
    t = (np.arange(1, 11, dtype=np.float64) / 10).astype(np.float32)
    return np.nextafter(t, np.float32(0))


def _hist_world(C, S, seed, flagged=True):
    """Keys and probabilities of HIST_LENGTHS: about 70 % of the bases annotated in runs (as elements are), labels 1 .. C-1, every
    stratum; at the true class of the first annotated bases the values of the issue, a NaN and 1.5 among them when `flagged`."""
    rng = np.random.default_rng(seed)
    n = sum(HIST_LENGTHS)
    keys = np.full(n, NONE, np.uint32)
    at = 0
    while at < n:
        run = int(rng.integers(1, 200))
        if rng.random() < 0.7:
            keys[at:at + run] = int(rng.integers(1, C)) << 8 | int(rng.integers(0, S))
        at += run
    keys[:S] = (np.uint32(1 + (np.arange(S) % (C - 1))) << np.uint32(8)) | np.arange(S, dtype=np.uint32)      # every stratum is there
    values = rng.random((n, C), dtype=np.float32)
    live = np.flatnonzero(keys != NONE)
    special = [0.0, 1.0, -0.0] + list(_tenths()) + ([np.nan, 1.5] if flagged else [])
    for b, v in zip(live[S + 5::3], special):                             # (behind the bases that make every stratum present)
        values[b, keys[b] >> 8] = v
    return keys, values


def _hist_layout(values, keys, lead=5):
    ln = np.asarray(HIST_LENGTHS, np.int64)
    row0 = np.zeros(len(ln), np.int64)
    np.cumsum((ln[:-1] + 63) // 64 * 64 + 1, out=row0[1:])                  # (+ 1: records start off the 16-byte grid too)
    probs = np.full((int(row0[-1] + ln[-1]) + 1, values.shape[1]), PAD, np.float32)
    off = (lead + np.r_[0, np.cumsum(ln)[:-1]]).astype(np.int64)
    at = 0
    for r, m in enumerate(ln):
        probs[row0[r]:row0[r] + m] = values[at:at + m]
        at += int(m)
    kbuf = np.concatenate([np.full(lead, 3 << 8, np.uint32), keys, np.full(4, 3 << 8, np.uint32)])
    return probs, row0, ln, kbuf, off


def _hist(L, dev, probs, row0, ln, kbuf, off, S, bins, arenas=None, short_work=0):
    C_ = probs.shape[1]
    d_probs, d_keys = torch.from_numpy(probs).to(dev), torch.from_numpy(kbuf.view(np.int32)).to(dev)
    wb = int(L.dgrp_prob_hist_strata_workspace_bytes(len(ln)))
    assert wb > 0
    hist, work = arenas or (Arena(C_ * S * bins * 8), Arena(wb))
    d_bad = torch.full((3,), 7, dtype=torch.int32, device=dev)
    rc = L.dgrp_prob_hist_strata_batch(d_probs.data_ptr(), C_, len(ln), i64ptr(row0), i64ptr(ln), d_keys.data_ptr(), i64ptr(off), S, bins,
                                       hist.ptr, d_bad[1:].data_ptr(), work.ptr, wb - short_work, _stream())
    torch.cuda.current_stream().synchronize()
    bad = d_bad.cpu().numpy()
    assert bad[0] == 7 and bad[2] == 7
    return rc, hist.body().cpu().numpy().view(np.int64).reshape(C_, S, bins).copy(), int(bad[1]), (hist, work)


@pytest.mark.parametrize("bins", [2, 100, 1000])
@pytest.mark.parametrize("S", [1, 40, 256])
@pytest.mark.parametrize("C_", [2, 5, 17])
def test_hist_equals_the_statement_and_the_old_entry_summed_over_strata(L, dev, C_, S, bins):
    keys, values = _hist_world(C_, S, 100 * C_ + S)
    want, flag = strata.reference_strata_hist(values, keys, S, bins)
    assert flag == 1 and want.sum() == (keys != NONE).sum() - 2
    assert (want.sum(axis=(0, 2)) > 0).all() and not want[0].any()
    layout = _hist_layout(values, keys)
    rc, got, bad, arenas = _hist(L, dev, *layout, S, bins)
    assert rc == 0, last_error()
    assert bad == 1
    np.testing.assert_array_equal(got, want)
    rc2, again, bad2, _ = _hist(L, dev, *layout, S, bins, arenas=arenas)     # the entry zeroes the histogram itself
    assert rc2 == 0 and bad2 == 1 and again.tobytes() == got.tobytes()
    assert all(a.guards_intact() for a in arenas)
    # dgrp_prob_hist_batch on the same records and the truth these keys state
    probs, row0, ln, kbuf, off = layout
    truth = np.where(kbuf == NONE, 0, kbuf >> 8).astype(np.int8)
    d_probs, d_truth = torch.from_numpy(probs).to(dev), torch.from_numpy(truth).to(dev)
    wb = int(L.dgrp_prob_hist_workspace_bytes(len(ln), C_, bins))
    d_old = torch.empty((C_, 2, bins), dtype=torch.int64, device=dev)
    d_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    assert L.dgrp_prob_hist_batch(d_probs.data_ptr(), C_, len(ln), i64ptr(row0), i64ptr(ln), d_truth.data_ptr(), i64ptr(off), bins,
                                  d_old.data_ptr(), d_bad.data_ptr(), work.data_ptr(), wb, _stream()) == 0, last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.sum(axis=1)[1:], d_old.cpu().numpy()[1:, 1])


def test_hist_flags_a_class_or_a_stratum_outside_the_table(L, dev):
    C_, S, bins = 5, 40, 100
    keys, values = _hist_world(C_, S, 77, flagged=False)
    want, flag = strata.reference_strata_hist(values, keys, S, bins)
    rc, got, bad, _ = _hist(L, dev, *_hist_layout(values, keys), S, bins)
    assert rc == 0 and bad == flag == 0
    np.testing.assert_array_equal(got, want)
    live = np.flatnonzero(keys != NONE)
    for key in (C_ << 8, 63 << 8 | 3, 1 << 8 | S, 2 << 8 | 255, 0xFFFFFFFE):
        k2 = keys.copy()
        k2[live[100]] = key
        want, flag = strata.reference_strata_hist(values, k2, S, bins)
        rc, got, bad, _ = _hist(L, dev, *_hist_layout(values, k2), S, bins)
        assert rc == 0 and bad == flag == 1 and got.sum() == live.size - 1
        np.testing.assert_array_equal(got, want)
    k0 = keys.copy()
    k0[live[100]] = 0 << 8 | 7                                           # class 0 is a class: counted where the statement counts it
    want, flag = strata.reference_strata_hist(values, k0, S, bins)
    rc, got, bad, _ = _hist(L, dev, *_hist_layout(values, k0), S, bins)
    assert bad == flag == 0 and got[0, 7].sum() == 1
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("change,code", [(dict(C_=0), EINVAL), (dict(C_=65), EINVAL), (dict(S=0), EINVAL), (dict(S=257), EINVAL),
                                         (dict(bins=1), EINVAL), (dict(bins=1001), EINVAL), (dict(nrec=-1), EINVAL), (dict(hist=0), EINVAL),
                                         (dict(hist_shift=4), EINVAL), (dict(neg=True), EINVAL), (dict(probs=0), EINVAL), (dict(keys=0), EINVAL),
                                         (dict(short=1), ENOMEM)], ids=str)
def test_hist_refusals_come_before_device_work(L, dev, change, code):
    C_, S, bins = 5, 6, 10
    keys, values = _hist_world(C_, S, 5, flagged=False)
    probs, row0, ln, kbuf, off = _hist_layout(values, keys)
    d_probs, d_keys = torch.from_numpy(probs).to(dev), torch.from_numpy(kbuf.view(np.int32)).to(dev)
    wb = int(L.dgrp_prob_hist_strata_workspace_bytes(len(ln)))
    hist, work = Arena(C_ * S * bins * 8 + 8), Arena(wb)
    d_bad = torch.full((1,), 7, dtype=torch.int32, device=dev)
    if change.get("neg"):
        ln = ln.copy()
        ln[2] = -1
    rc = L.dgrp_prob_hist_strata_batch(change.get("probs", d_probs.data_ptr()), change.get("C_", C_), change.get("nrec", len(ln)), i64ptr(row0),
                                       i64ptr(ln), change.get("keys", d_keys.data_ptr()), i64ptr(off), change.get("S", S), change.get("bins", bins),
                                       change.get("hist", hist.ptr + change.get("hist_shift", 0)), d_bad.data_ptr(), work.ptr,
                                       wb - change.get("short", 0), _stream())
    torch.cuda.synchronize()
    assert rc == code and "dgrp_prob_hist_strata_batch" in last_error()
    assert hist.untouched() and work.untouched() and int(d_bad.item()) == 7
    assert L.dgrp_prob_hist_strata_workspace_bytes(-1) == 0


def test_hist_with_nothing_to_count_gives_zeros_without_device_arrays(L, dev):
    C_, S, bins = 5, 6, 10
    hist = Arena(C_ * S * bins * 8)
    d_bad = torch.full((1,), 7, dtype=torch.int32, device=dev)
    assert L.dgrp_prob_hist_strata_batch(None, C_, 0, None, None, None, None, S, bins, hist.ptr, d_bad.data_ptr(), None, 0, _stream()) == 0, last_error()
    torch.cuda.synchronize()
    assert not hist.body().any() and int(d_bad.item()) == 0 and hist.guards_intact()
    hist.body().fill_(0xA5)
    d_bad.fill_(7)
    z = np.zeros(3, np.int64)
    assert L.dgrp_prob_hist_strata_batch(None, C_, 3, i64ptr(z), i64ptr(z), None, i64ptr(z), S, bins, hist.ptr, d_bad.data_ptr(), None, 0,
                                         _stream()) == 0, last_error()
    torch.cuda.synchronize()
    assert not hist.body().any() and int(d_bad.item()) == 0 and hist.guards_intact()


# ================================================================================================ stream order
@pytest.mark.parametrize("fill", [0xA5, 0x00, 0xFF], ids=lambda f: f"fill{f:02X}")
def test_hist_is_stream_ordered(H, L, fill):
    C_, S, bins = 5, 40, 100
    keys, values = _hist_world(C_, S, 11, flagged=False)
    probs, row0, ln, kbuf, off = _hist_layout(values, keys)
    p_probs = np.full_like(probs, 0.5)
    p_keys = np.full_like(kbuf, 1 << 8)
    wb = int(L.dgrp_prob_hist_strata_workspace_bytes(len(ln)))
    call = lambda b, w, s, t: (L.dgrp_prob_hist_strata_batch(b["probs"].data_ptr(), C_, len(ln), i64ptr(t["row0"]), i64ptr(t["ln"]), b["keys"].data_ptr(),
                                                             i64ptr(t["off"]), S, bins, b["hist"].data_ptr(), b["bad"].data_ptr(), w.data_ptr(), wb, s), None)
    late, *_ = H.run(call, {"probs": (probs, p_probs), "keys": (kbuf.view(np.int32), p_keys.view(np.int32))},
                     {"hist": np.full((C_, S, bins), -3, np.int64), "bad": np.full(1, 7, np.int32)}, work_bytes=wb, fill=fill,
                     tables={"row0": row0, "ln": ln, "off": off})
    want, flag = strata.reference_strata_hist(values, keys, S, bins)
    np.testing.assert_array_equal(late["hist"], want)
    assert late["bad"][0] == flag == 0


@pytest.mark.parametrize("fill", [0xA5, 0x00, 0xFF], ids=lambda f: f"fill{f:02X}")
def test_paint_synchronises_once_and_is_stream_ordered_behind_it(H, L, fill):
    lengths, origins = [65, 8193], [100, 0]
    rng = np.random.default_rng(4)
    pairs = [_rows_for(o, n, rng) for o, n in zip(origins, lengths)]
    flat, st = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    p_flat = flat.copy()
    p_flat["start"], p_flat["end"], p_flat["label"] = 0, 10 ** 6, 1
    ln, org = np.asarray(lengths, np.int64), np.asarray(origins, np.int64)
    off = np.array([0, 65, 65 + 8193], np.int64)
    ro = np.array([0, len(pairs[0][0]), len(flat)], np.int64)
    wb = int(L.dgrp_eval_workspace_bytes(2, len(flat)))
    call = lambda b, w, s, t: (L.dgrp_paint_strata_batch(b["keys"].data_ptr(), 2, i64ptr(t["off"]), i64ptr(t["ln"]), i64ptr(t["org"]), b["rows"].data_ptr(),
                                                         i64ptr(t["ro"]), b["st"].data_ptr(), w.data_ptr(), wb, s), None)
    late, *_ = H.run(call, {"rows": (flat.view(np.uint8), p_flat.view(np.uint8)), "st": (st, np.full_like(st, 77) + (st == 77))},
                     {"keys": np.full(int(off[-1]), 0x01010101, np.int32)}, work_bytes=wb, fill=fill, sync=True, drained=False,
                     tables={"off": off, "ln": ln, "org": org, "ro": ro})
    want = np.concatenate(strata.reference_keys(origins, lengths, [p[0] for p in pairs], [p[1] for p in pairs]))
    np.testing.assert_array_equal(late["keys"].view(np.uint32), want)
