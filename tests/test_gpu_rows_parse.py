"""dgrp_rows_parse on the GPU against its two statements: evaluation.read_annotation for a table, compare.tsv_flat_host for a TSV --
rows, names, lines and runs must agree exactly -- and its contract: what it does not decide, the first malformed line, the capacity,
the refusals before any launch, the same bytes from two calls, the stream it runs on."""
import ctypes as C

import numpy as np
import pytest

from compare_cases import TILE, boundary_profile, table_text, tsv_text

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EINVAL, ENOMEM = -1, -3
KEYS = ("begin", "end", "number", "name_pos", "name_len", "file_pos", "file_len", "line", "run_first")
POISON = -7


def _dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


def _upload(text: bytes, shift: int = 0):
    """The text in device memory, `shift` bytes behind an aligned address."""
    buf = torch.zeros(shift + max(len(text), 1), dtype=torch.uint8, device=_dev())
    if text:
        buf[shift:shift + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(buf.device)
    return buf[shift:shift + len(text)] if text else buf[:0]


def _poisoned(cap):
    i64 = lambda: torch.full((max(cap, 1) + 8,), POISON, dtype=torch.int64, device=_dev())
    i32 = lambda: torch.full((max(cap, 1) + 8,), POISON, dtype=torch.int32, device=_dev())
    return dict(begin=i64(), end=i64(), number=i64(), name_pos=i64(), name_len=i32(), file_pos=i64(), file_len=i32(), line=i64(), run_first=i64())


def _untouched(out):
    return all(bool((out[k] == POISON).all()) for k in KEYS)


def _parse(text, tsv, cap=None, shift=0):
    from deepgrp_amd.compare import rows_parse_device
    d_text = _upload(text, shift)
    cap = len(text) // 8 + 1 if cap is None else cap
    out = _poisoned(cap)
    counts, out, rc = rows_parse_device(d_text, len(text), tsv, cap, out)
    torch.cuda.synchronize()
    return counts, out, rc, d_text


def _flat(text, tsv, shift=0):
    from deepgrp_amd.compare import flat_of_device_text
    d_text = _upload(text, shift)
    flat, malformed = flat_of_device_text(d_text, len(text), tsv)
    assert flat is not None and malformed is None
    return flat


def _table_lines(text):
    """(lines of the file, [(line, name, begin, end, number)]) by str.split, the grammar of read_annotation."""
    ls = text.decode().replace("\r\n", "\n").split("\n")
    if ls and ls[-1] == "":
        ls.pop()
    rows = []
    for k, l in enumerate(ls, 1):
        f = l.split()
        if f and f[0][0] != "#":
            rows.append((k, f[0], int(f[1]), int(f[2]), int(f[3])))
    return len(ls), rows


def _check_table(tmp_path, text, shift=0):
    from deepgrp_amd.compare import _grouped
    from deepgrp_amd.evaluation import read_annotation
    flat = _flat(text, False, shift)
    nlines, want = _table_lines(text)
    names = np.repeat(np.array(flat.run_names, object), np.diff(flat.run_first)).tolist() if len(want) else []
    got = list(zip(flat.line.tolist(), names, flat.begin.tolist(), flat.end.tolist(), flat.number.tolist()))
    assert flat.lines == nlines and got == want
    runs = [i for i in range(len(want)) if i == 0 or want[i][1] != want[i - 1][1]]
    assert flat.run_first.tolist() == runs + [len(want)]
    p = tmp_path / "t.bed"
    p.write_bytes(text)
    ref = read_annotation(str(p), None)
    rows_of, lines_of = _grouped(str(p), flat, np.ones(len(want), bool))
    assert list(rows_of) == list(ref)
    for name in ref:
        assert rows_of[name].tolist() == ref[name].tolist()
        assert lines_of[name].tolist() == [w[0] for w in want if w[1] == name]
    return flat


def _check_tsv(tmp_path, text, shift=0):
    from deepgrp_amd.compare import tsv_flat_host
    p = tmp_path / "p.tsv"
    p.write_bytes(text)
    want = tsv_flat_host(str(p))
    flat = _flat(text, True, shift)
    for k in ("begin", "end", "number", "line", "run_first"):
        assert getattr(flat, k).tolist() == getattr(want, k).tolist(), k
    assert flat.run_names == want.run_names and flat.run_files == want.run_files and flat.lines == want.lines
    return flat


# ---------------------------------------------------------------- against the statements
@pytest.mark.parametrize("tsv", (False, True), ids=("table", "tsv"))
def test_empty_text(tsv):
    counts, out, rc, _t = _parse(b"", tsv)
    assert rc == 0 and counts == [0] * 6 and _untouched(out)


@pytest.mark.parametrize("text", [b"chr1 5 9 2", b"chr1 5 9 2\n", b"chr1\t5\t9\t2\r\n", b"\n", b"# only a comment", b"  chr1   5\t9  2   x y z\n"])
def test_one_table_line(tmp_path, text):
    _check_table(tmp_path, text)


@pytest.mark.parametrize("text", [b"g.fa\tchr1 x\t5\t9\t2", b"g.fa\tchr1 x\t5\t9\t2\n", b"g.fa\tchr1\tx\ty\t5\t9\t2\r\n", b"\n", b"d/chrA.fa.npz\th\t5\t9\t2\n",
                                  b"\t\t5\t9\t2\n"])
def test_one_tsv_line(tmp_path, text):
    _check_tsv(tmp_path, text)


@pytest.mark.parametrize("seed,shift", [(0, 0), (1, 3), (2, 0)])
def test_seeded_table_of_three_tiles(tmp_path, seed, shift):
    text = table_text(seed)
    on_chunk, on_tile, straddle = boundary_profile(text)
    assert len(text) > 3 * TILE and on_chunk > 100 and on_tile >= 1 and straddle >= 1
    flat = _check_table(tmp_path, text, shift)
    assert len(flat.begin) > 1000 and len(flat.run_names) > 20 and int(flat.begin.max()) >= 10 ** 17 and flat.route == "device"


@pytest.mark.parametrize("seed,shift", [(0, 0), (1, 5), (2, 0)])
def test_seeded_tsv_of_three_tiles(tmp_path, seed, shift):
    text = tsv_text(seed)
    on_chunk, on_tile, straddle = boundary_profile(text)
    assert len(text) > 3 * TILE and on_chunk > 100 and on_tile >= 1 and straddle >= 1
    flat = _check_tsv(tmp_path, text, shift)
    assert len(flat.begin) > 1000 and {"chr1", "chrA", "chrB", ""} <= set(flat.run_names) and int(flat.begin.max()) >= 10 ** 17


# ---------------------------------------------------------------- not decided
TRIGGERS = {"19 digits": b"1234567890123456789", "sign": b"-5", "underscore": b"1_000", "plus": b"+5", "letters": b"12a"}


@pytest.mark.parametrize("tsv", (False, True), ids=("table", "tsv"))
@pytest.mark.parametrize("what", sorted(TRIGGERS))
@pytest.mark.parametrize("column", (1, 2, 3))
def test_a_number_that_is_not_plain_is_not_decided(tsv, what, column):
    cols = [b"7", b"9", b"2"]
    cols[column - 1] = TRIGGERS[what]
    good = b"g.fa\tchr1\t1\t2\t3\n" if tsv else b"chr1 1 2 3\n"
    line = (b"g.fa\tchr1 h\t" + b"\t".join(cols) if tsv else b"chr1 " + b" ".join(cols)) + b"\n"
    counts, out, rc, _t = _parse(good * 40 + line + good * 3, tsv)
    assert rc == 0 and counts[3] == 1 and counts[2] == 0 and counts[4] == 0 and _untouched(out)


@pytest.mark.parametrize("tsv", (False, True), ids=("table", "tsv"))
@pytest.mark.parametrize("what,junk", [("0x80", b"\x80"), ("lone CR", b"\rX"), ("CR at the end", b"\r"), ("NUL", b"\x00"), ("DEL", b"\x7f"),
                                        ("vertical tab", b"\x0b")])
def test_a_byte_that_is_not_plain_is_not_decided(tsv, what, junk):
    good = b"g.fa\tchr1\t1\t2\t3\n" if tsv else b"chr1 1 2 3\n"
    text = good * 40 + (b"g.fa\tchr1 h" + junk + b"\t7\t9\t2" if tsv else b"chr1 7 9 2 x" + junk) + (b"" if what == "CR at the end" else b"\n" + good)
    counts, out, rc, _t = _parse(text, tsv)
    assert rc == 0 and counts[3] == 1 and counts[2] == 0 and _untouched(out)


def test_crlf_is_plain(tmp_path):
    _check_table(tmp_path, b"chr1 1 2 3\r\nchr2 4 5 1\r\n")
    _check_tsv(tmp_path, b"g.fa\tchr1\t1\t2\t3\r\n\r\ng.fa\tchr2\t4\t5\t1\r\n")


# ---------------------------------------------------------------- malformed lines
def test_short_line_is_reported_with_its_line_and_reason():
    counts, out, rc, _t = _parse(b"chr1 1 2 3\n# c\nchr1 1 2\nchr1 1\n", False)
    assert rc == 0 and counts[3] == 0 and counts[4:] == [3, 1] and counts[2] == 0 and _untouched(out)
    counts, out, rc, _t = _parse(b"g.fa\th\t1\t2\t3\n\ng.fa\t1\t2\t3\nx\n", True)
    assert rc == 0 and counts[3] == 0 and counts[4:] == [3, 2] and _untouched(out)
    # in the third tile, behind lines of every kind: the line is counted over the tiles in front
    for tsv, text, bad in ((False, table_text(0), b"chr9 77 88\n"), (True, tsv_text(0), b"chr9\t77\t88\t1\n")):
        cut = text.index(b"\n", 2 * TILE + 5000) + 1
        cut2 = text.index(b"\n", cut + 3000) + 1
        mixed = text[:cut] + bad + text[cut:cut2] + bad + text[cut2:]
        want = mixed[:cut].replace(b"\r\n", b"\n").count(b"\n") + 1
        counts, out, rc, _t = _parse(mixed, tsv)
        assert rc == 0 and counts[3] == 0 and counts[4:] == [want, 2 if tsv else 1] and _untouched(out)


# ---------------------------------------------------------------- capacity, determinism, refusals
@pytest.mark.parametrize("tsv", (False, True), ids=("table", "tsv"))
def test_capacity_one_too_small(tsv):
    text = tsv_text(0) if tsv else table_text(0)
    counts, out, rc, _t = _parse(text, tsv)
    need = counts[1]
    assert rc == 0 and need > 1000 and not _untouched(out)
    assert bool((out["begin"][need:] == POISON).all()) and bool((out["run_first"][counts[2]:] == POISON).all())   # nothing behind the rows
    counts2, out2, rc2, _t = _parse(text, tsv, cap=need - 1)
    assert rc2 == ENOMEM and counts2[1] == need and counts2[2] == 0 and _untouched(out2)
    from deepgrp_amd._lib import lib
    assert f"{need} rows for a capacity of {need - 1}" in lib().dgrp_last_error().decode()
    counts3, out3, rc3, _t = _parse(text, tsv, cap=need)
    assert rc3 == 0 and counts3 == counts
    for k in KEYS:
        assert torch.equal(out3[k][:need], out[k][:need]), k


@pytest.mark.parametrize("tsv", (False, True), ids=("table", "tsv"))
def test_two_calls_give_the_same_bytes(tsv):
    text = tsv_text(2) if tsv else table_text(2)
    a, b = _parse(text, tsv), _parse(text, tsv)
    assert a[0] == b[0] and a[2] == b[2] == 0
    for k in KEYS:
        assert torch.equal(a[1][k], b[1][k]), k


def test_refusals_before_any_launch():
    from deepgrp_amd._lib import lib
    from deepgrp_amd.pipeline import stream_ptr
    L = lib()
    text = b"chr1 1 2 3\n" * 50
    d_text = _upload(text)
    n, cap = len(text), 64
    wb = int(L.dgrp_rows_parse_workspace_bytes(n))
    assert wb > 0 and L.dgrp_rows_parse_workspace_bytes(-1) == 0
    work = torch.full((wb + 256,), 0x5A, dtype=torch.uint8, device=_dev())

    def call(text_ptr=d_text.data_ptr(), size=n, fmt=0, null=None, counts="own", work_ptr=work.data_ptr(), work_bytes=wb, cap=cap):
        out = _poisoned(cap)
        c = (C.c_int64 * 6)(*([99] * 6))
        ptrs = [None if k == null else out[k].data_ptr() for k in KEYS]
        rc = L.dgrp_rows_parse(text_ptr, size, fmt, *ptrs, cap, c if counts == "own" else None, work_ptr, work_bytes, stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 or _untouched(out)
        return rc, list(c)

    assert call()[0] == 0
    assert call(text_ptr=None) == (EINVAL, [0] * 6)
    assert call(size=-1) == (EINVAL, [0] * 6)
    assert call(fmt=2)[0] == EINVAL and call(fmt=-1)[0] == EINVAL
    assert call(cap=-1)[0] == EINVAL
    assert call(counts=None)[0] == EINVAL
    for k in ("begin", "end", "number", "name_pos", "name_len", "line", "run_first"):
        assert call(null=k)[0] == EINVAL, k
    assert call(null="file_pos")[0] == 0                               # a table has no file field
    assert call(fmt=1, null="file_pos")[0] == EINVAL and call(fmt=1, null="file_len")[0] == EINVAL
    assert call(work_ptr=None)[0] == EINVAL and call(work_ptr=work.data_ptr() + 8)[0] == EINVAL
    assert call(work_bytes=wb - 1)[0] == ENOMEM
    assert bool((work == 0x5A).all().item()) is False                  # (the good calls used it)
    fresh = torch.full((wb,), 0x5A, dtype=torch.uint8, device=_dev())
    assert call(work_ptr=fresh.data_ptr(), work_bytes=wb - 1)[0] == ENOMEM and bool((fresh == 0x5A).all())
    assert call(text_ptr=None, size=0) == (0, [0] * 6)


# ---------------------------------------------------------------- the stream contract
@pytest.fixture(scope="module")
def harness():
    from deepgrp_amd._lib import lib
    from stream_harness import Harness
    H = Harness(_dev())
    H.choose_side(lib())
    return H


@pytest.mark.parametrize("tsv", (False, True), ids=("table", "tsv"))
@pytest.mark.parametrize("fill", (0xA5, 0x00, 0xFF))
def test_runs_on_the_callers_stream_and_synchronises_it(harness, tsv, fill):
    """The late producer of tests/test_gpu_streams.py: the text arrives on a side stream behind a delay; a launch or copy on another
    stream would read the poison text (one malformed line: no rows).  The workspace arrives filled with `fill`."""
    from deepgrp_amd._lib import lib
    L, H = lib(), harness
    text = (tsv_text(1) if tsv else table_text(1))[:TILE + 3000]
    text = text[:text.rindex(b"\n") + 1]
    real = np.frombuffer(text, np.uint8).copy()
    n, cap = len(text), len(text) // 8 + 1
    wb = int(L.dgrp_rows_parse_workspace_bytes(n))
    seen = []

    def call(b, wk, st, _t):
        c = (C.c_int64 * 6)()
        rc = L.dgrp_rows_parse(b["text"].data_ptr(), n, 1 if tsv else 0, *(b[k].data_ptr() for k in KEYS), cap, c, wk.data_ptr(), wb, st)
        seen.append(list(c))
        return rc, list(c)
    sent = {k: np.full(cap, POISON, np.int32 if k.endswith("_len") else np.int64) for k in KEYS}
    late, late_counts, _idle, idle_counts = H.run(call, {"text": (real, np.full(n, ord("x"), np.uint8))}, sent, work_bytes=wb, fill=fill, sync=True,
                                                 drained=True)
    flat = _flat(text, tsv)
    assert late_counts == idle_counts and late_counts[1] == len(flat.begin) > 100 and late_counts[3:] == [0, 0, 0]
    assert late["begin"][:late_counts[1]].tolist() == flat.begin.tolist() and late["line"][:late_counts[1]].tolist() == flat.line.tolist()
    assert late["run_first"][:late_counts[2]].tolist() == flat.run_first[:-1].tolist()
