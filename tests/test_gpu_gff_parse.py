"""dgrp_gff_parse on the GPU against its statement, gffin.features_host, on every case of the corpus -- counts, arrays, runs and the
end of the features E must agree exactly -- and its contract: what it does not decide, the first malformed line, the capacity, the
refusals before any launch, the same bytes from two calls, unaligned text, the stream it runs on."""
import ctypes as C

import numpy as np
import pytest

from gff_in_cases import CASES, KEY, NAMES4, TILE, UNDECIDED, many_names

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EINVAL, ENOMEM = -1, -3
KEYS = ("begin", "end", "number", "name_pos", "name_len", "line", "run_first")
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
    return dict(begin=i64(), end=i64(), number=i64(), name_pos=i64(), name_len=torch.full((max(cap, 1) + 8,), POISON, dtype=torch.int32, device=_dev()),
                line=i64(), run_first=i64())


def _untouched(out):
    return all(bool((out[k] == POISON).all()) for k in KEYS)


def _parse(case, cap=None, shift=0):
    from deepgrp_amd.gffin import gff_parse_device
    d_text = _upload(case.text, shift)
    cap = len(case.text) // 11 + 1 if cap is None else cap
    out = _poisoned(cap)
    counts, out, rc = gff_parse_device(d_text, len(case.text), case.names, case.key, cap, out)
    torch.cuda.synchronize()
    return counts, out, rc, d_text


# ---------------------------------------------------------------- against the statement
@pytest.mark.parametrize("shift", (0, 3))
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_entry_against_the_statement(tmp_path, name, shift):
    from deepgrp_amd import gffin
    case = CASES[name]
    counts, out, rc, d_text = _parse(case, shift=shift)
    assert rc == 0
    if case.want == UNDECIDED:
        assert counts[3] == 1 and counts[2] == 0 and counts[4:6] == [0, 0] and _untouched(out)
        return
    if case.want[0] == "malformed":
        assert counts[3] == 0 and counts[4:6] == [case.want[1], 3] and counts[2] == 0 and _untouched(out)
        return
    p = tmp_path / "x.gff3"
    p.write_bytes(case.text)
    want, want_end = gffin.features_of_bytes(str(p), case.text, case.names, case.key)
    rows, runs = len(want.begin), len(want.run_names)
    assert counts == [want.lines, rows, runs, 0, 0, 0, want_end] and want_end == case.want[1] and rows == len(case.want[2])
    for k in ("begin", "end", "number", "line"):
        assert out[k][:rows].cpu().tolist() == getattr(want, k).tolist(), k
        assert bool((out[k][rows:] == POISON).all()), k                      # nothing behind the rows
    assert out["run_first"][:runs].cpu().tolist() == want.run_first[:-1].tolist() and bool((out["run_first"][runs:] == POISON).all())
    pos, ln = out["name_pos"][:rows].cpu().tolist(), out["name_len"][:rows].cpu().tolist()
    assert [case.text[a:a + b] for a, b in zip(pos, ln)] == [r[1] for r in case.want[2]]
    # the wrapper: the same Flat, names decoded, route "device"
    flat, malformed, end_at = gffin.features_device(d_text, len(case.text), case.names, case.key)
    assert malformed is None and end_at == want_end and flat.route == "device" and flat.run_names == want.run_names and flat.lines == want.lines
    for k in ("begin", "end", "number", "line", "run_first"):
        assert getattr(flat, k).tolist() == getattr(want, k).tolist(), k


def test_malformed_line_in_the_third_tile():
    case = CASES["bulk"]
    cut = case.text.index(b"\n", 2 * TILE + 5000) + 1
    cut2 = case.text.index(b"\n", cut + 3000) + 1
    text = case.text[:cut] + b"chr9\tx\ty\t1\t2\t.\t.\t.\n" + case.text[cut:cut2] + b"short\n" + case.text[cut2:]
    counts, out, rc, _t = _parse(case._replace(text=text))
    assert rc == 0 and counts[3] == 0 and counts[4:6] == [case.text[:cut].count(b"\n") + 1, 3] and counts[2] == 0 and _untouched(out)
    # behind E a short line is no line at all
    text = case.text[:cut] + b"##FASTA\n" + b"short\n" + case.text[cut:]
    counts, out, rc, _t = _parse(case._replace(text=text))
    in_front = case.text[:cut].count(b"\n")
    assert rc == 0 and counts[3:] == [0, 0, 0, cut] and counts[0] == in_front
    assert counts[1] == sum(1 for r in case.want[2] if r[0] <= in_front) > 900
    # and a byte the device does not decide raises no flag there
    counts2, _out, rc, _t = _parse(case._replace(text=text + b"\n\xff\x00\r\n"))
    assert rc == 0 and counts2 == counts


def test_read_features_raises_on_both_routes(tmp_path):
    from deepgrp_amd import gffin
    from deepgrp_amd.evaluation import AnnotationError
    for name, line, why in (("eight fields", 3, gffin.REASON), ("start 0", 1, "negative begin"), ("end below begin", 1, "end below begin")):
        p = tmp_path / "x.gff3"
        p.write_bytes(CASES[name].text)
        said = []
        for device in (True, False):
            with pytest.raises(AnnotationError) as e:
                gffin.read_features(str(p), NAMES4, KEY, device=device)
            said.append(str(e.value))
        assert said[0] == said[1] and said[0].startswith(f"{p}:{line}: {why}: '")
    for name in ("bulk", "19 digits", "size 0", "escaped seqid"):                        # device, host (not decided), empty
        p = tmp_path / "y.gff3"
        p.write_bytes(CASES[name].text)
        a, b = gffin.read_features(str(p), NAMES4, KEY), gffin.read_features(str(p), NAMES4, KEY, device=False)
        assert a.route == ("host" if name == "19 digits" else "device") and b.route == "host"
        assert a.run_names == b.run_names and a.lines == b.lines
        for k in ("begin", "end", "number", "line", "run_first"):
            assert getattr(a, k).tolist() == getattr(b, k).tolist(), (name, k)
    got = gffin.read_annotation(str(p), NAMES4, KEY, [3])
    assert list(got) == ["chr|3"] and len(got["chr|3"]) == 3 and got.route == "device"


# ---------------------------------------------------------------- capacity, determinism, refusals
def test_capacity_one_too_small():
    case = CASES["bulk"]
    counts, out, rc, _t = _parse(case)
    need = counts[1]
    assert rc == 0 and need == len(case.want[2]) and not _untouched(out)
    counts2, out2, rc2, _t = _parse(case, cap=need - 1)
    assert rc2 == ENOMEM and counts2[1] == need and counts2[2] == 0 and _untouched(out2)
    from deepgrp_amd._lib import lib
    assert f"{need} rows for a capacity of {need - 1}" in lib().dgrp_last_error().decode()
    counts3, out3, rc3, _t = _parse(case, cap=need)
    assert rc3 == 0 and counts3 == counts
    for k in KEYS:
        assert torch.equal(out3[k][:need], out[k][:need]), k


def test_the_row_bound_holds_for_the_shortest_lines():
    """Lines of 11 bytes: n / 11 + 1 rows, and 12 of them start in one lane's 128 bytes."""
    from gff_in_cases import Case
    text = b"\t\t\t1\t2\t\t\t\t\n" * 3000 + b"\t\t\t1\t2\t\t\t\t"
    counts, out, rc, _t = _parse(Case(text, NAMES4, KEY, None))
    assert rc == 0 and counts[:4] == [3001, 3001, 1, 0] and 3001 == len(text) // 11 + 1
    assert out["line"][:3001].cpu().tolist() == list(range(1, 3002)) and out["name_pos"][:3001].cpu().tolist() == list(range(0, 11 * 3001, 11))


def test_two_calls_give_the_same_bytes():
    a, b = _parse(CASES["bulk"]), _parse(CASES["bulk"])
    assert a[0] == b[0] and a[2] == b[2] == 0
    for k in KEYS:
        assert torch.equal(a[1][k], b[1][k]), k


def test_refusals_before_any_launch():
    from deepgrp_amd import gffin
    from deepgrp_amd._lib import lib
    from deepgrp_amd.pipeline import stream_ptr
    L = lib()
    text = CASES["size 129"].text * 8
    d_text = _upload(text)
    n, cap = len(text), 128
    wb = int(L.dgrp_gff_parse_workspace_bytes(n))
    assert wb > 0 and L.dgrp_gff_parse_workspace_bytes(-1) == 0
    work = torch.full((wb + 256,), 0x5A, dtype=torch.uint8, device=_dev())
    blob, off, number, count = gffin.names_table(NAMES4)
    d_blob, d_off, d_number = (torch.from_numpy(a).to(_dev()) for a in (blob, off, number))
    d_key = torch.from_numpy(np.frombuffer(KEY, np.uint8).copy()).to(_dev())
    table = dict(names=d_blob.data_ptr(), off=d_off.data_ptr(), number=d_number.data_ptr())

    def call(text_ptr=d_text.data_ptr(), size=n, null=None, nnames=count, key_ptr=d_key.data_ptr(), key_len=len(KEY), counts="own",
             work_ptr=work.data_ptr(), work_bytes=wb, cap=cap):
        out = _poisoned(cap)
        c = (C.c_int64 * 7)(*([99] * 7))
        ptrs = [None if k == null else out[k].data_ptr() for k in KEYS]
        tab = [None if k == null else table[k] for k in ("names", "off", "number")]
        rc = L.dgrp_gff_parse(text_ptr, size, *tab, nnames, key_ptr, key_len, *ptrs, cap, c if counts == "own" else None, work_ptr,
                              work_bytes, stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 or _untouched(out)
        return rc, list(c)

    fresh = torch.full((wb,), 0x5A, dtype=torch.uint8, device=_dev())
    unused = dict(work_ptr=fresh.data_ptr())
    assert call(text_ptr=None, **unused) == (EINVAL, [0] * 7)
    assert call(size=-1, **unused) == (EINVAL, [0] * 7)
    assert call(cap=-1, **unused)[0] == EINVAL and call(counts=None, **unused)[0] == EINVAL
    for k in KEYS + ("names", "off", "number"):
        assert call(null=k, **unused)[0] == EINVAL, k
    assert call(nnames=4097, **unused)[0] == EINVAL and call(nnames=-1, **unused)[0] == EINVAL
    assert call(key_ptr=None, **unused)[0] == EINVAL and call(key_len=256, **unused)[0] == EINVAL and call(key_len=-1, **unused)[0] == EINVAL
    assert call(work_ptr=None)[0] == EINVAL and call(work_ptr=fresh.data_ptr() + 8)[0] == EINVAL
    assert call(work_bytes=wb - 1, **unused)[0] == ENOMEM
    assert bool((fresh == 0x5A).all())                                 # no refusal touched the workspace
    assert call(text_ptr=None, size=0, **unused) == (0, [0] * 7) and bool((fresh == 0x5A).all())
    rc, counts = call()
    assert rc == 0 and counts[1] == 8 * len(CASES["size 129"].want[2]) and bool((work[:wb] == 0x5A).all().item()) is False
    # an empty table and the type column need no pointers
    rc, counts0 = call(null="names", nnames=0)
    assert rc == 0 and counts0 == counts
    assert call(key_ptr=None, key_len=0)[0] == 0


def test_4096_alternatives_on_many_rows():
    from gff_in_cases import Case, feature
    names = many_names()
    picks = [0, 1, 40, 400, 4095, 4096, 2047, 999]
    text = b"".join(feature(attrs=b"Name=fam%d" % k) + b"\n" for k in picks * 50)
    counts, out, rc, _t = _parse(Case(text, names, KEY, None))
    assert rc == 0 and counts[1] == 400
    assert out["number"][:400].cpu().tolist() == [0 if k >= 4096 else k % 4 + 1 for k in picks] * 50


# ---------------------------------------------------------------- the stream contract
@pytest.fixture(scope="module")
def harness():
    from deepgrp_amd._lib import lib
    from stream_harness import Harness
    H = Harness(_dev())
    H.choose_side(lib())
    return H


@pytest.mark.parametrize("fill", (0xA5, 0x00, 0xFF))
def test_runs_on_the_callers_stream_and_synchronises_it(harness, fill):
    """The late producer of tests/test_gpu_streams.py: the text arrives on a side stream behind a delay; a launch or copy on another
    stream would read the poison text (one malformed line: no rows).  The workspace arrives filled with `fill`."""
    from deepgrp_amd import gffin
    from deepgrp_amd._lib import lib
    L, H = lib(), harness
    case = CASES["##FASTA inside a chunk"]._replace(text=CASES["bulk"].text[:TILE + 3000])
    text = case.text[:case.text.rindex(b"\n") + 1] + b"##FASTA\n>chr1\nACGT\n"
    real = np.frombuffer(text, np.uint8).copy()
    n, cap = len(text), len(text) // 11 + 1
    wb = int(L.dgrp_gff_parse_workspace_bytes(n))
    blob, off, number, count = gffin.names_table(NAMES4)
    d_blob, d_off, d_number = (torch.from_numpy(a).to(_dev()) for a in (blob, off, number))
    d_key = torch.from_numpy(np.frombuffer(KEY, np.uint8).copy()).to(_dev())
    torch.cuda.synchronize()

    def call(b, wk, st, _t):
        c = (C.c_int64 * 7)()
        rc = L.dgrp_gff_parse(b["text"].data_ptr(), n, d_blob.data_ptr(), d_off.data_ptr(), d_number.data_ptr(), count, d_key.data_ptr(), len(KEY),
                              *(b[k].data_ptr() for k in KEYS), cap, c, wk.data_ptr(), wb, st)
        return rc, list(c)
    sent = {k: np.full(cap, POISON, np.int32 if k.endswith("_len") else np.int64) for k in KEYS}
    late, late_counts, _idle, idle_counts = H.run(call, {"text": (real, np.full(n, ord("x"), np.uint8))}, sent, work_bytes=wb, fill=fill, sync=True,
                                                 drained=True)
    want, want_end = gffin.features_of_bytes("x", text, NAMES4, KEY)
    rows = len(want.begin)
    assert late_counts == idle_counts == [want.lines, rows, len(want.run_names), 0, 0, 0, want_end] and rows > 300 and want_end == n - 19
    for k in ("begin", "end", "number", "line"):
        assert late[k][:rows].tolist() == getattr(want, k).tolist(), k
    assert late["run_first"][:late_counts[2]].tolist() == want.run_first[:-1].tolist()
