"""dgrp_rm_parse and deepgrp_amd/annotation.py on the GPU: for every case of the corpus (tests/rm_cases.py) the device's rows, line
numbers and contig grouping equal those of _scripts/parse_rm.read_repeatmasker on the same text; files that are not plain raise the
flag and are still read, by the host path; the call is reproducible and respects its capacity; the reference's fixture pair through
the gzip path."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import rm_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from deepgrp_amd import annotation  # noqa: E402

CASES = rm_cases.cases(annotation.TILE_BYTES)
FALLBACK = rm_cases.fallback_cases()
ENOMEM = -3
_WANT = {}


def _want(name, data):
    """The port's rows of a case, computed once."""
    if name not in _WANT:
        _WANT[name] = rm_cases.port_rows(data)
    return _WANT[name]


def _device(data, offset=0):
    """The text on the device, `offset` bytes behind an aligned address."""
    buf = torch.empty(len(data) + offset, dtype=torch.uint8, device="cuda")
    if data:
        buf[offset:] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return buf[offset:]


def _flat(listing):
    """[(contig, begin, end, number, line)] of a Listing, file order."""
    names = np.repeat(np.arange(len(listing.run_names)), np.diff(listing.run_first))
    return [(listing.run_names[c], int(b), int(e), int(n), int(ln))
            for c, b, e, n, ln in zip(names, listing.begin, listing.end, listing.number, listing.line)]


@pytest.mark.parametrize("name,data", CASES, ids=[c[0] for c in CASES])
def test_device_rows_equal_the_ports(name, data):
    want = _want(name, data)
    d_text = _device(data)
    listing = annotation.listing_of_device_text("<case>", d_text, len(data))
    assert listing is not None, "the not-plain flag on a plain file"
    got = _flat(listing)
    assert len(got) == len(want)
    assert got == want
    assert listing.lines == len(data.decode().split("\n")) - (1 if data.endswith(b"\n") or not data else 0)
    # runs: maximal stretches of one name
    names = [w[0] for w in want]
    first = [i for i in range(len(names)) if i == 0 or names[i] != names[i - 1]]
    assert listing.run_first.tolist() == first + [len(names)] and listing.run_names == [names[i] for i in first]
    # the grouping is the table's
    rows = listing.grouped(listing.table_mask())
    grouped = rm_cases.grouped(want)
    assert sorted(rows[0]) == sorted(grouped)
    for ctg, exp in grouped.items():
        assert [tuple(int(x) for x in (r["start"], r["end"], r["label"])) for r in rows[0][ctg]] == [e[:3] for e in exp]
        assert rows[1][ctg].tolist() == [e[3] for e in exp]


@pytest.mark.parametrize("offset", [1, 7, 16])
def test_text_at_any_alignment(offset):
    name, data = next(c for c in CASES if c[0] == "two_tiles_plus_1")
    listing = annotation.listing_of_device_text("<case>", _device(data, offset), len(data))
    assert _flat(listing) == _want(name, data)


@pytest.mark.parametrize("name,data", FALLBACK, ids=[c[0] for c in FALLBACK])
def test_files_that_are_not_plain_go_to_the_host(tmp_path, name, data):
    counts, _out, rc = annotation.parse_device(_device(data))
    assert rc == 0 and counts[3] == 1
    p = tmp_path / "l.out"
    p.write_bytes(data)
    got = annotation.read_rows(str(p), fmt="repeatmasker")
    assert got.route == "host"
    want = rm_cases.grouped(rm_cases.port_rows(data))
    assert sorted(got) == sorted(want)
    for ctg, exp in want.items():
        assert [tuple(int(x) for x in (r["start"], r["end"], r["label"])) for r in got[ctg]] == [e[:3] for e in exp]
        assert got.lines[ctg].tolist() == [e[3] for e in exp]


def test_the_flag_is_found_anywhere_in_a_large_file():
    name, data = CASES[[c[0] for c in CASES].index("generated_40000")]
    for at in (0, annotation.TILE_BYTES - 1, len(data) // 2, len(data) - 1):
        bad = bytearray(data)
        bad[at] = 0x0b
        assert annotation.parse_device(_device(bytes(bad)))[0][3] == 1, at


def test_the_same_call_gives_the_same_bytes():
    name, data = CASES[[c[0] for c in CASES].index("generated_40000")]
    d_text = _device(data)
    runs = []
    for _ in range(2):
        counts, out, rc = annotation.parse_device(d_text)
        assert rc == 0
        kept, nruns = counts[1], counts[2]
        runs.append((counts, [out[k][:nruns if k == "run_first" else kept].cpu().numpy().tobytes() for k in sorted(out)]))
    assert runs[0] == runs[1] and runs[0][0][1] == len(_want(name, data))


def test_a_capacity_one_below_the_need_writes_nothing_and_reports_the_need():
    name, data = next(c for c in CASES if c[0] == "alternating_300")
    from deepgrp_amd._lib import lib
    d_text = _device(data)
    counts, out, rc = annotation.parse_device(d_text, cap=300)
    assert rc == 0 and counts[1] == 300 and counts[2] == 300
    # guarded arrays of 299 rows
    import ctypes as C
    from deepgrp_amd.pipeline import stream_ptr
    L = lib()
    d_names, d_off, d_pent, nnames, unit = annotation._device_tables(d_text.device)
    guard, cap = 64, 299
    arrs = {k: torch.full((cap + guard,), -77, dtype=(torch.int32 if k in ("number", "name_len") else torch.int64), device="cuda")
            for k in ("begin", "end", "number", "name_pos", "name_len", "line", "run_first")}
    wb = int(L.dgrp_rm_parse_workspace_bytes(len(data)))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    c4 = (C.c_int64 * 4)()
    rc = L.dgrp_rm_parse(d_text.data_ptr(), len(data), d_names.data_ptr(), d_off.data_ptr(), nnames, d_pent.data_ptr(), unit,
                         *(arrs[k].data_ptr() for k in ("begin", "end", "number", "name_pos", "name_len", "line", "run_first")), cap, c4,
                         work.data_ptr(), wb, stream_ptr())
    torch.cuda.synchronize()
    assert rc == ENOMEM and c4[1] == 300 and c4[3] == 0
    assert "300 rows for a capacity of 299" in L.dgrp_last_error().decode()
    for k, a in arrs.items():
        assert bool((a == -77).all()), k


def test_the_golden_listing_through_the_gzip_path_equals_the_golden_table():
    from deepgrp_amd.evaluation import read_annotation
    got = annotation.read_rows(os.path.join(GOLDEN, "parse_rm_input.out.gz"))
    want = read_annotation(os.path.join(GOLDEN, "parse_rm_expect.bed"), None)
    assert got.route == "device" and sorted(got) == sorted(want)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes()


def test_plain_and_bgzf_files_give_the_same_listing(tmp_path):
    from deepgrp_amd import gz
    name, data = CASES[[c[0] for c in CASES].index("generated_40000")]
    plain, packed = tmp_path / "g.out", tmp_path / "g.out.gz"
    plain.write_bytes(data)
    packed.write_bytes(gz.bgzf_compress(data))
    a, b = annotation.read_listing(str(plain)), annotation.read_listing(str(packed))
    assert a.route == b.route == "device"
    assert _flat(a) == _flat(b) == _want(name, data)
    empty = tmp_path / "e.out"
    empty.write_bytes(b"")
    assert len(annotation.read_listing(str(empty))) == 0 and annotation.read_rows(str(empty), fmt="repeatmasker") == {}
