"""The corpus of fasta_edge_cases.py held to the reference -- not to the kernels it is for.  Every hand-written plain flag is the
one the package's host rule gives; where it is 1, the reference's own line loop over the text-mode lines of the record yields what
`reference` says, down to the class indices; where a body has an empty line, that loop raises.  And the corpus is where it claims
to be: features on both sides of and across both tile edges, large records on both sides of a full round of the carry loop, chunk
starts in both sweeps and in the scalar tail."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_edge_cases as fc                          # noqa: E402

from deepgrp_amd.fasta import _text_lines              # noqa: E402


def _loop(orc, body: bytes):
    return orc.read_multi_fasta(_text_lines(b">h\n" + body))


def _hold(orc, case):
    plain, total, startpos, kept, idx = fc.reference(case.body)
    assert plain == case.plain, case.name
    seq = case.body.translate(None, b"\r\n")
    assert total == len(seq) and idx.size == total
    if case.plain:
        assert not case.blank
        assert _loop(orc, case.body) == [("h", seq.upper().decode("ascii"))], case.name
        assert orc.strip_n(seq.upper()) == (startpos, kept), case.name
        np.testing.assert_array_equal(orc.encode_idx(seq.upper()), idx, case.name)
        np.testing.assert_array_equal(orc.encode_idx(seq), idx, case.name)               # (the lookup takes either case)
    if case.blank:
        assert not case.plain
        with pytest.raises(IndexError):
            _loop(orc, case.body)


@pytest.mark.parametrize("name", list(fc.FEATURES))
def test_edge_bodies_have_the_flag_written_by_hand(orc, name):
    feat, plain = fc.FEATURES[name]
    cases = fc.edge_bodies(name)
    assert len(cases) == 2 * (len(feat) + 3)
    for case in cases:
        assert len(case.body) == fc.EDGE_BODY and case.body[case.at:case.at + len(feat)] == feat and case.plain == plain
        lfs = [p for p in range(fc.LINE - 1, case.at - 2, fc.LINE)]                  # lines in front; two letters before the feature
        assert [i for i, c in enumerate(case.body[:case.at]) if c == 10] == lfs and len(lfs) >= 32
        assert not set(case.body[case.at + len(feat):]) - set(fc.ALPHABET)
        _hold(orc, case)


def test_ends_lengths_and_n_bodies_have_the_flag_written_by_hand(orc):
    ends = {c.name: c for c in fc.end_bodies()}
    assert [ends[f"ends_{t}"].plain for t in ("cr", "crlf", "lf", "none", "lflf")] == [0, 1, 1, 1, 0]
    assert all(len(ends[f"ends_{t}"].body) == fc.TILE for t in ("cr", "crlf", "lf", "none", "lflf"))
    assert [ends[f"opens_{t}"].plain for t in ("lf", "crlf", "cr")] == [0, 0, 0]
    assert sorted(len(c.body) for c in ends.values() if c.name.startswith("len")) == [1, 2047, 2048, 2049, 4095, 4096, 4097]
    for case in list(ends.values()) + fc.n_bodies():
        _hold(orc, case)


def test_n_bodies_say_what_they_plant():
    by = {c.name: fc.reference(c.body) for c in fc.n_bodies()}
    T = fc.N_TOTAL
    assert T >= 3 * fc.TILE
    for tag in ("oneline", "crlf"):
        for k in fc.N_PLANTS + (T - 1,):
            assert by[f"n_{tag}_one@{k}"][:4] == (1, T, k, 1)
        assert by[f"n_{tag}_two"][:4] == (1, T, 1000, T - 100 - 1000 + 1)              # tile 0 and tile 3: tiles 1 and 2 are all N
        assert 1000 < fc.TILE and T - 100 >= 3 * fc.TILE
        assert by[f"n_{tag}_two_edges"][:4] == (1, T, fc.TILE - 1, 2 * fc.TILE + 2)
        assert by[f"n_{tag}_none"][:4] == (1, T, T, -T)
    assert by["n_single_N"][:4] == (1, 1, 1, -1) == by["n_single_n"][:4] and by["n_single_A"][:4] == (1, 1, 0, 1)
    assert fc.reference(b"")[:4] == (1, 0, 0, 0)
    for c in fc.n_bodies():
        if "oneline" in c.name:
            assert len(c.body) == T and not set(c.body) & {10, 13}
        elif "crlf" in c.name:
            assert c.body.count(b"\r\n") == c.body.count(b"\n") == c.body.count(b"\r") == -(-T // 60)
        if "_none" in c.name:
            assert {78, 110} == set(c.body) - {10, 13}                                # mixed case


def test_boundary_profile():
    """Every feature of two or more bytes lies wholly in front of, across and wholly behind each of the two tile edges.  A feature
    of one byte cannot lie across an edge; it must be the last byte of the tile and the first of the next.  Every feature with a CR
    or LF has a case whose look-ahead leaves the tile."""
    prof = fc.boundary_profile(fc.matrix())
    assert sorted(prof) == sorted(fc.FEATURES)
    for name, (feat, _plain) in fc.FEATURES.items():
        for edge in fc.EDGES:
            before, straddle, behind, flush, ahead = prof[name][edge]
            assert before >= 2 and behind >= 2 and flush == 2, (name, edge)
            assert straddle == len(feat) - 1, (name, edge)                            # every split
            if set(feat) & {10, 13}:
                assert ahead >= 1, (name, edge)
    assert all(fc.position(c, e) == "straddle" for c in fc.edge_bodies("crlf") for e in fc.EDGES if c.at == e - 1)


def test_mixed_batch_is_where_it_claims_to_be(orc):
    b = fc.mixed_batch()
    assert b.len.tolist()[:7] == [0, 1, fc.SMALL - 1, fc.SMALL, fc.SMALL + 1, 3 * fc.SMALL // 2, 0] and b.len[-2:].tolist() == [5000, 0]
    assert 6_000_000 < len(b.text) < 8_000_000
    large = [int(n) for n in b.len if n > fc.SMALL]
    assert len(large) == 4
    assert any(fc.ntiles(n) % 256 == 0 for n in large) and any(fc.ntiles(n) % 256 == 1 for n in large)
    assert fc.ntiles(fc.SMALL + 1) == 513 and fc.ntiles(3 * fc.SMALL // 2) == 768
    assert {int(o) % 2 for o in b.off} == {0, 1}
    assert b.bodies[3] == b.bodies[2] + b"A" and b.bodies[4] == b.bodies[2] + b"AN"
    for r, body in enumerate(b.bodies):
        o = int(b.off[r])
        assert b.text[o:o + len(body)] == body and b.text[:o].endswith(b">" + b.names[r].encode() + b"\n")
        assert o + len(body) == len(b.text) or b.text[o + len(body):].lstrip(b"\n")[:1] == b">"
        assert fc.reference(body)[0] == b.plain[r], r
    spoiled = b.bodies[7]
    odd = [i for i, c in enumerate(spoiled) if c <= 32 and c != 10]
    assert len(odd) == 1 and spoiled[odd[0]] == 32 and odd[0] // fc.TILE == fc.ntiles(len(spoiled)) - 1
    assert b.bodies[8].count(b"\r\n") == b.bodies[8].count(b"\n") > 10_000
    # the whole text through the reference's loop: the records `reference` states, the spoiled one among them (strip() of its
    # lines leaves the inner space in place)
    want = orc.read_multi_fasta(_text_lines(b.text))
    assert [h for h, _s in want] == b.names
    for r, (_h, s) in enumerate(want):
        if b.plain[r]:
            _plain, total, startpos, kept, idx = fc.reference(b.bodies[r])
            assert len(s) == total and orc.strip_n(s.encode()) == (startpos, kept), r
            np.testing.assert_array_equal(orc.encode_idx(s.encode()), idx)
    e = fc.empty_batch()
    assert e.len.tolist() == [0, 0, 0] and len(e.off) == 3 and e.text.count(b">") == 3


@pytest.mark.parametrize("shift", fc.SEAM_SHIFTS)
def test_seam_text_has_a_chunk_start_in_every_part_of_the_walk(shift):
    d = fc.seam_text(shift)
    assert d.size == fc.GT_SWEEP + 4 * fc.VEC + 5
    starts, first_lf = fc.seam_answer(d)
    assert {fc.seam_region(int(s)) for s in starts[1:]} == {"first", "second", "tail"}
    assert fc.GT_SWEEP + shift in starts.tolist() and d[fc.GT_SWEEP + shift - 1] == 10
    assert sum(1 for s in starts[1:] if s % fc.VEC == 0 and s < fc.GT_SWEEP) >= 3          # '\n' the last byte of a vector
    assert int(starts[-1]) == d.size - 1 and int(first_lf[-1]) == d.size                     # the tail's last byte; no line feed
    assert (first_lf[1:-1] == starts[1:-1] + 3).all() and int(first_lf[0]) == 5 * fc.VEC - 1
    assert np.count_nonzero(d == 62) == starts.size - 1 + 4                                  # four '>' that open nothing
    text = d.tobytes()
    pos, found = text.find(b"\n>"), [0]
    while pos != -1:
        found.append(pos + 1)
        pos = text.find(b"\n>", pos + 1)
    assert found == starts.tolist()
