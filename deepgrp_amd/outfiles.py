"""Staged output files, the layer under `predict --track_dir` and `--bed_dir` (tracks.TrackFiles, bed.BedFiles): a file is written
under a temporary name next to its final one and renamed when its input is done (`StagedFile`); a BGZF file takes the members of
every write and, where a tabix index was asked for, builds `<file>.tbi` or `<file>.csi` beside it (`BgzfSink`); `StagedOutputs`
is what the files of one input share: the rule on record names, one warning when the input cannot be indexed, and a commit that leaves no temporary
file behind when it fails.  The outputs that are written when their input is done (--mask_dir, --seq_dir, --summary_dir) share
`RowsOutput` and its handle `AtCommit`; the plans of the outputs share `plan_inputs`, what they refuse of their inputs, and
`class_list`, the type of their label flags.  The reports of `evaluate` share `plan_prefix`, the refusals of their `--<report>
PREFIX`, and `write_texts`, their staged text files."""
from __future__ import annotations

import os
import sys
import tempfile
from typing import Iterable, Optional, Sequence

from . import tabix
from .gz import BGZF_EOF


class StagedFile:
    """`final`, written as `.<basename>.<random>.tmp` in its directory (`fh`).  `finish` completes the temporary file, `commit`
    renames the finished file into place, `abort` removes it; `commit` and `abort` are safe behind each other."""

    def __init__(self, final: str, mode: str = "wb"):
        self.final = final
        fd, self.tmp = tempfile.mkstemp(prefix="." + os.path.basename(final) + ".", suffix=".tmp", dir=os.path.dirname(final) or ".")
        self.fh = os.fdopen(fd, mode)

    def append(self, data: bytes, *_index) -> None:
        self.fh.write(data)

    def finish(self) -> None:
        self.fh.close()

    def commit(self) -> None:
        if self.tmp is not None:
            os.replace(self.tmp, self.final)
        self.tmp = None

    def abort(self) -> None:
        self.fh.close()
        if self.tmp is not None and os.path.exists(self.tmp):
            os.remove(self.tmp)
        self.tmp = None


class BgzfSink:
    """One BGZF file from the members of its writes.  With `index`, `builder` (a tabix.IndexBuilder, until someone sets it to None)
    takes every write at the file offset it goes to.  `finish` puts the EOF member behind the members and stages the `.tbi`;
    `commit` renames the file, then its `.tbi` -- or, the index dropped, removes a `.tbi` an earlier run left.  Without `index` a
    `.tbi` beside the file is not this run's to touch.  `preset`: the index's preset where it is not tabix.PRESET_BED.
    `fmt` "csi": the index is `<file>.csi` (tabix.CSI_DEPTH levels), staged, committed and aborted as the `.tbi` is.  With `index`,
    `commit` also removes the other format's index of this file where one lies: it describes an earlier run's bytes, and a reader
    looks for `.csi` before `.tbi`."""

    def __init__(self, final: str, index: bool = False, preset=tabix.PRESET_BED, fmt: str = "tbi"):
        self.fmt = fmt
        depth = tabix.CSI_DEPTH if fmt == "csi" else 5
        self.index_wanted, self.builder = index, tabix.IndexBuilder(preset, fmt, depth) if index else None
        self.off = 0                                    # bytes of members written
        self.tbi: Optional[StagedFile] = None           # the staged index, of either format
        self.data = StagedFile(final)

    def append(self, members: bytes, names: Sequence[bytes], chunks, linear, wpref, last_end=None) -> None:
        """The members of one write and, while the index lives, its part of it (tabix.IndexBuilder.add; an IndexRefused leaves them written)."""
        self.data.fh.write(members)
        off, self.off = self.off, self.off + len(members)
        if self.builder is not None and members:
            sizes, text_len = tabix.member_sizes(members)
            self.builder.add(off, sizes, text_len, names, chunks, linear, wpref, last_end)

    def finish(self) -> None:
        self.data.fh.write(BGZF_EOF)
        self.data.finish()
        if self.builder is not None:
            self.tbi = StagedFile(self.data.final + "." + self.fmt)
            self.tbi.fh.write(tabix.index_file(self.builder.payload()))
            self.tbi.finish()

    def commit(self) -> None:
        self.data.commit()
        if self.tbi is not None:
            self.tbi.commit()
        elif self.index_wanted and os.path.exists(self.data.final + "." + self.fmt):
            os.remove(self.data.final + "." + self.fmt)
        other = self.data.final + (".tbi" if self.fmt == "csi" else ".csi")
        if self.index_wanted and os.path.exists(other):
            os.remove(other)

    def abort(self) -> None:
        self.data.abort()
        if self.tbi is not None:
            self.tbi.abort()


class StagedOutputs:
    """The files of one input (`parts`: one StagedFile or BgzfSink per file) behind one `commit` and one `abort`.  `indexed` says
    whether a tabix index is still being built; `no_index` drops it for every part, with one warning to `log` that names the input
    and the flag."""

    def __init__(self, log, filename: str, flag: str, indexed: bool, parts: Iterable):
        self.log, self.filename, self.flag, self.indexed = log, filename, flag, indexed
        self.seen, self.last = set(), None
        self.parts = []
        try:
            for p in parts:                             # (made one by one: the ones made go when a later one cannot be)
                self.parts.append(p)
        except BaseException:
            self.abort()
            raise

    def name_order(self, names: Sequence[bytes]) -> Optional[str]:
        """The rule a tabix index has for the record names of an input, over all its writes: none empty, and none that comes back
        behind another name (the same name twice in a row is one sequence).  Registers `names`: why there is no index, or None."""
        for nm in names:
            if not nm:
                return "a record with an empty name"
            if nm != self.last:
                if nm in self.seen:
                    return f"the record name {nm.decode('utf-8', 'replace')!r} reappears after another name"
                self.seen.add(nm)
                self.last = nm
        return None

    def distinct_names(self, names: Sequence[bytes]) -> Optional[str]:
        """The rule a bigWig or bigBed has for the record names of an input, over all its writes: none empty, no two alike.
        Registers `names` (in `seen`, as name_order does: a file has one rule or the other): why there is no file, or None."""
        for nm in names:
            if not nm:
                return "a record with an empty name"
            if nm in self.seen:
                return f"two records have the name {nm.decode('utf-8', 'replace')!r}"
            self.seen.add(nm)
        return None

    def no_index(self, why: Optional[str]) -> None:
        if why is not None and self.indexed:
            self.log.warning("%s: no tabix index is written (%s): %s", self.filename, self.flag, why)
            for p in self.parts:
                p.builder = None
            self.indexed = False

    def append(self, k: int, data: bytes, names: Sequence[bytes] = (), chunks=None, linear=None, wpref=None, last_end=None) -> None:
        """One write's bytes for file k, with its part of the index while there is one (an IndexRefused ends it)."""
        try:
            self.parts[k].append(data, names, chunks, linear, wpref, last_end)
        except tabix.IndexRefused as e:
            self.no_index(str(e))

    def commit(self) -> None:
        """Every part finished, then every part renamed into place.  When a `finish` raises, all parts are aborted first: no
        temporary file remains, no file of this run appears, and what an earlier run left is untouched."""
        try:
            for p in self.parts:
                p.finish()
        except BaseException:
            self.abort()
            raise
        for p in self.parts:
            p.commit()

    def abort(self) -> None:
        for p in self.parts:
            p.abort()


class AtCommit:
    """The handle of a RowsOutput for one input: `take` has nothing to do with a work item, `commit(rows, log)` is the output's
    `write(filename, rows, log)`, and `abort` has nothing to remove, because `write` stages its own files and leaves none behind
    when it raises."""

    def __init__(self, output, filename: str):
        self.output, self.filename = output, filename

    def take(self, names, batch, rows, scores, texts) -> None:
        pass

    def commit(self, rows, log) -> None:
        self.output.write(self.filename, rows, log)

    def abort(self) -> None:
        pass


class RowsOutput:
    """An output of `predict` that is written when its input is done, from all of the input's rows (--mask_dir, --seq_dir,
    --summary_dir): it wants the rows kept, asks nothing of the RecordRunner, and has `write(filename, rows, log)`."""
    wants_rows = True
    runner: dict = {}

    def __init__(self, plan):
        self.plan = plan

    def open(self, filename: str) -> AtCommit:
        return AtCommit(self, filename)


def plan_inputs(flag: str, inputs: Sequence[str], outputs_of, copies: str, output: str = "output", stdin: Optional[str] = None,
                npz: Optional[str] = None, every_input: bool = False, directory: Optional[str] = None) -> dict:
    """What the outputs of `predict` refuse of their inputs (sys.exit, before the model is read), input by input: standard input
    (`stdin`: what cannot be done with it; None: it is an input like any other), a one-hot .npz (`npz`: why not; None: the same),
    two inputs whose first output has one file name -- `copies` names the outputs in the plural --, an output that is an input
    (`output` names it; every_input: any of the inputs, else the output's own one), and an input given twice.  outputs_of(input)
    -> the path of its output, or the paths of its outputs with None where one is not written; it may refuse the input itself.
    Real paths are compared throughout.  `directory` is made once nothing was refused.  -> {input: what outputs_of gave}"""
    plan, seen = {}, {}
    for f in inputs:
        if f == "-" and stdin is not None:
            sys.exit(f"{flag}: standard input cannot be {stdin} (give a FASTA file)")
        if f.endswith(".npz") and npz is not None:
            sys.exit(f"{flag}: {f} is a one-hot .npz, not a FASTA file; it {npz}")
        outs = outputs_of(f)
        paths = (outs,) if isinstance(outs, str) else outs
        base = os.path.basename(paths[0])
        if base in seen and os.path.realpath(seen[base]) != os.path.realpath(f):
            sys.exit(f"{flag}: the {copies} of {seen[base]} and {f} have the same file name {base}; they would collide")
        seen[base] = f
        for out in filter(None, paths):
            for g in inputs if every_input else [f]:
                if g != "-" and os.path.exists(g) and os.path.realpath(out) == os.path.realpath(g):
                    sys.exit(f"{flag}: the {output} {out} would overwrite the input {g}")
        plan[f] = outs
    if len(plan) != len(inputs):
        sys.exit(f"{flag}: an input file is given twice")
    if directory is not None:
        os.makedirs(directory, exist_ok=True)
    return plan


def class_list(text: str) -> tuple:
    """A command-line value that is a comma-separated list of labels (argparse `type=`)."""
    import argparse
    try:
        out = tuple(int(x) for x in text.split(",") if x.strip())
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a comma-separated list of labels: {text!r}") from None
    if not out:
        raise argparse.ArgumentTypeError("no label given")
    return out


def plan_prefix(flag: str, prefix: str, suffixes: Sequence[str], args, why: str, refuse_directory: bool = True,
                other_inputs: Sequence[str] = ("annotation", "model")) -> tuple:
    """What the `evaluate` reports refuse of `flag PREFIX` (sys.exit, before the model is read): a prefix that is a directory (one
    that only exists as a directory passes with refuse_directory False), WORLD_SIZE > 1 -- `why` says what could not be summed --,
    a directory that does not exist, an output PREFIX + suffix that is an input: args.FASTA and args.<other_inputs>.
    -> the output paths."""
    if prefix == "" or prefix.endswith(os.sep) or (refuse_directory and os.path.isdir(prefix)):
        sys.exit(f"{flag} takes a file name prefix, not the directory {prefix!r}")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        sys.exit(f"{flag} runs in one process (WORLD_SIZE > 1 is not supported: {why})")
    where = os.path.dirname(prefix) or "."
    if not os.path.isdir(where):
        sys.exit(f"{flag}: the directory {where} does not exist")
    paths = tuple(prefix + s for s in suffixes)
    for f in list(getattr(args, "FASTA", [])) + [getattr(args, k, None) for k in other_inputs]:
        for out in paths:
            if f not in (None, "-") and os.path.exists(f) and os.path.realpath(out) == os.path.realpath(f):
                sys.exit(f"{flag}: the file {out} would overwrite the input {f}")
    return paths


def write_texts(log, prefix: str, flag: str, paths: Sequence[str], texts: Sequence[str]) -> None:
    """The text files of one report, staged: a failure leaves none of them, nor a temporary file."""
    out = StagedOutputs(log, prefix, flag, False, (StagedFile(f, "w") for f in paths))
    try:
        for part, text in zip(out.parts, texts):
            part.fh.write(text)
    except BaseException:
        out.abort()
        raise
    out.commit()
