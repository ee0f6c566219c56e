"""predict on a 2bit file end to end: every output equals, byte for byte, the output on the text of the file (tests/twobit_corpus.py
states the text), apart from the input's name -- TSV, masked copy (plain and BGZF), probability tracks and scored BED, on the
one-by-one path and, with a file of 3 000 short records, on the batch path.  One child process per model runs the command lines."""
import gzip
import json
import os
import subprocess
import sys

import pytest

import twobit_corpus as tc
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

FLAGS = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
DRIVER = ("import json, sys\n"
          "from deepgrp_amd.__main__ import main\n"
          "for argv in json.load(open(sys.argv[1])):\n"
          "    main(argv)\n")


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("model", ["model_u8_T20.h5", "model_u16_T30_att_vlen.h5"])
def test_every_output_is_the_output_on_the_text(tmp_path, model):
    model_file = os.path.join(GOLDEN, model)
    recs, many = tc.cli_file(), tc.batch_file(3000)
    inputs = {"corpus.2bit": tc.write(recs), "corpus.fa": tc.text(recs), "swapped.2bit": tc.write(recs, ">"),
              "many.2bit": tc.write(many), "many.fa": tc.text(many)}
    for name, data in inputs.items():
        (tmp_path / name).write_bytes(data)

    def argv(name, tag, *extra):
        d = tmp_path / tag
        return FLAGS + ["predict", model_file, str(tmp_path / name), "--output", str(d) + ".tsv"] + [str(x).replace("DIR", str(d)) for x in extra]

    outputs = ("--mask_dir", "DIR/masked", "--track_dir", "DIR/tracks", "--bed_dir", "DIR/bed")
    runs = [argv("corpus.2bit", "tb", *outputs), argv("corpus.fa", "fa", *outputs), argv("swapped.2bit", "be", *outputs),
            argv("corpus.2bit", "tb_hard", "--mask_dir", "DIR/masked", "--mask", "hard", "--mask_gzip"),
            argv("corpus.fa", "fa_hard", "--mask_dir", "DIR/masked", "--mask", "hard"),
            argv("many.2bit", "tb_many"), argv("many.fa", "fa_many")]
    (tmp_path / "runs.json").write_text(json.dumps(runs))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "-c", DRIVER, str(tmp_path / "runs.json")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def tsv(tag, name, as_name):
        """The TSV of a run with the input's name in its first column mapped."""
        lines = (tmp_path / f"{tag}.tsv").read_bytes().split(b"\n")
        old, new = str(tmp_path / name).encode() + b"\t", str(tmp_path / as_name).encode() + b"\t"
        assert all(ln.startswith(old) for ln in lines[:-1])
        return b"\n".join(new + ln[len(old):] if ln else ln for ln in lines)

    want = (tmp_path / "fa.tsv").read_bytes()
    assert want.count(b"\n") > 0
    for tag, name in (("tb", "corpus.2bit"), ("be", "swapped.2bit")):
        assert tsv(tag, name, "corpus.fa") == want, tag
        masked = _files(tmp_path / tag / "masked")
        assert list(masked) == [name + ".fa"]
        assert masked[name + ".fa"] == (tmp_path / "fa" / "masked" / "corpus.fa").read_bytes(), tag
        tracks, bed = _files(tmp_path / tag / "tracks"), _files(tmp_path / tag / "bed")
        want_tracks = _files(tmp_path / "fa" / "tracks")
        assert len(want_tracks) >= 1 and all(len(v) > 0 for v in want_tracks.values())
        assert {k.replace(name, "corpus.fa", 1): v for k, v in tracks.items()} == want_tracks, tag
        assert {k.replace(name, "corpus.fa", 1): v for k, v in bed.items()} == _files(tmp_path / "fa" / "bed"), tag
    # the soft-masked copy has the text's length and letters; it is not the text itself (the prediction decides the case)
    soft = (tmp_path / "fa" / "masked" / "corpus.fa").read_bytes()
    assert soft.lower() == tc.text(recs).lower()
    # hard mask, BGZF: the member stream inflates to the hard-masked text
    hard = _files(tmp_path / "tb_hard" / "masked")
    assert list(hard) == ["corpus.2bit.fa.gz"]
    assert gzip.decompress(hard["corpus.2bit.fa.gz"]) == (tmp_path / "fa_hard" / "masked" / "corpus.fa").read_bytes()
    assert tsv("tb_hard", "corpus.2bit", "corpus.fa") == (tmp_path / "fa_hard.tsv").read_bytes() == want
    # 3 000 short records: the batch path
    want_many = (tmp_path / "fa_many.tsv").read_bytes()
    assert want_many.count(b"\n") > 0
    assert tsv("tb_many", "many.2bit", "many.fa") == want_many
