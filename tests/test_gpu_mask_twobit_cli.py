"""predict --mask_dir DIR --mask_twobit end to end: every .2bit written equals, byte for byte, the 2bit file that
tests/mask_twobit_cases.py states for the plain masked copy of the same input, rows, mode and classes; FASTA, BGZF and 2bit inputs
(both byte orders) give one and the same file; the TSV does not change; and predict on the written file gives the TSV of the
original input.  One child process per model runs the command lines.

The corpus is twobit_corpus.cli_file().  Two of its records are named `r` (sizes 1 and 70 001), which a 2bit file cannot hold, so
the byte-for-byte runs use the corpus with the later record of a name renamed, and the corpus as it is runs once more for what the
contract asks of it: one warning, no .2bit, the TSV unaffected."""
import gzip
import json
import os
import subprocess
import sys

import pytest

import mask_twobit_cases as mc
import twobit_corpus as tc
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

FLAGS = ["-b", "7", "-s", "4", "-x", "5", "-l", "3"]
DRIVER = ("import json, sys\n"
          "from deepgrp_amd.__main__ import main\n"
          "for argv in json.load(open(sys.argv[1])):\n"
          "    main(argv)\n")
MODES = {"soft": (), "hard": ("--mask", "hard"), "class1": ("--mask_classes", "1")}


def _unique(recs):
    seen, out = set(), []
    for i, r in enumerate(recs):
        name = r.name.strip().split()[0] if r.name.strip() else b""
        out.append(r._replace(name=r.name + b"_%d" % i) if name and name in seen else r)
        seen.add(name)
    return out


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("model", ["model_u8_T20.h5", "model_u16_T30_att_vlen.h5"])
def test_the_2bit_is_the_file_of_the_plain_masked_copy(tmp_path, model):
    from deepgrp_amd import gz, twobit
    from deepgrp_amd.fasta import _upload_file
    from deepgrp_amd.pipeline import require_gpu
    model_file = os.path.join(GOLDEN, model)
    as_is, many = tc.cli_file(), tc.batch_file(3000)
    recs = _unique(as_is)
    assert [r.name for r in as_is].count(b"r") == 2 and len(recs) == len(as_is)
    text = tc.text(recs)
    inputs = {"corpus.fa": text, "corpus.fa.gz": gz.bgzf_compress(text), "corpus.2bit": tc.write(recs), "swapped.2bit": tc.write(recs, ">"),
              "many.fa": tc.text(many), "dup.fa": tc.text(as_is)}
    for name, data in inputs.items():
        (tmp_path / name).write_bytes(data)

    def argv(name, tag, *extra):
        d = tmp_path / tag
        return FLAGS + ["predict", model_file, str(tmp_path / name), "--output", str(d) + ".tsv"] + [str(x).replace("DIR", str(d)) for x in extra]

    names = ["corpus.fa", "corpus.fa.gz", "corpus.2bit", "swapped.2bit", "many.fa"]
    runs = []
    for name in names:
        for mode, flags in MODES.items():
            runs.append(argv(name, f"tb_{name}_{mode}", "--mask_dir", "DIR", "--mask_twobit", *flags))
            runs.append(argv(name, f"plain_{name}_{mode}", "--mask_dir", "DIR", *flags, *(("--mask_gzip",) if name.endswith(".gz") else ())))
    runs.append(argv("dup.fa", "dup", "--mask_dir", "DIR", "--mask_twobit"))
    runs.append(argv("dup.fa", "dup_plain"))
    # reader, model and writer end to end: predict on the soft-masked .2bit written above
    runs.append(argv("tb_corpus.fa_soft/corpus.fa.2bit", "again"))
    (tmp_path / "runs.json").write_text(json.dumps(runs))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "-c", DRIVER, str(tmp_path / "runs.json")], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]

    out_name = {"corpus.fa": "corpus.fa.2bit", "corpus.fa.gz": "corpus.fa.2bit", "corpus.2bit": "corpus.2bit", "swapped.2bit": "swapped.2bit",
                "many.fa": "many.fa.2bit"}
    written = {}
    for name in names:
        for mode in MODES:
            plain = _files(tmp_path / f"plain_{name}_{mode}")
            assert len(plain) == 1
            (pname, masked), = plain.items()
            masked = gzip.decompress(masked) if pname.endswith(".gz") else masked
            got = _files(tmp_path / f"tb_{name}_{mode}")
            assert list(got) == [out_name[name]], (name, mode)
            assert got[out_name[name]] == mc.file_of(masked), (name, mode)
            written[name, mode] = got[out_name[name]]
            # the flag does not reach the TSV
            assert (tmp_path / f"tb_{name}_{mode}.tsv").read_bytes() == (tmp_path / f"plain_{name}_{mode}.tsv").read_bytes()
            if mode == "hard" and name == "corpus.fa":
                # the text of the hard-masked file is the plain hard-masked copy, normalised (case aside: both keep the input's)
                path = tmp_path / f"tb_{name}_{mode}" / out_name[name]
                back = twobit.DeviceTwoBit(twobit.open_twobit(path), require_gpu(), _upload_file).text().cpu().numpy().tobytes()
                assert back == mc.normalised(masked) and back.lower() == mc.normalised(masked).lower()
                assert masked != text
    tsv = (tmp_path / "tb_corpus.fa_soft.tsv").read_bytes()
    assert tsv.count(b"\n") > 0 and (tmp_path / "tb_many.fa_soft.tsv").read_bytes().count(b"\n") > 0
    for mode in MODES:
        # FASTA, BGZF and 2bit inputs in either byte order: one file
        assert written["corpus.fa", mode] == written["corpus.fa.gz", mode] == written["corpus.2bit", mode] == written["swapped.2bit", mode], mode
    assert written["corpus.fa", "soft"] != written["corpus.fa", "hard"]
    # the corpus as it is: two records named `r` -- one warning that names the input and the record, no file, the TSV as without the flag
    assert os.listdir(tmp_path / "dup") == []
    warned = [ln for ln in r.stderr.splitlines() if "--mask_twobit" in ln]
    assert len(warned) == 1 and str(tmp_path / "dup.fa") in warned[0] and "b'r'" in warned[0], r.stderr[-2000:]
    assert (tmp_path / "dup.tsv").read_bytes() == (tmp_path / "dup_plain.tsv").read_bytes()

    # predict on the soft-masked .2bit gives the TSV of the original input (case does not reach the encoder), apart from the name column
    old, new = str(tmp_path / "tb_corpus.fa_soft" / "corpus.fa.2bit").encode() + b"\t", str(tmp_path / "corpus.fa").encode() + b"\t"
    lines = (tmp_path / "again.tsv").read_bytes().split(b"\n")
    assert all(ln.startswith(old) for ln in lines[:-1])

    def first_word(data):
        """The TSV with every record header (second column) cut to its first word, as the 2bit file names the record."""
        rows = [ln.split(b"\t") for ln in data.split(b"\n")]
        return b"\n".join(b"\t".join(c[:1] + [c[1].split()[0]] + c[2:]) if len(c) > 1 else b"".join(c) for c in rows)

    assert b" padded\t" in tsv                                         # (one header of the corpus is more than its first word)
    assert b"\n".join(new + ln[len(old):] if ln else ln for ln in lines) == first_word(tsv)
