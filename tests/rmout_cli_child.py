"""The child process of tests/test_gpu_rmout_cli.py (a plain helper, no tests here): `python tests/rmout_cli_child.py JOBS.json` runs
the jobs of the file one after the other in this one process.  A job is {"main": argv} -- the command line --, {"parse_rm": argv} --
the console script -- or {"compose": {...}}: the rows, scores and end coordinate of every record of an input by the Python API
(merged -> labels -> segments -> row_scores), pickled as [(record name, rows, scores, rec_end), ...] for the parent to state the
listing from with rmout.reference_lines."""
import json
import logging
import pickle
import sys


def compose(model_file, path, out, flags):
    from deepgrp_amd import model as dgmodel
    from deepgrp_amd.__main__ import _records_of
    from deepgrp_amd.evaluation import record_name
    from deepgrp_amd.pipeline import ROW_SCORE_DTYPE, SEGMENT_DTYPE, ContigPipeline, record_indices
    import numpy as np
    model = dgmodel.load_model(model_file)
    pipe = ContigPipeline(model, flags["s"], flags["b"], flags["l"], flags["x"])
    recs = []
    for header, rec in _records_of(path):
        startpos, d_idx = record_indices(rec)
        if d_idx.numel() == 0:
            recs.append((record_name(path, header), np.zeros(0, SEGMENT_DTYPE), np.zeros(0, ROW_SCORE_DTYPE), int(startpos)))
            continue
        merged = pipe.merged(d_idx)
        rows = pipe.segments(pipe.labels(merged), startpos)
        recs.append((record_name(path, header), rows, pipe.row_scores(merged, startpos, rows), int(startpos) + len(merged)))
    with open(out, "wb") as fh:
        pickle.dump({"classes": int(model.output_shape[2]), "records": recs}, fh)
    pipe.close()
    model.close()


if __name__ == "__main__":
    from deepgrp_amd.__main__ import main
    from deepgrp_amd._scripts import parse_rm
    with open(sys.argv[1]) as fh:
        jobs = json.load(fh)
    for job in jobs:
        if "main" in job:
            main(job["main"])
            logging.getLogger("deepgrp_amd.__main__").setLevel(logging.WARNING)      # -vv sets the module's level for the process
        elif "parse_rm" in job:
            parse_rm.main(job["parse_rm"])
        else:
            compose(**job["compose"])
