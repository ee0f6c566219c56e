"""The workspaces of the two zoom entries without a GPU.  Both ladders stand on one carve of the levels (csrc/bbi_zoom.h), and the
header promises 40 bytes per bigWig window and 12.04 per bigBed window: the two queries, which are host arithmetic, return what
they returned before the ladder was shared."""
import numpy as np
import pytest

# nrows, record ends: the `zoom` and `batch` cases of test_gpu_bigbed.py
BED = {"zoom": (10, [900, 5000, 3_200_000, 2000, 6000], 80_384),
       "batch": (1215, [77, 50_000, 50_000, 1, 50_000], 91_136)}
# bin width -> bytes, for the records of _case in test_gpu_bigwig.py with four classes
TRACK = {1: 1_019_904, 50: 946_176, 65: 946_176}


@pytest.fixture(scope="module")
def L():
    from deepgrp_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", list(BED))
def test_bed_zoom_workspace_is_the_parents(L, name):
    """The constants are what the library of commit 9d2fe2f (the last one with a ladder per format) returned for these shapes."""
    nrows, ends, want = BED[name]
    ends = np.array(ends, np.int64)
    assert L.dgrp_bed_zoom_workspace_bytes(nrows, len(ends), ends.ctypes.data) == want


@pytest.mark.parametrize("width", list(TRACK))
def test_track_zoom_workspace_is_the_parents(L, width):
    """The constants are what the library of commit 9d2fe2f (the last one with a ladder per format) returned for these shapes."""
    b = width
    n = np.array([1, 777, 1024 * b, 1025 * b, 300, 18_000 * b], np.int64)
    spos = np.array([0, 13, 3 * b, 0, 5, 2 * b + (b > 1)], np.int64)
    assert L.dgrp_track_zoom_workspace_bytes(len(n), n.ctypes.data, spos.ctypes.data, b, 4) == TRACK[width]
