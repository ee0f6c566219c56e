"""One phase of gru_split2_kernel, held bit for bit across changes of its schedule: where the generated interleave puts a link, which
LDS round trip a wait covers and how an address is formed must not show in a single bit of the output.

Every case runs `forward_windows` (mode 1, window rows) and `ContigPipeline.merged` (mode 0, the image in LDS) on the split2 kernel at
128 and at 97 units and is held
  * to the float64 statement at 1e-5, the bound of the other forward tests, and
  * to a SHA-256 of the output bytes (window rows, merged rows), recorded ONCE on an MI355X from the build of commit 1a347eb
    ("Test the LSTM cell and the GRU above 128 units on saturated gates"), the parent of the change that re-cut the phase's waits.

Cases: T = 40, s = 7 at 1, 16, 17, 32 and 33 windows (one tile, a full tile, a second tile of one window, a full pair, a second pair);
T = 3, 2 and 1, where the time loop's body runs once or not at all and XP reads a byte outside the window, so that the clamp of
tab_rows decides; and class 4 at the places the two arms of `bf < 4 ? bf : 4` and `br < 4 ? 3 - br : 4` turn on: a record whose
windows all begin and end with class 4, and a record of disjoint windows with one window of nothing but class 4 and one without any
in each tile, so that both arms of both selects run at every step position.

The weights are drawn element by element from numpy's Generator (no factorisation: the same bits wherever numpy is the same)."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NCLS, B = 5, 16
UNITS = (128, 97)

# (name, T, s, windows, kind of record)
SHAPES = [
    ("T40-s7-nw1", 40, 7, 1, "random"),
    ("T40-s7-nw16", 40, 7, 16, "random"),
    ("T40-s7-nw17", 40, 7, 17, "random"),
    ("T40-s7-nw32", 40, 7, 32, "random"),
    ("T40-s7-nw33", 40, 7, 33, "random"),
    ("T3-s2-nw33", 3, 2, 33, "random"),
    ("T2-s1-nw33", 2, 1, 33, "random"),
    ("T1-s1-nw33", 1, 1, 33, "random"),
    ("T40-s7-nw33-edges4", 40, 7, 33, "edges4"),
    ("T40-s40-nw33-mixed4", 40, 40, 33, "mixed4"),
]
CASES = [(u, *shape) for u in UNITS for shape in SHAPES]

# SHA-256 of (window rows, merged rows) as float32 bytes, from the build of commit 1a347eb on an MI355X
RECORDED = {
    "u128-T40-s7-nw1": ("26cbf74b54867b1e777113a2208cbf0fcfce8fc07cecd4121d8b55fb52761b94",
                        "e167de852e17eb50d1fa55c67642c542f96b8c5c6fbcb2bc8175c0cc2ba13daa"),
    "u128-T40-s7-nw16": ("952c523225a210d916767670b40721e2eb7217457d16e3f1492992129d16a376",
                        "b21461dd9f5254fd0b0bd19c3214cc09648cdec9b38354e823c2965ec1666708"),
    "u128-T40-s7-nw17": ("9867599013e8f2c0f477ed3cf8f5afa5d69ee05a8ee08ab172dc2776169f651b",
                        "c123c5ef823288a8e434cb6b131135862d87001c8d54092c2b27721c71fdeac2"),
    "u128-T40-s7-nw32": ("bc4bf0a8855919bb6a28d94c452195fc72ea145b191e053505e18c427bc329fe",
                        "403a1b4a25872baf9d04a5611d5e6474523c28977f77e28c72cae07394257e9b"),
    "u128-T40-s7-nw33": ("549b1fb4df34685563debf491a087a5c389ffac7fd00be80478b33a809bfde42",
                        "f462a7520912bccb70dcd604e45c941c0989db1e6bb0fa960853fdeb06cee782"),
    "u128-T3-s2-nw33": ("f131dac5f8d95d18c71d82971003f9b654008d916f4fa010f46cabf3348e4064",
                        "598005ff325ec786091efd5468cccd8b44c31da14bf6133301c6b92bea5c7a60"),
    "u128-T2-s1-nw33": ("a5dd52996d82e0e6449630099b69e417322274158759c6180e472c9d24f7169f",
                        "3b9c5b2f46674330fdb6618505f16c067da4fbd0641377f58be0b414cdf4dc42"),
    "u128-T1-s1-nw33": ("24948785cc8f0d5b443526719e8750c3f017c3a594480180190562e48a68cbae",
                        "3e5b2c228989324db1d6ab8724cd9c85e35ea0fdd2b2c09d6cad2acd5cda82a6"),
    "u128-T40-s7-nw33-edges4": ("35708b9080b35212b6d4bb59df5a5840dbb41499c9b46d7ccc5eeabfe9140b04",
                        "913876b7ddc566db0dfc85d8d689432962869d3f3942f55c33d835ff9a919fc8"),
    "u128-T40-s40-nw33-mixed4": ("800608e1eb76722d8d7e7d68fb7f7f104fa78c038dd64ac7974bda0cfb351df6",
                        "96a9a031f01fa0fb6d2fafc9c5301c2b86e4904c845d3577b469f2d560f45bfd"),
    "u97-T40-s7-nw1": ("d26e423b351b0c3b32414926c9050627d25bc1b4e8e58bcf7984eb8ca15f1797",
                        "a4b933b46e25dc102068b9ceabaed75fd9ddb1ada9dec401b4ff93a6b2cd9abd"),
    "u97-T40-s7-nw16": ("55910583fde508b808b29a4e39789614480f9b69006aa452941d47196f340a96",
                        "175c6d9ed1226f9898ae9355a08ff7f4a63166c4287a2e04df9cee3d2c901a5a"),
    "u97-T40-s7-nw17": ("5d627aaaa9507acfc119a78fccaee875e66b418542726d918b6d9de209ad0385",
                        "6908a22995b5a7ff1f33bd25a5cf32b8e2b4a6b360ea117d1aa5417b69d25d1c"),
    "u97-T40-s7-nw32": ("ab5d05497cc5c41bea345be9c7adb2acc592cbd04dab221629c24ab74194a03e",
                        "e09d384e7e2b95bc9daa0840c32eb80f76376aaaac23ec82458aad65c5edc106"),
    "u97-T40-s7-nw33": ("275c569b2e673150f96e85345833232cbf3b4383ad55af93a5a169ada856d704",
                        "e6e059b8d06f70b310f5e077c57f7f934890e351cbf8e032b30ffbd43a393148"),
    "u97-T3-s2-nw33": ("47dc4869fa29fb0fd4b72c62e585eba1cabc7ee25c2f776573d773401e38096e",
                        "85d6337634b8527c0edea8f7bbeae4ca3e6eb2b3242a667082bb85ff19b929ca"),
    "u97-T2-s1-nw33": ("b9d77505c0171bed295842f9f31366f484e60d57024bd5364a30fc7e4ed80ecb",
                        "7681c23d264e720d7e2926892e8f7756d858f5e9649ec73718d7f622dc9fb34f"),
    "u97-T1-s1-nw33": ("d0fa3e890d061fe129456ddd68bf87d6a1af6bff6b9ba76be876b1452a8c244a",
                        "55657ec04821b5e872d08c47d6cf3d4cf1133c97d63692ffe10333951defb6ae"),
    "u97-T40-s7-nw33-edges4": ("ca1f465f30aa1d04b5d60fe0bbb2449812dce20e6cd84ed6dd3441f3da1768de",
                        "fd3d795c9c02b193cba3abe461d4ec331f5852fc5092b08c0cb8e5a1ed99346a"),
    "u97-T40-s40-nw33-mixed4": ("6b3571e8fea83da1d67bd41a3a4607a7bac34a98dfae5ac0e0f7e4291545675c",
                        "40cb5916ca6561c3857e887934064a5393645db05ddc274513cd7ca803a0acf0"),
}


def _id(case):
    return f"u{case[0]}-{case[1]}"


def _weights(orc, u, T, seed):
    rng = np.random.default_rng(seed)
    lim = np.sqrt(6.0 / (5 + 3 * u))
    kernel = rng.uniform(-lim, lim, size=(5, 3 * u)) * 2.0
    recurrent = rng.normal(scale=2.0 / np.sqrt(u), size=(u, 3 * u))
    bias = rng.normal(scale=0.2, size=(2, 3 * u))
    lim = np.sqrt(6.0 / (u + NCLS))
    ffk = rng.uniform(-lim, lim, size=(u, NCLS)) * 2.0
    ffb = rng.normal(scale=0.2, size=(NCLS,))
    return orc.Weights(kernel, recurrent, bias, ffk, ffb, None, T)


def _record(kind, T, s, nw, seed):
    """the shortest record that is cut into nw windows"""
    rng = np.random.default_rng(seed)
    n = T + s * (nw - 1) + 1
    if kind == "random":
        return rng.choice(5, size=n, p=[0.24, 0.25, 0.25, 0.24, 0.02]).astype(np.uint8)
    idx = rng.integers(0, 4, size=n).astype(np.uint8)
    if kind == "edges4":
        for w in range(nw):
            idx[w * s] = idx[w * s + T - 1] = 4
        return idx
    assert kind == "mixed4" and s >= T and nw > 21
    some = rng.random(n) < 0.3
    idx[some] = 4
    for all4, none4 in ((5, 6), (20, 21)):                       # one of each in either tile of the first pair
        idx[all4 * s:all4 * s + T] = 4
        idx[none4 * s:none4 * s + T] = rng.integers(0, 4, size=T)
    for t in range(T):                                           # both arms of both selects at every step position
        col = idx[np.arange(nw) * s + t]
        assert (col == 4).any() and (col < 4).any()
    return idx


@pytest.fixture(scope="module")
def dev():
    from deepgrp_amd.pipeline import require_gpu
    return require_gpu()


@pytest.fixture(scope="module")
def models(dev, orc):
    """(units, T) -> (oracle weights, device model): built once, shared, never written to"""
    from deepgrp_amd.pipeline import DeviceModel
    out = {}
    for u in UNITS:
        for T in sorted({shape[1] for shape in SHAPES}):
            w = _weights(orc, u, T, seed=1000 * u + T)
            out[u, T] = (w, DeviceModel(w.kernel, w.recurrent, w.bias, w.ff_kernel, w.ff_bias, None, vecsize=T))
    yield out
    for _w, dm in out.values():
        dm.close()


def _sha(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_phase_bits_and_float64(dev, orc, models, case):
    from deepgrp_amd.pipeline import ContigPipeline
    u, name, T, s, nw, kind = case
    w, dm = models[u, T]
    idx = _record(kind, T, s, nw, seed=u + 7 * T + s + nw)
    n = idx.size
    assert orc.window_count(n, T, s) == nw
    d = torch.from_numpy(idx).to(dev)
    pipe = ContigPipeline(dm, s, B, 50, 50, True)
    assert dm.plan(1, s).kernel == "split2" and dm.plan(0, s, handle=pipe.handle).kernel == "split2"
    rows = dm.forward_windows(d, s, 0, nw).cpu().numpy()
    merged = pipe.merged(d).cpu().numpy()
    pipe.close()
    assert rows.shape == (nw, T, NCLS) and merged.shape == (n, NCLS)

    got = (_sha(rows), _sha(merged))
    print(f'    "{_id(case)}": ("{got[0]}",\n        "{got[1]}"),')

    want = orc.nn_forward(idx, w, s, 0, nw, np.float64)
    err = float(np.abs(rows - want).max())
    err_m = float(np.abs(merged - orc.merge_all(want.astype(np.float32), n, s, B)).max())
    print(f"{_id(case)}: window rows max |dp| = {err:.3e}, merged rows {err_m:.3e}")
    assert err < 1e-5 and err_m < 1e-5
    assert got == RECORDED[_id(case)]
