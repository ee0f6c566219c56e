"""The weight families of blend_family.py are what test_gpu_blend.py takes them for: on the intended side of the constructor's
bound, saturating the gates they name, and so well conditioned that a float32 evaluation of the plain statement stays within a tenth
of the kernels' contract of the float64 one -- a GPU failure on these inputs can then only be the kernel's."""
import numpy as np
import pytest

import blend_family as bf

SHAPES = sorted({(u, att, T, s, nw) for fam, u, T, att, s, nw, level, one, small in bf.TABLE})
IDS = [f"u{u}{'att' if att else ''}-T{T}" for u, att, T, s, nw in SHAPES]


def test_blend_bound_restates_the_constructor_by_hand():
    """Two units whose bound can be worked out on paper: unit 0 carries the z terms, unit 1 the candidate terms; the two z biases
    are summed before the absolute value, the two candidate biases after it."""
    class W:
        pass
    w = W()
    w.u = 2
    w.kernel = np.zeros((5, 6), np.float32)
    w.recurrent = np.zeros((2, 6), np.float32)
    w.bias = np.zeros((2, 6), np.float32)
    w.kernel[3, 0], w.kernel[1, 0] = -0.5, 0.25                  # kz of unit 0: 0.5
    w.bias[0, 0], w.bias[1, 0] = 8.0, -6.0                       # |8 - 6| = 2
    w.recurrent[:, 0] = (1.0, -2.0)                              # 3
    w.kernel[2, 5] = 0.75                                        # kg of unit 1
    w.bias[0, 5], w.bias[1, 5] = 8.0, -6.0                       # 8 + 6 = 14
    w.recurrent[:, 5] = (-0.5, 0.25)                             # 0.75
    w.recurrent[:, 2] = 100.0                                    # the r gate is no part of the bound
    assert bf.blend_bound(w) == pytest.approx(1 + 2 * bf.LOG2E * 15.5, rel=1e-15)
    w.bias[0, 0] = 60.0                                          # unit 0: 1 + log2e (0.5 + 54 + 3)
    assert bf.blend_bound(w) == pytest.approx(1 + bf.LOG2E * 57.5, rel=1e-15)


@pytest.mark.parametrize("u,att,T,s,nw", SHAPES, ids=IDS)
def test_families_lie_on_their_side_of_the_bound(orc, u, att, T, s, nw):
    """base < 100 < near <= 119 < 120 < 130 <= above; near holds a unit whose biases alone reach 2^90, its z bias negative and its
    candidate bias positive (both exponentials large), and units of the other three sign combinations; above holds z and candidate
    biases of either sign up to 90 and 45."""
    b = bf.base(orc, u, bf.C, T, att, bf.SEED)
    assert bf.blend_bound(b) < 100.0
    wa, ua = bf.above(orc, u, bf.C, T, att, bf.SEED)
    wn, un = bf.near(orc, u, bf.C, T, att, bf.SEED)
    assert bf.blend_bound(wa) >= 130.0
    assert 100.0 <= bf.blend_bound(wn) <= 119.0 < bf.LIMIT

    bz = lambda w, j: w.bias[0, j].astype(np.float64) + w.bias[1, j]
    drive = bf.bias_drive(wn)
    assert (drive[un["drive"]] >= 90.0).all()
    assert (bz(wn, un["drive"]) < -45).all() and (wn.bias[0, 2 * u + un["drive"]] > 10).all()
    signs = {(np.sign(bz(wn, j)), np.sign(wn.bias[0, 2 * u + j])) for j in un["other"]}
    assert signs == {(1, 1), (-1, -1), (1, -1)}
    picked = np.concatenate([un["drive"], un["other"]])
    assert len(set(picked)) == len(picked)

    za, ha = bz(wa, ua["zbias"]), wa.bias[:, 2 * u:][:, ua["hbias"]].sum(axis=0)
    assert za.max() > 19 and za.min() < -19 and np.abs(za).max() > 89 and np.abs(za).min() > 19
    assert ha.max() > 9 and ha.min() < -9 and np.abs(ha).max() > 44 and np.abs(ha).min() > 9
    assert len(ua["cols"]) >= 1 and len(set(np.concatenate(list(ua.values())))) == sum(map(len, ua.values()))
    for j in ua["cols"]:
        np.testing.assert_allclose(wa.recurrent[:, j], 6 * b.recurrent[:, j], rtol=1e-6)
        np.testing.assert_allclose(wa.recurrent[:, 2 * u + j], 6 * b.recurrent[:, 2 * u + j], rtol=1e-6)
        np.testing.assert_array_equal(wa.recurrent[:, u + j], b.recurrent[:, u + j])
    # nothing but the named units' columns differs from the base
    for w, touched in ((wa, np.concatenate(list(ua.values()))), (wn, picked)):
        keep = np.ones(3 * u, bool)
        keep[np.concatenate([touched, 2 * u + touched])] = False
        np.testing.assert_array_equal(w.recurrent[:, keep], b.recurrent[:, keep])
        np.testing.assert_array_equal(w.bias[:, keep], b.bias[:, keep])
        np.testing.assert_array_equal(w.kernel, b.kernel)
        np.testing.assert_array_equal(w.ff_kernel, b.ff_kernel)


@pytest.mark.parametrize("kind", ["above", "near"])
@pytest.mark.parametrize("u,att,T,s,nw", SHAPES, ids=IDS)
def test_families_are_well_conditioned(orc, kind, u, att, T, s, nw):
    """float32 against float64, both the plain statement on the CPU: within 1e-6, a tenth of the level-1 contract (measured: at most
    3.2e-7).  A condition on the inputs, not a measurement of any kernel: a shape that misses it wants another seed or other
    magnitudes, not another figure."""
    w, idx, want = bf.case(orc, kind, u, T, att, s, nw)
    got = orc.nn_forward(idx, w, s, 0, nw, np.float32)
    err = float(np.abs(got - want).max())
    print(f"{kind} u={u} T={T} att={att}: float32 - float64 = {err:.2e}")
    assert err < 1e-6
    assert np.isfinite(want).all() and want.shape == (nw, T, bf.C)
    # the saturated units leave the output alive: no class probability collapses to 0 or 1
    assert want.max() < 0.99 and want.min() > 1e-3


def test_saturated_units_reach_the_ends_of_both_gates(orc):
    """What the families are for, shown on the float64 numpy statement of the cell: in `near` the driven units sit at h = 1 from
    the first step (z = 0, tanh = 1: both exponentials of the one-reciprocal product large), the (+z) units stay at their initial
    0 and the (-z, -h) unit at -1; in `above` every z-bias unit is frozen at 0 or follows its candidate."""
    u, T, s, nw = 48, 30, 5, 4
    idx = bf.sequence(u, T, s, nw)
    for kind in ("near", "above"):
        w, named = getattr(bf, kind)(orc, u, bf.C, T, False, bf.SEED)
        W, U = w.kernel.astype(np.float64), w.recurrent.astype(np.float64)
        bi, br = w.bias.astype(np.float64)
        h = np.zeros((nw, u))
        win = idx[(np.arange(nw) * s)[:, None] + np.arange(T)[None, :]]
        zs, hs = [], []
        for t in range(T):
            xm, hm = np.eye(5)[win[:, t]] @ W + bi, h @ U + br
            z = 1 / (1 + np.exp(-(xm[:, :u] + hm[:, :u])))
            r = 1 / (1 + np.exp(-(xm[:, u:2 * u] + hm[:, u:2 * u])))
            h = z * h + (1 - z) * np.tanh(xm[:, 2 * u:] + r * hm[:, 2 * u:])
            zs.append(z), hs.append(h)
        zs, hs = np.stack(zs), np.stack(hs)
        bz = bi[:u] + br[:u]
        if kind == "near":
            assert np.abs(hs[:, :, named["drive"]] - 1).max() < 1e-8 and zs[:, :, named["drive"]].max() < 1e-20
            for j in named["other"]:
                want = 0.0 if bz[j] > 0 else -1.0
                assert np.abs(hs[:, :, j] - want).max() < 1e-8, (j, bz[j])
        else:
            for j in named["zbias"]:
                if bz[j] > 0:
                    assert np.abs(hs[:, :, j]).max() < 1e-6 and zs[:, :, j].min() > 1 - 1e-6
                else:
                    assert zs[:, :, j].max() < 1e-6
            for j in named["hbias"]:
                if abs(bi[2 * u + j]) > 9:                       # the input bias sits outside r * (...): the tanh is at its end
                    assert (np.sign(hs[-1, :, j]) == np.sign(bi[2 * u + j])).all()
