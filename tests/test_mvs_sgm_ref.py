"""tests/mvs_sgm_ref.py, the CPU restatement of MultiViewStereo's semi-global aggregation (the header's definition), checked
against itself and against the oracle's MRF terms -- no device."""
import ctypes as C

import numpy as np
import pytest

import mrf_cases
import mvs_sgm_ref as G
import oracle_ffi as O

GRIDS = [(1, 1), (5, 1), (1, 6), (4, 3), (9, 7)]


def _case(w, h, K, seed=None):
    return mrf_cases.peaks_case(w, h, K=K, seed=w * 131 + h + K if seed is None else seed, fill=0.6)


@pytest.mark.parametrize("K", [1, 4, 9, 15])
def test_vectorised_and_loop_forms_agree_bit_for_bit(K):
    for w, h in GRIDS:
        peaks, mask = _case(w, h, K)
        a = G.aggregate(peaks, view_mask=mask, depth=np.full((h, w), -7.0))
        b = G.aggregate_loops(peaks, view_mask=mask, depth=np.full((h, w), -7.0))
        for k in range(8):
            assert G.same_bits(a["paths"][k], b["paths"][k]), (w, h, K, k)
        assert G.same_bits(a["S"], b["S"]) and np.array_equal(a["labels"], b["labels"])
        assert G.same_bits(a["depth"], b["depth"]) and a["energy"] == b["energy"]
        assert (a["depth"][mask != 1] == -7.0).all()
        sel = a["depth"][mask == 1]
        assert (np.isinf(sel) | (sel > 0)).all()


def test_pairwise_term_is_the_oracles():
    L = O.lib()
    rng = np.random.default_rng(5)
    K = 4
    m = O.mrf_params()
    for trial in range(40):
        pk1 = np.ascontiguousarray(np.stack([rng.uniform(0.95, 1.0, K), rng.uniform(1.0, 4.0, K)], axis=-1))
        pk2 = np.ascontiguousarray(np.stack([rng.uniform(0.95, 1.0, K), rng.uniform(1.0, 4.0, K)], axis=-1))
        if trial % 3 == 0:
            pk1[0] = (0.0, -1.0)
        if trial % 4 == 0:
            pk2[:2] = (0.0, -1.0)
        V = G.smooth_matrix(pk1[None, :, 1], pk2[None, :, 1], m.psi_u)[0]
        for k in range(K + 1):
            for d in range(K + 1):
                want = L.sro_mrf_smooth_cost(C.byref(m), K, O.dptr(pk1), O.dptr(pk2), k, d)
                zq = pk1[k, 1] if k < K else 0.0
                zp = pk2[d, 1] if d < K else 0.0
                got = G.smooth(float(zq), k, float(zp), d, K, m.psi_u)
                assert np.float64(want).view(np.uint64) == np.float64(got).view(np.uint64) == V[k, d].view(np.uint64), (trial, k, d)
        # symmetric bit for bit: a direction and its opposite evaluate the same quotients
        assert G.same_bits(V, G.smooth_matrix(pk2[None, :, 1], pk1[None, :, 1], m.psi_u)[0].T)


def test_energy_is_the_oracles():
    peaks, mask = _case(9, 7, 4)
    ref = G.aggregate(peaks)
    m = O.mrf_params()
    D = G.data_costs(peaks)
    assert ref["energy"] == O.mrf_energy(peaks, ref["labels"], m, data_costs=D)
    zeros = np.zeros((7, 9), np.int32)
    assert G.energy(D, peaks[..., 1], zeros, m.psi_u) == O.mrf_energy(peaks, zeros, m, data_costs=D)


def test_sum_of_single_directions():
    peaks, mask = _case(9, 7, 9)
    full = G.aggregate(peaks)
    for path_mask in (0xFF, 0x0F, 0xA5):
        S = None
        for k in range(8):
            if path_mask >> k & 1:
                one = G.aggregate(peaks, mask=1 << k)
                assert G.same_bits(one["S"], full["paths"][k])
                S = one["S"].copy() if S is None else S + one["S"]
        assert G.same_bits(S, G.aggregate(peaks, mask=path_mask)["S"])


def test_mirror_symmetry():
    """flipping the image swaps the directions pairwise"""
    peaks, mask = _case(9, 7, 4)
    D, z = G.data_costs(peaks), np.ascontiguousarray(peaks[..., 1])
    flip_x = {0: 1, 1: 0, 2: 2, 3: 3, 4: 7, 7: 4, 5: 6, 6: 5}
    flip_y = {0: 0, 1: 1, 2: 3, 3: 2, 4: 6, 6: 4, 5: 7, 7: 5}
    for k in range(8):
        want = G.path(D, z, k, 0.002)
        assert G.same_bits(G.path(D[:, ::-1].copy(), z[:, ::-1].copy(), flip_x[k], 0.002)[:, ::-1], want), k
        assert G.same_bits(G.path(D[::-1].copy(), z[::-1].copy(), flip_y[k], 0.002)[::-1], want), k


def test_no_smoothness_gives_the_per_pixel_argmin():
    peaks, mask = _case(9, 7, 9)
    peaks[..., 1] = 2.5                                                # identical depths: every peak pair costs 0
    D = G.data_costs(peaks)
    one = G.aggregate(peaks, psi_u=0.0, mask=0x01)
    assert G.same_bits(one["S"], D)
    full = G.aggregate(peaks, psi_u=0.0)
    assert np.array_equal(full["labels"], np.argmin(D, axis=2))


def _c40():
    return mrf_cases.peaks_case_fast(40, 28, K=9, seed=40 * 131 + 28, fill=0.6)


def test_regularises_towards_the_trws_energy():
    """the case of the design note: one pass lands between the initial labelling and TRW-S, nearer to TRW-S"""
    peaks, mask = _c40()
    m = O.mrf_params()
    ref = O.mvs_mrf(peaks, mask, m)
    got = G.aggregate(peaks)
    D = G.data_costs(peaks)
    e = O.mrf_energy(peaks, got["labels"], m, data_costs=D)
    print("energy: initial %.2f, TRW-S %.2f (%d sweeps), semi-global %.2f" % (ref["energy_initial"], ref["energy_final"], ref["iterations"], e))
    assert e < 0.5 * (ref["energy_initial"] + ref["energy_final"])
    assert (got["labels"] != np.argmin(D, axis=2)).sum() > 100


def test_ties_are_decided_by_the_lowest_index():
    peaks, mask = _c40()
    got = G.aggregate(peaks, phi_u=2.0)
    two = np.sort(got["S"], axis=2)[..., :2]
    ties = two[..., 0] == two[..., 1]
    print("pixels whose two lowest sums are equal:", int(ties.sum()))
    assert ties.sum() > 10
    first = np.array([[int(np.flatnonzero(got["S"][y, x] == two[y, x, 0])[0]) for x in range(40)] for y in range(28)])
    assert np.array_equal(got["labels"], first)
