"""The adversarial kNN fixtures (tests/knn_cases.py) proved on the CPU: this tests
the fixtures and the exact reference, not the kernel.  Every condition a case
was built for is an assertion here, so tests/test_knn_gpu.py can rely on it."""
import numpy as np
import pytest

import knn_cases as K
import oracle_ffi as O


@pytest.mark.parametrize("name", K.NAMES)
def test_case_reference_and_mode(name):
    c = K.get(name)
    assert len(c.q) >= 1 and c.q.shape[1] == c.t.shape[1] == (32 if c.matcher == K.ORB_BF else 128)
    if c.matcher == K.SIFT_BF:
        for a in (c.q, c.t):
            assert a.min() >= 0 and a.max() <= 255 and np.array_equal(a, np.floor(a))
    # the exact reference equals the oracle bit for bit
    idx, dist = K.knn2_exact(c.q, c.t, c.norm)
    oi, od = O.knn2(c.q, c.t, c.norm)
    np.testing.assert_array_equal(idx, oi)
    np.testing.assert_array_equal(dist, od)
    for r in c.ratios + (0.7,):
        np.testing.assert_array_equal(K.ratio_exact(idx, dist, r), O.ratio(oi, od, r))
    # the case lands in the key mode it names (api.cpp knn_host: s = mq + mt;
    # s > 2048 -> sqrt keys, s^2 < 2^21 - 1 -> packed keys, between them unpacked L2)
    assert K.mode_for(c.q, c.t, c.matcher, c.norm) == c.mode
    if c.matcher == K.SIFT_BF and c.norm == K.NORM_L2:
        s = K.norm_sum(c.q, c.t)
        lo, hi = {K.MODE_L2P: (0.0, np.sqrt(2.0 ** 21 - 1)), K.MODE_L2: (np.sqrt(2.0 ** 21 - 1), 2048.0),
                  K.MODE_SQRT: (2048.0, 1e9)}[c.mode]
        assert (lo <= s <= hi) if c.mode == K.MODE_L2 else (lo <= s < hi) if c.mode == K.MODE_L2P else (lo < s)
    # what the case was constructed to give is what the reference gives
    if c.expect is not None:
        n = len(c.expect[0])
        np.testing.assert_array_equal(idx[:n], c.expect[0])
        np.testing.assert_array_equal(dist[:n], c.expect[1])
    # the matrix form of d^2 equals the direct sum (small cases)
    if c.norm == K.NORM_L2 and len(c.t) <= 5000:
        np.testing.assert_array_equal(K.distances_exact(c.q, c.t, c.norm),
                                      np.sqrt(K.sq_dist_exact(c.q, c.t).astype(np.float32)))


def test_registry_covers_the_issue_list():
    assert len(set(K.NAMES)) == len(K.NAMES)
    assert len(K.SWEEP_PAIRS) == len(set(K.SWEEP_PAIRS)) == 24
    assert {p[0] for p in K.SWEEP_PAIRS} == set(K.SWEEP_NQ) and {p[1] for p in K.SWEEP_PAIRS} == set(K.SWEEP_NT)
    for fam in ("pk", "l2", "sqrt", "ham"):
        for step, nt in ((4, 200), (32, 200), (64, 330)):
            assert f"seam_ties-{fam}-{nt}-{step}" in K.NAMES and f"seam_ties-{fam}-{nt}-{step}-swapped" in K.NAMES
    for fam in ("pk", "ham"):
        for nt in (65536, 65537):
            assert f"seam_ties-{fam}-{nt}-1024" in K.BIG and f"seam_ties-{fam}-{nt}-1024-swapped" in K.BIG
    for fam in K.FAMILIES:
        assert all(f"all_equal-{fam}-{nt}" in K.NAMES for nt in (2, 5, 33, 65, 1025))
    assert set(K.VARIANT_NAMES) < set(K.NAMES) and set(K.BIG) < set(K.VARIANT_NAMES)


def test_row_with_sqnorm_exact():
    rng = np.random.default_rng(0)
    ns = list(range(0, 300)) + [int(x) for x in rng.integers(0, 1 << 22, 300)] + [(1 << 21) - 2, (1 << 22) - 1,
                                                                                 6000299, 128 * 255 * 255]
    for n in ns:
        r = K.row_with_sqnorm(n)
        assert r.shape == (128,) and r.min() >= 0 and r.max() <= 255
        assert int((r.astype(np.int64) ** 2).sum()) == n


def test_mode_edges_straddle_the_thresholds():
    n = K._edge_sqnorm()
    assert (1024.0 + np.sqrt(float(n - 1))) ** 2 < 2.0 ** 21 - 1 <= (1024.0 + np.sqrt(float(n))) ** 2
    s = {x: K.norm_sum(K.get(f"mode_edges-{x}").q, K.get(f"mode_edges-{x}").t)
         for x in ("below_packed", "above_packed", "sum_2048", "above_2048")}
    assert s["below_packed"] ** 2 < 2.0 ** 21 - 1 <= s["above_packed"] ** 2
    assert s["above_packed"] - s["below_packed"] < 2e-3
    assert s["sum_2048"] == 2048.0 and 2048.0 < s["above_2048"] < 2048.2
    for x in s:
        assert len(K.get(f"mode_edges-{x}").t) >= 2


def test_adjacent_d2_below_2p22():
    """all 300 consecutive d^2 below 2^22 have distinct f32 roots: ranking by d^2 is ranking by distance"""
    v = (1 << 22) - 300 + np.arange(300)
    assert len(np.unique(np.sqrt(v.astype(np.float32)))) == 300
    c = K.get("adjacent_d2_below_2p22")
    d2 = K.sq_dist_exact(c.q, c.t)[0]
    assert set(v.tolist()) <= set(d2.tolist())
    idx, dist = K.knn2_exact(c.q, c.t, c.norm)
    assert sorted(d2[idx[0]].tolist()) == sorted(d2.tolist())[:2] and dist[0, 0] < dist[0, 1]


def test_adjacent_d2_sqrt_ties_conditions():
    v = K.SQRT_TIES_BASE + np.arange(300)
    r = np.sqrt(v.astype(np.float32))
    eq = r[1:] == r[:-1]
    share = np.zeros(300, bool)
    share[1:] |= eq
    share[:-1] |= eq
    assert len(np.unique(r)) == 251 and share.sum() >= 40        # 49 collisions, 98 values share a root
    # from 6,000,000 the three smallest roots are distinct: no shuffle shows a tie in the top two
    assert K.sqrt_ties_seed(K.SQRT_TIES_BASE) is None
    # from 6,000,002 the two smallest d^2 share a root and the larger sits at the lower index
    assert K.sqrt_ties_seed(K.SQRT_TIES_BASE_TOP2) is not None
    c = K.get(f"adjacent_d2_sqrt_ties-{K.SQRT_TIES_BASE_TOP2}")
    d2 = K.sq_dist_exact(c.q[:1], c.t)[0]
    assert sorted(d2.tolist()) == list(range(K.SQRT_TIES_BASE_TOP2, K.SQRT_TIES_BASE_TOP2 + 300))
    idx, dist = K.knn2_exact(c.q, c.t, c.norm)
    i0, i1 = idx[0]
    assert dist[0, 0] == dist[0, 1] and i0 < i1 and d2[i0] == d2[i1] + 1 == K.SQRT_TIES_BASE_TOP2 + 1
    by_d2 = np.lexsort((np.arange(300), d2))[:2]
    assert by_d2.tolist() == [i1, i0]                            # a d^2-ranking kernel returns them swapped
    for base in (K.SQRT_TIES_BASE, K.SQRT_TIES_BASE_TOP2):
        assert K.norm_sum(*K.get(f"adjacent_d2_sqrt_ties-{base}")[1:3]) > 2048.0


def test_field_extremes_fields():
    """the packed field d^2 - |q'|^2 + 2^21 (q' = q - 128) of each case's best rows"""
    def field(c):
        idx, _ = K.knn2_exact(c.q, c.t, c.norm)
        d2 = K.sq_dist_exact(c.q, c.t)
        qn = ((c.q.astype(np.int64) - 128) ** 2).sum(1)
        return d2[np.arange(len(c.q)), idx[:, 0]] - qn + (1 << 21), d2
    f, _ = field(K.get("field_extremes-zeros"))
    assert np.all(f == 0)
    f, d2 = field(K.get("field_extremes-all127"))
    assert np.all(f > (1 << 22) - (1 << 16)) and np.all(f < 1 << 22) and d2.max() < (1 << 21) - 1
    f, d2 = field(K.get("field_extremes-d2_limit"))
    assert d2.max() == (1 << 21) - 2 and np.all(f < 1 << 22)


def test_ratio_edge_is_an_equality():
    assert K.RATIO_EQ * 4.0 == 3.0 and K.RATIO_ABOVE * 4.0 > 3.0 and K.RATIO_ABOVE > K.RATIO_EQ
    for fam in ("pk", "l1", "ham"):
        c = K.get(f"ratio_edge-{fam}")
        idx, dist = K.knn2_exact(c.q, c.t, c.norm)
        assert len(K.ratio_exact(idx, dist, K.RATIO_EQ)) == 0 and len(K.ratio_exact(idx, dist, K.RATIO_ABOVE)) == 1
        c = K.get(f"ratio_edge_700-{fam}")
        m = K.ratio_exact(*K.knn2_exact(c.q, c.t, c.norm), K.RATIO_EQ)
        assert len(c.q) == 700 and m["queryIdx"].tolist() == list(range(0, 700, 3))


def test_hamming_and_l1_extremes_reach_the_extremes():
    c = K.get("hamming_extremes-small")
    d = K.distances_exact(c.q, c.t, c.norm)
    assert {0.0, 1.0, 2.0, 256.0} <= set(d.ravel().tolist())
    c = K.get("hamming_extremes-65536")
    assert c.expect[0][1, 0] % 1024 == 1023 and c.expect[0][0, 0] == c.expect[0][1, 0] + 1
    assert K.distances_exact(c.q[:1], c.t[c.expect[0][1, 0]][None], c.norm)[0, 0] == 256
    c = K.get("l1_extremes-32640")
    assert K.distances_exact(c.q, c.t, c.norm)[0, 0] == 32640 == 128 * 255
    c = K.get("l1_extremes-tile_ties")
    idx, dist = K.knn2_exact(c.q, c.t, c.norm)
    assert idx[0].tolist() == [20, 63] and dist[0].tolist() == [0, 0] and 1.0 in dist.ravel().tolist()


def test_expected_variant_table():
    assert K.expected_variant(K.MODE_L2P) == K.V_PK_QT2 and K.expected_variant(K.MODE_HAMP) == K.V_PK_QT2
    assert K.expected_variant(K.MODE_L2P, pipe=1) == K.expected_variant(K.MODE_HAMP, pipe=1) == K.V_PIPE_QT2
    assert K.expected_variant(K.MODE_L2P, pipe=2) == K.V_PIPE_QT1
    assert K.expected_variant(K.MODE_L2P, pipe=3) == K.V_PK_QT1
    assert K.expected_variant(K.MODE_L2P, xcd=1) == K.V_PK_QT2 | K.V_XCD
    assert K.expected_variant(K.MODE_L2, pipe=1, xcd=1) == K.expected_variant(K.MODE_SQRT) == K.V_MFMA
    assert K.expected_variant(K.MODE_L1P, pipe=2) == K.V_L1
