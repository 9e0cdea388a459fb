"""The exact predicates as the device evaluates them: slam_delaunay_predicates
runs the star kernel's own orient / incircle / closer wrappers (csrc/delaunay.hip,
with their out-of-line exact paths) and the f64 filters of csrc/exact_pred.h,
one thread per case.  Every sign is compared with fractions.Fraction arithmetic,
and the filter's answers, row for row, with those of the g++ build of the same
header (tests/cpp/exact_pred_test.cpp): with contraction off on both sides the
filters are the same f64 operations, so a difference means that the device
build fuses, flushes or reorders something."""
import shutil

import numpy as np
import pytest

import slamhip
from slamhip import _lib as L
from slamhip import api
from test_exact_pred import (CASES, exact_sign, generate_cases, generate_lifted_cases, parse_cases, read_cases,
                             run_driver)

pytestmark = pytest.mark.gpu

F32 = np.float32


def arrays_of(cases):
    """(kinds, vals n x 8) of [(kind, [Fraction, ...])]: every Fraction is an f32 value"""
    vals = np.zeros((len(cases), 8), F32)
    for r, (_, v) in enumerate(cases):
        vals[r, :len(v)] = [float(x) for x in v]
        assert all(float(vals[r, q]) == x for q, x in enumerate(v))
    return "".join(k for k, _ in cases), vals


def check_signs(cases, want, fs, s):
    """the assertions of test_exact_pred.test_predicates_against_fractions"""
    assert len(fs) == len(s) == len(cases)
    undecided = {"o": 0, "i": 0, "c": 0}
    zeros = {"o": 0, "i": 0, "c": 0}
    for n, ((kind, _), w) in enumerate(zip(cases, want)):
        assert int(s[n]) == w, (n, kind, int(s[n]), w)
        assert int(fs[n]) in (w, 2), (n, kind, "the filter alone returned a wrong sign", int(fs[n]), w)
        undecided[kind] += int(fs[n]) == 2
        zeros[kind] += w == 0
    for kind in "oic":
        assert undecided[kind] >= 50 and zeros[kind] >= 30, (kind, undecided, zeros)
        assert {w for (k, _), w in zip(cases, want) if k == kind} == {-1, 0, 1}


@pytest.fixture(scope="module")
def committed():
    cases = read_cases()
    assert len(cases) == 1580
    kinds, vals = arrays_of(cases)
    return cases, [exact_sign(k, v) for k, v in cases], kinds, vals


def test_device_signs_equal_the_exact_rationals(gpu_ctx, committed):
    cases, want, kinds, vals = committed
    fs, s = api.delaunayPredicates(kinds, vals, ctx=gpu_ctx)
    check_signs(cases, want, fs, s)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_device_filter_equals_the_host_filter_row_for_row(gpu_ctx, committed, tmp_path):
    cases, want, kinds, vals = committed
    host = run_driver(tmp_path, (), "exact_pred_test")
    fs, s = api.delaunayPredicates(kinds, vals, ctx=gpu_ctx)
    assert len(host) == len(cases)
    diff = [(n, cases[n][0], int(fs[n]), host[n][0]) for n in range(len(cases)) if int(fs[n]) != host[n][0]]
    assert not diff, diff[:10]
    assert [int(v) for v in s] == [h[1] for h in host]


def test_a_second_list_under_another_seed(gpu_ctx, committed):
    text = generate_cases(seed=77003)
    cases = parse_cases(text)
    with open(CASES) as f:
        assert text != f.read() and len(cases) > 1500              # not the committed list again
    kinds, vals = arrays_of(cases)
    fs, s = api.delaunayPredicates(kinds, vals, ctx=gpu_ctx)
    check_signs(cases, [exact_sign(k, v) for k, v in cases], fs, s)


def test_incircle_where_the_low_part_of_two_prod_decides(gpu_ctx):
    """the device's fma in two_prod: every row passes the filter undecided, and
    the exact sum is wrong without the low parts (test_exact_pred.generate_lifted_cases)"""
    text = generate_lifted_cases()
    cases = parse_cases(text)
    want = [exact_sign(k, v) for k, v in cases]
    kinds, vals = arrays_of(cases)
    fs, s = api.delaunayPredicates(kinds, vals, ctx=gpu_ctx)
    assert len(cases) == 240 and (fs == 2).all()
    assert [int(v) for v in s] == want
    assert want.count(0) >= 120 and want.count(1) >= 30 and want.count(-1) >= 30


@pytest.mark.parametrize("n", [0, 1, 63, 65])
def test_launch_edges(gpu_ctx, committed, n):
    """sizes that are no multiple of the block (the full list is 1580 = 24 * 64 + 44);
    the exactly cocircular incircle rows lead, so that even n = 1 takes the exact path"""
    cases, want, kinds, vals = committed
    lead = [i for i in range(len(cases)) if kinds[i] == "i" and want[i] == 0]
    rows = (lead + [i for i in range(len(cases)) if not (kinds[i] == "i" and want[i] == 0)])[:n]
    fs, s = api.delaunayPredicates("".join(kinds[i] for i in rows), vals[rows], ctx=gpu_ctx)
    assert len(fs) == len(s) == n
    assert [int(v) for v in s] == [want[i] for i in rows]
    assert all(int(f) in (want[i], 2) for f, i in zip(fs, rows))
    assert n == 0 or int(fs[0]) == 2


def test_argument_checks(gpu_ctx):
    lib = slamhip.lib()
    kinds, vals = np.frombuffer(b"oic", np.uint8).copy(), np.ones((3, 8), F32)
    fs, s = np.full(3, 9, np.int8), np.full(3, 9, np.int8)
    h = gpu_ctx.handle
    assert lib.slam_delaunay_predicates(h, L.ptr(kinds), L.ptr(vals), 0, L.ptr(fs), L.ptr(s)) == L.SLAM_OK
    assert lib.slam_delaunay_predicates(h, L.ptr(kinds), L.ptr(vals), -1, L.ptr(fs), L.ptr(s)) == L.SLAM_E_INVALID_ARG
    assert lib.slam_delaunay_predicates(h, None, L.ptr(vals), 3, L.ptr(fs), L.ptr(s)) == L.SLAM_E_INVALID_ARG
    assert lib.slam_delaunay_predicates(h, L.ptr(kinds), None, 3, L.ptr(fs), L.ptr(s)) == L.SLAM_E_INVALID_ARG
    assert lib.slam_delaunay_predicates(h, L.ptr(kinds), L.ptr(vals), 3, None, L.ptr(s)) == L.SLAM_E_INVALID_ARG
    assert lib.slam_delaunay_predicates(h, L.ptr(kinds), L.ptr(vals), 3, L.ptr(fs), None) == L.SLAM_E_INVALID_ARG
    assert lib.slam_delaunay_predicates(None, L.ptr(kinds), L.ptr(vals), 3, L.ptr(fs), L.ptr(s)) == L.SLAM_E_INVALID_ARG
    bad = np.frombuffer(b"oxc", np.uint8).copy()
    assert lib.slam_delaunay_predicates(h, L.ptr(bad), L.ptr(vals), 3, L.ptr(fs), L.ptr(s)) == L.SLAM_E_INVALID_ARG
    assert (fs == 9).all() and (s == 9).all()                      # nothing written by any of these
    assert lib.slam_delaunay_predicates(h, L.ptr(kinds), L.ptr(vals), 3, L.ptr(fs), L.ptr(s)) == L.SLAM_OK
    assert fs.tolist() == [0, 2, 2] and s.tolist() == [0, 0, 0]    # all points equal: every sign is zero
