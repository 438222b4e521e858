"""No-GPU checks of the ensemble feature: the numpy / integer reference (tests/_fuse_ref.py) against a brute-force loop over the
samples, its gradient and Hessian against central differences of its own NLL, its Newton fit against scipy and on separable data;
the two summation orders that the cap of tests/test_fuse_gpu.py's score comparison rests on; the ABI constants, the argument checks
of the new entry points through the raw ABI (nothing is launched) and dfd_fuse_plan at both sides of its boundaries; the diversity
figures from integer tables; and the orchestrator's `ensemble:` key, parsed and on a CPU device."""

from __future__ import annotations

import ctypes
import json
import math

import numpy as np
import pytest
import torch

from deepfakedetection_amd import _lib
from deepfakedetection_amd import metrics as M
from tests import _fuse_ref as R


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        from deepfakedetection_amd.build import build

        build()
    return _lib.load()


# ------------------------------------------------------------------ the reference against a loop over the samples
def _brute_nll(zs, targets, a):
    K = len(zs)
    out = [[] for _ in range(R.terms(K))]
    for i, y in enumerate(targets.tolist()):
        rows = [z[i].tolist() for z in zs]
        if any(math.isnan(v) or math.isinf(v) for row in rows for v in row) or not 0 <= y < len(rows[0]):
            continue
        J = len(rows[0])
        f = [math.fsum(a[k] * rows[k][j] for k in range(K)) for j in range(J)]
        m = max(f)
        e = [math.exp(v - m) for v in f]
        s = math.fsum(e)
        mean = [math.fsum(e[j] * rows[k][j] for j in range(J)) / s for k in range(K)]
        out[0].append(m + math.log(s) - f[y])
        o = 1 + K
        for k in range(K):
            out[1 + k].append(mean[k] - rows[k][y])
            for l in range(k, K):
                out[o].append(math.fsum(e[j] * rows[k][j] * rows[l][j] for j in range(J)) / s - mean[k] * mean[l])
                o += 1
    return [math.fsum(v) for v in out]


@pytest.mark.parametrize("n,J,K", [(1, 2, 1), (200, 2, 2), (200, 3, 3), (60, 17, 2), (100, 2, 8)])
def test_nll_reference_equals_brute_force(n, J, K):
    zs, y = R.members_case(n + J + K, n, J, K)
    if n > 10:
        zs[0][2, 0], zs[K - 1][4, J - 1] = np.nan, -np.inf                     # one member only
        y[6], y[8] = -1, J
    cands = [[1.0 / K] * K, R.capped_coef(zs, 5)]
    ref = R.nll(zs, y, cands)
    assert ref.stats == ([2, 2] if n > 10 else [0, 0]) and ref.valid == n - sum(ref.stats)
    assert ref.out.shape == (2, R.terms(K)) and R.terms(8) == _lib.FUSE_MAX_TERMS
    for c, a in enumerate(cands):
        want = _brute_nll(zs, y, a)
        for o in range(R.terms(K)):
            assert abs(ref.out[c, o] - want[o]) <= R.sum_bound(ref.mag[c, o], 1, R.fuse_per_row(J, K, ref.amax[c])), (c, o)


@pytest.mark.parametrize("J,K", [(2, 1), (2, 3), (5, 2), (17, 8)])
def test_gradient_and_hessian_are_the_derivatives_of_the_reference_nll(J, K):
    zs, y = R.members_case(J * K, 150, J, K, scale=1.0)
    a = np.random.default_rng(J + K).uniform(0.1, 0.6, size=K)
    _, g, H = R.unpack(R.nll(zs, y, [a]).out[0], K)
    eps = 1e-5
    for k in range(K):
        step = np.zeros(K)
        step[k] = eps
        up, down = R.nll(zs, y, [a + step, a - step]).out
        assert abs((up[0] - down[0]) / (2 * eps) - g[k]) <= 1e-6 * max(1.0, abs(g[k])), k
        g_up, g_down = R.unpack(up, K)[1], R.unpack(down, K)[1]
        assert np.all(np.abs((g_up - g_down) / (2 * eps) - H[k]) <= 1e-6 * np.maximum(1.0, np.abs(H[k]))), k
    assert np.all(np.linalg.eigvalsh(H) >= -1e-9 * np.abs(H).max())             # a covariance, summed: positive semi-definite


def _brute_scores(zs, coef, mode, beta):
    K, (n, J) = len(zs), zs[0].shape
    probs = np.zeros((n, J))
    for i in range(n):
        rows = [z[i].astype(np.float64) for z in zs]
        if mode == R.LOGIT:
            f = [math.fsum(coef[k] * float(rows[k][j]) for k in range(K)) for j in range(J)]
            m = max(f)
            s = math.fsum(math.exp(v - m) for v in f)
            probs[i] = [math.exp(v - m) / s for v in f]
        else:
            for k in range(K):
                b = [beta[k] * float(v) for v in rows[k]]
                m = max(b)
                s = math.fsum(math.exp(v - m) for v in b)
                probs[i] += [coef[k] * math.exp(v - m) / s for v in b]
    return probs


@pytest.mark.parametrize("mode", [R.LOGIT, R.PROB])
@pytest.mark.parametrize("n,J,K", [(50, 2, 3), (40, 17, 2), (30, 3, 8)])
def test_scores_reference_equals_brute_force(n, J, K, mode):
    zs, _ = R.members_case(n + J, n, J, K)
    coef = R.capped_coef(zs, 3) if mode == R.LOGIT else (np.arange(1, K + 1) / (K * (K + 1) / 2)).tolist()
    beta = [0.5 + 0.25 * k for k in range(K)]
    zs[1 % K][5, 1] = np.nan
    probs, preds, fused, nonfinite = R.scores(zs, coef, mode, beta)
    assert nonfinite == 1 and np.isnan(probs[5]).all() and np.isnan(fused[5]).all() and preds[5] == 0
    keep = np.arange(n) != 5
    want = _brute_scores([z[keep] for z in zs], coef, mode, beta)
    assert np.all(np.abs(probs[keep] - want) <= 2.0 ** -23 * want + 1e-45) and np.array_equal(preds[keep], probs[keep].argmax(axis=1))
    assert np.allclose(probs[keep].sum(axis=1), 1.0, atol=1e-6)
    if mode == R.LOGIT:
        assert np.array_equal(fused[keep], R.pool(R.stack(zs)[:, keep], coef).astype(np.float32))
    else:
        assert np.allclose(fused[keep], np.log(want), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("K,J", R.SHAPES)
def test_two_summation_orders_stay_within_the_cap_of_the_scores_test(K, J):
    """tests/test_fuse_gpu.py lets the stored probabilities differ from this reference by at most 1 ulp on at most 1 element in
    1000: the kernel's f64 error is about 1e-14 relative, so only a value that close to a rounding tie of f32 (spacing 6e-8
    relative) lands on the other side, about 2e-6 of the elements.  That cap is a condition, not a measurement: here the
    reference itself, evaluated in two summation orders (a difference of the same size as the kernel's), stays within it on the
    very inputs of that test, and every probability is a normal f32."""
    from deepfakedetection_amd import kernels

    sizes = R.sizes(kernels.fuse_plan(1, J, K).rows, kernels.FUSE_STAGE2_WIDTH)
    zs, coef = R.score_case(K, J, sizes[-1])
    assert sum(abs(c) * np.abs(z.astype(np.float64)) for c, z in zip(coef, zs)).max() <= 30.0
    for mode, a in ((R.LOGIT, coef), (R.PROB, R.ramp_weights(K))):
        one, _, _, _ = R.scores(zs, a, mode, R.ramp_betas(K))
        two, _, _, _ = R.scores(zs, a, mode, R.ramp_betas(K), reverse=True)
        assert np.all(one >= np.finfo(np.float32).tiny) and np.all(two >= np.finfo(np.float32).tiny)
        for n in sizes:                                                         # the test slices the last n rows of this case
            differ, worst = R.ulp_mismatches(one[-n:], two[-n:])
            assert worst <= 1 and differ * 1000 <= n * J, (mode, n, differ, worst)


# ------------------------------------------------------------------ the reference fit
@pytest.mark.parametrize("K,J,n", [(1, 2, 65), (2, 3, 257), (3, 2, 2049), (8, 17, 257), (3, 65, 65), (8, 2, 2049)])
def test_reference_fit_converges_on_data_that_are_not_separable(K, J, n):
    zs, y = R.members_case(K * 1000 + J + n, n, J, K, scale=1.0 if K * J > 100 else 3.0)
    fit = R.fit(zs, y)
    assert fit.converged and not fit.at_bound and 1 <= fit.iterations <= 12 and fit.nll_after <= fit.nll_before
    _, g, H = R.unpack(R.nll(zs, y, [fit.coef]).out[0], K)
    assert np.abs(g).max() / n <= 1e-10 and np.all(np.linalg.eigvalsh(H) > 0.0)
    ridge = R.fit(zs, y, l2=1e-2)
    assert ridge.converged and ridge.nll_after >= fit.nll_after - 1e-12           # the ridge pulls away from the minimum of the NLL


@pytest.mark.parametrize("n", [65, 257])
def test_reference_fit_on_separable_data_grows_until_it_is_stopped(n):
    zs, y = R.separable_case(n)
    fit = R.fit(zs, y)
    assert not fit.converged and fit.at_bound and max(abs(c) for c in fit.coef) > 32.0 and fit.iterations <= 30
    ridge = R.fit(zs, y, l2=1e-2)
    assert ridge.converged and not ridge.at_bound                               # the same data have a minimum under the ridge


def test_reference_fit_agrees_with_scipy():
    optimize = pytest.importorskip("scipy.optimize")
    zs, y = R.members_case(77, 3000, 3, 3)
    fit = R.fit(zs, y)

    def value_and_gradient(a):
        value, g, _ = R.unpack(R.nll(zs, y, [a]).out[0], 3)
        return value, g

    res = optimize.minimize(value_and_gradient, np.full(3, 1.0 / 3), jac=True, method="BFGS", options={"gtol": 1e-9})
    assert np.all(np.abs(res.x - np.array(fit.coef)) <= 1e-6) and fit.nll_after * fit.valid <= res.fun + 1e-9


def test_device_fit_runs_the_reference_steps():
    """metrics.newton_fusion (the host loop of fit_fusion) on the reference's evaluations takes the reference fit's steps."""
    for zs, y, l2 in (R.members_case(5, 500, 3, 3) + (0.0,), R.members_case(6, 300, 2, 4) + (1e-2,), R.separable_case(257) + (0.0,)):
        K = len(zs)

        def evaluate(cands):
            res = R.nll(zs, y, cands)
            return [M.unpack_fusion_terms(row, K) for row in res.out], res.valid

        coef, before, after, iterations, at_bound, converged, valid = M.newton_fusion(evaluate, [1.0 / K] * K, l2, 32.0)
        ref = R.fit(zs, y, l2=l2)
        assert (coef, iterations, at_bound, converged, valid) == (ref.coef, ref.iterations, ref.at_bound, ref.converged, ref.valid)
        assert (before / valid, after / valid) == (ref.nll_before, ref.nll_after)


# ------------------------------------------------------------------ agreement tables and diversity
def test_agree_reference_and_diversity_figures():
    rng = np.random.default_rng(4)
    n, J, K = 500, 3, 4
    y = rng.integers(0, J, size=n)
    preds = [np.where(rng.random(n) < 0.5 + 0.1 * k, y, (y + 1) % J) for k in range(K)]
    y[:7] = [-1, J, 5, -9, J + 1, 99, -2]
    pair, hist, stats = R.agree(preds, y, J)
    assert stats == [n - 7, 7] and sum(hist) == n - 7
    for a in range(K):
        assert pair[a][a][1] == pair[a][a][2] == 0
        for b in range(K):
            assert sum(pair[a][b]) == n - 7 and pair[a][b][1] == pair[b][a][2]
            assert pair[a][b] == [sum(1 for i in range(7, n) if (preds[a][i] == y[i]) == ra and (preds[b][i] == y[i]) == rb)
                                  for ra, rb in ((True, True), (True, False), (False, True), (False, False))]
    div = M.diversity_from_counts(pair, hist, stats[0])
    right = np.array([[p[i] == y[i] for i in range(7, n)] for p in preds])
    assert div.accuracy == [int(r.sum()) / (n - 7) for r in right]
    assert div.oracle_accuracy == int(right.any(axis=0).sum()) / (n - 7)
    assert div.majority_accuracy == int((right.sum(axis=0) * 2 > K).sum()) / (n - 7)
    for a in range(K):
        assert div.disagreement[a][a] == 0.0 and div.kappa[a][a] == 1.0 and div.yule_q[a][a] == 1.0
        for b in range(K):
            po = (right[a] == right[b]).mean()
            pe = right[a].mean() * right[b].mean() + (1 - right[a].mean()) * (1 - right[b].mean())
            assert abs(div.kappa[a][b] - (po - pe) / (1 - pe)) <= 1e-12 and abs(div.disagreement[a][b] - (1 - po)) <= 1e-12
            assert div.double_fault[a][b] == int((~right[a] & ~right[b]).sum()) / (n - 7)
    empty = M.diversity_from_counts([[[0, 0, 0, 0]]], [0, 0], 0)
    assert empty.accuracy == [None] and empty.oracle_accuracy is None and empty.kappa == [[None]] and empty.yule_q == [[None]]
    always = M.diversity_from_counts([[[9, 0, 0, 0]]], [0, 9], 9)                # never wrong: Q and kappa have no denominator
    assert always.accuracy == [1.0] and always.yule_q == [[None]] and always.kappa == [[None]] and always.double_fault == [[0.0]]


# ------------------------------------------------------------------ the ABI without a device
def test_abi_constants_and_sources(lib):
    from deepfakedetection_amd.build import SOURCES

    assert lib.dfd_version() >= 151 and "dfd_fuse.hip" in SOURCES
    header = (_lib.LIB_PATH.parents[1] / "include" / "dfd_hip.h").read_text()
    for name, value in (("DFD_FUSE_MAX_MODELS", _lib.FUSE_MAX_MODELS), ("DFD_FUSE_MAX_CANDS", _lib.FUSE_MAX_CANDS),
                        ("DFD_FUSE_MAX_J", _lib.FUSE_MAX_J), ("DFD_FUSE_MAX_TERMS", _lib.FUSE_MAX_TERMS),
                        ("DFD_FUSE_THREAD_MAX_KJ", _lib.FUSE_THREAD_MAX_KJ), ("DFD_FUSE_MAX_BLOCKS", _lib.FUSE_MAX_BLOCKS),
                        ("DFD_FUSE_STAGE2_WIDTH", _lib.FUSE_STAGE2_WIDTH), ("DFD_FUSE_LAYOUT_THREAD", _lib.FUSE_LAYOUT_THREAD),
                        ("DFD_FUSE_LAYOUT_WAVE", _lib.FUSE_LAYOUT_WAVE), ("DFD_FUSE_LOGIT", _lib.FUSE_LOGIT), ("DFD_FUSE_PROB", _lib.FUSE_PROB)):
        assert f"#define {name} {value}\n" in header, name
    assert "#define DFD_FUSE_MAX_N (1 << 28)" in header and _lib.FUSE_MAX_N == 1 << 28
    assert (_lib.FUSE_MAX_MODELS, _lib.FUSE_MAX_CANDS, _lib.FUSE_MAX_J) == (8, 8, 1024)
    assert " * 151 = dfd_fuse_scores" in header
    for name in ("DiversityResult", "FusionFit", "diversity", "fit_fusion", "fuse"):
        assert name in M.__all__ and hasattr(M, name)


def test_bad_arguments_are_rejected_without_a_gpu(lib):
    EINVAL, EWORKSPACE = -1, -4
    one, big = 0x1000, 1 << 30                                      # a non-null address: rejected calls launch nothing
    MAX_N, MAX_J, MAX_K, MAX_C = _lib.FUSE_MAX_N, _lib.FUSE_MAX_J, _lib.FUSE_MAX_MODELS, _lib.FUSE_MAX_CANDS
    ptrs = (ctypes.c_void_p * 9)(*([one] * 9))
    holed = (ctypes.c_void_p * 3)(one, None, one)
    d = lambda *v: (ctypes.c_double * len(v))(*v)                   # noqa: E731
    shapes = ((-1, 2, 3), (MAX_N + 1, 2, 3), (8, 0, 3), (8, MAX_J + 1, 3), (8, 2, 0), (8, 2, MAX_K + 1))
    # dfd_fuse_scores(ptrs, K, n, J, mode, coef, beta, probs, logits_out, preds, stats, stream)
    third, ones = d(0.25, 0.25, 0.5), d(1.0, 1.0, 1.0)
    for n, J, K in shapes:
        assert lib.dfd_fuse_scores(ptrs, K, n, J, 0, d(*([0.1] * 9)), None, one, one, one, one, None) == EINVAL, (n, J, K)
    for mode in (-1, 2):
        assert lib.dfd_fuse_scores(ptrs, 3, 8, 2, mode, third, ones, one, one, one, one, None) == EINVAL
    assert lib.dfd_fuse_scores(None, 3, 8, 2, 0, third, ones, one, one, one, one, None) == EINVAL
    assert lib.dfd_fuse_scores(holed, 3, 8, 2, 0, third, ones, one, one, one, one, None) == EINVAL
    assert lib.dfd_fuse_scores(ptrs, 3, 8, 2, 0, None, ones, one, one, one, one, None) == EINVAL
    assert lib.dfd_fuse_scores(ptrs, 3, 8, 2, 1, third, None, one, one, one, one, None) == EINVAL          # the linear pool reads beta
    assert lib.dfd_fuse_scores(ptrs, 3, 8, 2, 0, third, ones, one, one, None, one, None) == EINVAL         # preds
    assert lib.dfd_fuse_scores(ptrs, 3, 8, 2, 0, third, ones, one, one, one, None, None) == EINVAL         # stats
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.dfd_fuse_scores(ptrs, 3, 8, 2, 0, d(0.5, bad, 0.5), ones, one, one, one, one, None) == EINVAL, bad
        assert lib.dfd_fuse_scores(ptrs, 3, 8, 2, 1, third, d(1.0, bad, 1.0), one, one, one, one, None) == EINVAL, bad
    for coef in (d(0.5, -0.25, 0.75), d(0.25, 0.25, 0.25), d(0.5, 0.5, 1e-9)):                              # negative, short, long
        assert lib.dfd_fuse_scores(ptrs, 3, 8, 2, 1, coef, ones, one, one, one, one, None) == EINVAL
    for beta in (d(1.0, 0.0, 1.0), d(1.0, -2.0, 1.0)):
        assert lib.dfd_fuse_scores(ptrs, 3, 8, 2, 1, third, beta, one, one, one, one, None) == EINVAL
    # dfd_fuse_nll(ptrs, K, targets, n, J, cands (host), C, ws, ws_bytes, out, stats, stream)
    cands = d(*([0.1] * 72))
    for n, J, K in shapes:
        assert lib.dfd_fuse_nll_ws(n, J, K, 2) == 0 and lib.dfd_fuse_nll(ptrs, K, one, n, J, cands, 2, one, big, one, one, None) == EINVAL
    for C in (0, MAX_C + 1):
        assert lib.dfd_fuse_nll_ws(8, 2, 3, C) == 0 and lib.dfd_fuse_nll(ptrs, 3, one, 8, 2, cands, C, one, big, one, one, None) == EINVAL
    assert lib.dfd_fuse_nll_ws(8, 2, 3, 2) == (2 * 10 + 2) * 8 and lib.dfd_fuse_nll_ws(0, 2, 8, 8) == (8 * 45 + 2) * 8
    assert lib.dfd_fuse_nll(None, 3, one, 8, 2, cands, 2, one, big, one, one, None) == EINVAL
    assert lib.dfd_fuse_nll(holed, 3, one, 8, 2, cands, 2, one, big, one, one, None) == EINVAL
    for hole in range(5):                                           # targets, cands, ws, out, stats
        args = [one, cands, one, one, one]
        args[hole] = None
        assert lib.dfd_fuse_nll(ptrs, 3, args[0], 8, 2, args[1], 2, args[2], big, args[3], args[4], None) == EINVAL, hole
    for bad in (float("nan"), float("inf")):
        assert lib.dfd_fuse_nll(ptrs, 3, one, 8, 2, d(0.1, 0.1, 0.1, 0.1, bad, 0.1), 2, one, big, one, one, None) == EINVAL
    assert lib.dfd_fuse_nll(ptrs, 3, one, 8, 2, cands, 2, one, lib.dfd_fuse_nll_ws(8, 2, 3, 2) - 1, one, one, None) == EWORKSPACE
    # dfd_fuse_agree(pred_ptrs, K, targets, n, J, pair, hist, stats, stream)
    for n, J, K in shapes:
        assert lib.dfd_fuse_agree(ptrs, K, one, n, J, one, one, one, None) == EINVAL, (n, J, K)
    assert lib.dfd_fuse_agree(None, 3, one, 8, 2, one, one, one, None) == EINVAL
    assert lib.dfd_fuse_agree(holed, 3, one, 8, 2, one, one, one, None) == EINVAL
    for hole in range(4):                                           # targets, pair, hist, stats
        args = [one] * 4
        args[hole] = None
        assert lib.dfd_fuse_agree(ptrs, 3, args[0], 8, 2, args[1], args[2], args[3], None) == EINVAL, hole
    # dfd_fuse_plan(n, J, K, out)
    out = (ctypes.c_int * 4)()
    for n, J, K in shapes:
        assert lib.dfd_fuse_plan(n, J, K, out) == EINVAL, (n, J, K)
    assert lib.dfd_fuse_plan(8, 2, 3, None) == EINVAL


def test_plan_on_both_sides_of_every_boundary():
    from deepfakedetection_amd import kernels as K

    T, W = K.FUSE_LAYOUT_THREAD, K.FUSE_LAYOUT_WAVE
    edge = K.FUSE_THREAD_MAX_KJ
    for members, J, layout in ((1, edge, T), (1, edge + 1, W), (2, edge // 2, T), (2, edge // 2 + 1, W), (8, 2, T), (8, 3, W),
                               (4, 4, T), (3, 5, T), (3, 6, W), (1, 1, T), (8, K.FUSE_MAX_J, W)):      # the layout boundary is in K J
        assert K.fuse_plan(100, J, members).layout == layout, (members, J)
    for members, J, layout in ((3, 2, T), (8, 2, T), (2, 17, W), (8, 1000, W)):
        rows = K.fuse_plan(1, J, members).rows
        assert rows == (256 if layout == T else 32)
        assert K.fuse_plan(0, J, members) == K.FusePlan(layout, rows, 1, 1)                             # an empty input: one workgroup
        assert K.fuse_plan(rows, J, members).blocks == 1 and K.fuse_plan(rows + 1, J, members).blocks == 2
        width = K.FUSE_STAGE2_WIDTH
        assert K.fuse_plan(width * rows, J, members) == K.FusePlan(layout, rows, width, 1)              # a second stage-2 trip
        assert K.fuse_plan(width * rows + 1, J, members) == K.FusePlan(layout, rows, width + 1, 2)
        cap = K.FUSE_MAX_BLOCKS
        assert K.fuse_plan(cap * rows, J, members).blocks == cap and K.fuse_plan(cap * rows + 1, J, members).blocks == cap
        assert K.fuse_plan(K.FUSE_MAX_N, J, members) == K.FusePlan(layout, rows, cap, cap // width)
    with pytest.raises(RuntimeError, match="DFD_EINVAL"):
        K.fuse_plan(8, 2, K.FUSE_MAX_MODELS + 1)
    with pytest.raises(ValueError):
        K.fuse_nll_ws(8, 2, 3, K.FUSE_MAX_CANDS + 1)
    assert K.fuse_terms(1) == 3 and K.fuse_terms(3) == 10 and K.fuse_terms(8) == _lib.FUSE_MAX_TERMS


# ------------------------------------------------------------------ the orchestrator's key
def test_ensemble_settings_parse():
    from pathlib import Path

    from rich.console import Console

    from deepfakedetection_amd.orchestration.orchestrator import EnsembleSettings, ensemble_settings

    out = Console(file=open("/dev/null", "w"))                      # noqa: SIM115
    base = {"models": {"a": {}, "b": {}, "c": {}}, "selection": ["a", "b"]}
    parse = lambda block: ensemble_settings({**base, "ensemble": block}, out)   # noqa: E731
    assert ensemble_settings(base, out) is None and parse(None) is None and parse(False) is None
    assert parse({}) == parse(True) == EnsembleSettings(("a", "b"), "logit", "fit", 0.0, Path("runs/ensemble"))
    assert parse({"members": ["b", "a"], "mode": "prob", "output_dir": "x/y"}) == EnsembleSettings(("b", "a"), "prob", "equal", 0.0, Path("x/y"))
    assert parse({"weights": [0.25, 0.75], "mode": "prob"}).weights == (0.25, 0.75)
    assert parse({"weights": [2, -1], "l2": 0.5}) == EnsembleSettings(("a", "b"), "logit", (2.0, -1.0), 0.5, Path("runs/ensemble"))
    assert parse({"weights": "equal", "members": ["a"]}).members == ("a",)
    assert ensemble_settings({"models": {"a": {}, "b": {}}, "ensemble": {}}, out).members == ("a", "b")       # no selection: every model
    for bad in (15, "on", {"members": []}, {"members": ["a", "c"]}, {"members": ["a", "z"]}, {"members": ["a", "a"]}, {"members": "a"},
                {"mode": "vote"}, {"weights": "best"}, {"weights": [1.0]}, {"weights": [0.5, float("nan")]}, {"weights": ["x", "y"]},
                {"mode": "prob", "weights": "fit"}, {"mode": "prob", "weights": [0.5, 0.6]}, {"mode": "prob", "weights": [1.5, -0.5]},
                {"l2": -1}, {"l2": float("inf")}):
        with pytest.raises(ValueError, match="ensemble"):
            parse(bad)


def test_orchestrator_skips_the_ensemble_off_device(tmp_path, capsys, monkeypatch):
    """The networks run on a HIP device only, so a small torch model stands in for the checkpoint: what is under test is the job
    around it.  On a CPU device nothing keeps scores for the ensemble: it warns, and the members run as without the key."""
    import yaml
    from PIL import Image

    from deepfakedetection_amd.orchestration import orchestrator as O

    torch.manual_seed(0)
    stand_in = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(2), torch.nn.Flatten(), torch.nn.Linear(12, 2)).eval()
    monkeypatch.setattr(O, "load_model", lambda *args, **kwargs: stand_in)
    rng = np.random.default_rng(5)
    for split in ("val", "test"):
        for cls in ("fake", "real"):
            folder = tmp_path / "data" / split / cls
            folder.mkdir(parents=True)
            for i in range(2):
                Image.fromarray(rng.integers(0, 256, size=(24, 24, 3), dtype=np.uint8)).save(folder / f"{cls}_{i}.png")
    rows = {}
    for out, ensemble in (("plain", None), ("fused", {"weights": "equal", "output_dir": str(tmp_path / "fused" / "ensemble")})):
        infer = {"split": "test", "batch_size": 4, "num_workers": 0, "img_size": 32, "device_metrics": True}
        cfg = {"seed": 1, "device": "cpu",
               "data": {"root": str(tmp_path / "data"), "val_split": "val", "test_split": "test", "num_classes": 2, "img_size": 32},
               "models": {name: {"output_dir": str(tmp_path / out / name), "inference": infer} for name in ("efficientnet_b0", "efficientnet_b3")}}
        if ensemble is not None:
            cfg["ensemble"] = ensemble
        path = tmp_path / f"{out}.yaml"
        path.write_text(yaml.safe_dump(cfg))
        O.orchestrate(path, mode="inference")
        text = capsys.readouterr().out
        assert ("ensemble skipped" in text) == (out == "fused") and ("kept no scores" in text) == (out == "fused")
        assert not (tmp_path / out / "ensemble").exists()
        rows[out] = {}
        for name in ("efficientnet_b0", "efficientnet_b3"):
            (run,) = [p for p in (tmp_path / out / name).iterdir() if p.is_dir()]
            rows[out][name] = [json.loads(s) for s in (run / "logs" / "metrics.jsonl").read_text().splitlines()]
            assert sorted(p.name for p in run.iterdir()) == ["checkpoints", "config_snapshot.yaml", "logs", "plots"]
    for name in ("efficientnet_b0", "efficientnet_b3"):
        plain, fused = rows["plain"][name], rows["fused"][name]
        assert len(plain) == len(fused) == 1
        assert {k: v for k, v in plain[0].items() if k != "timestamp"} == {k: v for k, v in fused[0].items() if k != "timestamp"}


def test_ensemble_refuses_members_that_scored_other_samples(tmp_path):
    """The checks that come before any launch: what stops the ensemble with a warning (ensemble_obstacle) and what is an error."""
    from dataclasses import replace
    from pathlib import Path

    from deepfakedetection_amd.orchestration import orchestrator as O

    settings = O.InferenceSettings(name="m", root=tmp_path, split="test", val_split="val", num_classes=2, image_size=32, batch_size=4,
                                   num_workers=0, amp=False, device=torch.device("cpu"), fp8_weights=False, transform=None,
                                   device_metrics=True, calibration=None, robustness=(), cam_limit=None)
    y = torch.tensor([0, 1, 1, 0])
    one = O.MemberScores(settings=settings, classes=["fake", "real"], paths=["a", "b", "c", "d"], val=None, val_paths=[],
                         clean=(torch.zeros(4, 2), y), preds=y, levels={}, temperature=None, record={})
    ens = O.EnsembleSettings(("a", "b"), "logit", "equal", 0.0, tmp_path / "ensemble")
    assert O.ensemble_obstacle(ens, {"a": one, "b": one}) is None
    assert "b kept no scores" in O.ensemble_obstacle(ens, {"a": one, "b": None}) and "kept no scores" in O.ensemble_obstacle(ens, {"a": one})
    for key, value in (("split", "other"), ("val_split", "dev"), ("num_classes", 3)):
        assert f"differ in {key}" in O.ensemble_obstacle(ens, {"a": one, "b": replace(one, settings=replace(settings, **{key: value}))})
    paths = O.ensure_run_dirs(Path(tmp_path / "ensemble"), "now")
    for other in (replace(one, paths=["a", "b", "d", "c"]), replace(one, clean=(torch.zeros(4, 2), 1 - y)),
                  replace(one, val=(torch.zeros(2, 2), y[:2]), val_paths=["e", "f"])):
        with pytest.raises(ValueError, match="scored other samples or targets"):
            O.run_ensemble_job(ens, ["a", "b"], [one, other], paths)
    assert not (paths.run_dir / "ensemble.json").exists() and not (paths.logs / "metrics.jsonl").exists()
