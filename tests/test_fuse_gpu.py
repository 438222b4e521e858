"""The ensemble kernels (csrc/dfd_fuse.hip through kernels.fuse_scores / fuse_nll / fuse_agree and deepfakedetection_amd.metrics)
against the reference of tests/_fuse_ref.py.  The integer outputs are compared with ==.  The f64 sums are compared at a bound the
test computes from the data (see _close_sums).  The stored probabilities may differ from the rounded float64 reference by 1 ulp on
1 element in 1000 (tests/test_fuse_cpu.py holds the reference itself to that cap on the same inputs).  Every output is an interior
slice of a buffer filled with a canary (-1 for the integers, NaN for the floats), and the canaries around it must survive.  The
tier every case names is asserted through dfd_fuse_plan."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import torch

from deepfakedetection_amd import kernels as K
from deepfakedetection_amd import metrics as M
from tests import _fuse_ref as R

pytestmark = pytest.mark.gpu

GUARD = 32
EDGE = K.FUSE_THREAD_MAX_KJ


def _guarded(shape, dtype, canary):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device="cuda")
    return big, big[GUARD:GUARD + n].view(*shape)


def _intact(big: torch.Tensor) -> bool:
    host = big.cpu()
    rest = torch.cat([host[:GUARD], host[-GUARD:]])
    return bool(torch.isnan(rest).all()) if big.dtype.is_floating_point else bool((rest == -1).all())


def _sizes(members: int, J: int) -> list[int]:
    return R.sizes(K.fuse_plan(1, J, members).rows, K.FUSE_STAGE2_WIDTH)


def _assert_tier(n: int, J: int, members: int) -> None:
    plan = K.fuse_plan(n, J, members)
    thread = members * J <= EDGE
    assert plan.layout == (K.FUSE_LAYOUT_THREAD if thread else K.FUSE_LAYOUT_WAVE) and plan.rows == (256 if thread else 32)
    assert plan.blocks == min(-(-n // plan.rows), K.FUSE_MAX_BLOCKS) and plan.trips == -(-plan.blocks // K.FUSE_STAGE2_WIDTH)


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _device_scores(zs, coef, mode, beta=None):
    n, J = zs[0].shape
    p_big, probs = _guarded((n, J), torch.float32, float("nan"))
    f_big, fused = _guarded((n, J), torch.float32, float("nan"))
    i_big, preds = _guarded((n,), torch.int64, -1)
    s_big, stats = _guarded((1,), torch.int64, -1)
    K.fuse_scores(_dev(zs), coef, mode, beta, out=(probs, preds, fused, stats))
    torch.cuda.synchronize()
    assert _intact(p_big) and _intact(f_big) and _intact(i_big) and _intact(s_big), "a write outside probs / logits / preds / stats"
    return probs.cpu().numpy(), preds.cpu().numpy(), fused.cpu().numpy(), int(stats.cpu()[0])


def _device_nll(zs, targets, cands):
    o_big, out = _guarded((len(cands), K.fuse_terms(len(zs))), torch.float64, float("nan"))
    s_big, stats = _guarded((2,), torch.int64, -1)
    K.fuse_nll(_dev(zs), torch.from_numpy(targets).cuda(), cands, out=(out, stats))
    torch.cuda.synchronize()
    assert _intact(o_big) and _intact(s_big), "a write outside out / stats"
    return out.cpu().numpy(), stats.cpu().tolist()


def _device_agree(preds, targets, J):
    members = len(preds)
    p_big, pair = _guarded((members, members, 4), torch.int64, -1)
    h_big, hist = _guarded((members + 1,), torch.int64, -1)
    s_big, stats = _guarded((2,), torch.int64, -1)
    K.fuse_agree(_dev(preds), torch.from_numpy(targets).cuda(), J, out=(pair, hist, stats))
    torch.cuda.synchronize()
    assert _intact(p_big) and _intact(h_big) and _intact(s_big), "a write outside pair / hist / stats"
    return pair.cpu().tolist(), hist.cpu().tolist(), stats.cpu().tolist()


def _close_sums(got, want, mag, addends: int, per_row: float, what: str) -> None:
    """|device - fsum reference| <= _calib_ref.sum_bound (tests/test_calib_gpu.py's _close_sums), with the per-row factor
    _fuse_ref.fuse_per_row derives for the pooled logit.  Nothing is added on top."""
    bound = R.sum_bound(float(mag), addends, per_row)
    print(f"[fuse] {what}: |diff| {abs(float(got) - float(want)):.3e} (bound {bound:.3e}, magnitude {float(mag):.3e})")
    assert abs(float(got) - float(want)) <= bound, what


def _check_nll(zs, targets, cands, what: str, stats=(0, 0)) -> None:
    members, (n, J) = len(zs), zs[0].shape
    want = R.nll(zs, targets, cands)
    got, nstats = _device_nll(zs, targets, cands)
    assert nstats == want.stats == list(stats), what
    names = ["nll"] + [f"g{k}" for k in range(members)] + [f"H{k}{l}" for k in range(members) for l in range(k, members)]
    for c in range(len(cands)):
        factor = R.fuse_per_row(J, members, want.amax[c])
        for o, name in enumerate(names):
            _close_sums(got[c, o], want.out[c, o], want.mag[c, o], n, factor, f"{name} {what} cand={c}")


# ------------------------------------------------------------------ fuse_agree
def _preds_case(seed: int, n: int, J: int, members: int):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, J, size=n).astype(np.int64)
    preds = [np.where(rng.random(n) < 0.4 + 0.07 * k, y, rng.integers(0, J, size=n)).astype(np.int64) for k in range(members)]
    return preds, y


@pytest.mark.parametrize("members,J", [(1, 2), (2, 2), (3, 3), (8, 2), (8, 17), (5, 1000)])
def test_agree_equals_the_reference_at_every_size(members, J):
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 513] + ([K.FUSE_MAX_BLOCKS * 256 + 1] if members == 3 else [])      # the last: a second stride
    preds_all, y_all = _preds_case(members * J, sizes[-1], J, members)
    for n in sizes:
        preds, y = [p[:n] for p in preds_all], y_all[:n]
        got = _device_agree(preds, y, J)
        assert got == R.agree(preds, y, J), (n, members, J)
        assert got[2] == [n, 0] and sum(got[1]) == n
    n = 300
    preds, y = [p[:n].copy() for p in preds_all], y_all[:n].copy()
    for case, ps in (("all right", [y.copy() for _ in preds]), ("all wrong", [(y + 1) % J for _ in preds]),
                     ("identical", [preds[0]] * members)):
        pair, hist, stats = _device_agree(ps, y, J)
        assert (pair, hist, stats) == R.agree(ps, y, J), case
        if case == "all right":
            assert hist == [0] * members + [n] and all(cell == [n, 0, 0, 0] for row in pair for cell in row)
        if case == "identical":
            assert all(cell[1] == cell[2] == 0 for row in pair for cell in row) and sum(hist[1:members]) == 0
    y[:6] = [-1, J, 2 ** 40 + 1, -(2 ** 40), J + 7, 2 ** 32]                    # out of range, two of them in range once truncated
    got = _device_agree(preds, y, J)
    assert got == R.agree(preds, y, J) and got[2] == [n - 6, 6]
    perm = np.random.default_rng(1).permutation(n)                              # the integers do not depend on the order
    assert _device_agree([p[perm] for p in preds], y[perm], J) == got
    with pytest.raises(ValueError, match="outside"):
        M.diversity(_dev(preds), torch.from_numpy(y).cuda(), J)
    res = M.diversity(_dev([p[6:] for p in preds]), torch.from_numpy(y[6:]).cuda(), J)
    pair, hist, stats = R.agree([p[6:] for p in preds], y[6:], J)
    assert res == M.diversity_from_counts(pair, hist, stats[0]) and res.valid == n - 6


# ------------------------------------------------------------------ fuse_nll
@pytest.mark.parametrize("members,J", R.SHAPES)
def test_nll_at_every_size(members, J):
    sizes = _sizes(members, J)
    zs_all, y_all = R.members_case(members * 31 + J, sizes[-1], J, members)
    cands = [[1.0 / members] * members, R.capped_coef(zs_all, J), (-np.asarray(R.capped_coef(zs_all, J + 1))).tolist()]
    for n in sizes:
        _assert_tier(n, J, members)
        _check_nll([z[-n:] for z in zs_all], y_all[-n:], cands, f"n={n} J={J} K={members}")


@pytest.mark.parametrize("members,J", [(3, 2), (2, 17)])
def test_nll_with_eight_candidates_and_with_one(members, J):
    n = 2 * K.fuse_plan(1, J, members).rows + 1
    zs, y = R.members_case(50 + J, n, J, members)
    rng = np.random.default_rng(J)
    eight = [(np.asarray(R.capped_coef(zs, c)) * rng.uniform(0.2, 1.0)).tolist() for c in range(K.FUSE_MAX_CANDS)]
    _check_nll(zs, y, eight, f"eight candidates J={J} K={members}")
    _check_nll(zs, y, eight[3:4], f"one candidate J={J} K={members}")
    both, alone = _device_nll(zs, y, eight)[0], _device_nll(zs, y, eight[3:4])[0]
    assert both[3].tobytes() == alone[0].tobytes()                              # a candidate's sums do not depend on its neighbours
    with pytest.raises(ValueError):
        K.fuse_nll(_dev(zs), torch.from_numpy(y).cuda(), eight + eight[:1])


@pytest.mark.parametrize("members,J", [(3, 2), (8, 2), (2, 17), (2, 1000)])
def test_two_calls_return_the_same_bits(members, J):
    n = K.FUSE_STAGE2_WIDTH * K.fuse_plan(1, J, members).rows + 1
    zs, y = R.members_case(90 + J, n, J, members)
    cands = [[1.0 / members] * members, R.capped_coef(zs, 2)]
    a, b = _device_nll(zs, y, cands)[0], _device_nll(zs, y, cands)[0]
    assert a.tobytes() == b.tobytes()
    coef = cands[1]
    first, second = _device_scores(zs, coef, K.FUSE_LOGIT), _device_scores(zs, coef, K.FUSE_LOGIT)
    assert all(x.tobytes() == y_.tobytes() for x, y_ in zip(first[:3], second[:3]))


@pytest.mark.parametrize("members,J", [(2, 2), (3, 3), (8, 2), (2, 17), (8, 17), (2, 1000)])
def test_rows_that_are_not_finite_in_one_member_and_targets_out_of_range(members, J):
    n = 300
    zs, y = R.members_case(7 * J + members, n, J, members)
    for i, bad in zip((10, 11, 12), (np.nan, np.inf, -np.inf)):
        zs[i % members][i, (i * 7) % J] = bad                                   # one member only
    y[20], y[21], y[22] = -1, J, 2 ** 40 + 1                                    # the last one is in range once truncated to 32 bits
    zs[members - 1][23, 0], y[23] = np.nan, -1                                  # non-finite and out of range: counted as non-finite
    cands = [[1.0 / members] * members, R.capped_coef(zs, 9)]
    _check_nll(zs, y, cands, f"bad rows J={J} K={members}", stats=(4, 3))
    for mode, coef in ((K.FUSE_LOGIT, cands[1]), (K.FUSE_PROB, R.ramp_weights(members))):
        probs, preds, fused, nonfinite = _device_scores(zs, coef, mode, R.ramp_betas(members))
        bad_rows = [10, 11, 12, 23]
        assert nonfinite == 4 and np.isnan(probs[bad_rows]).all() and np.isnan(fused[bad_rows]).all() and (preds[bad_rows] == 0).all()
        good = np.setdiff1d(np.arange(n), bad_rows)
        assert np.isfinite(probs[good]).all() and np.isfinite(fused[good]).all()
    dev = _dev(zs)
    with pytest.raises(ValueError, match="outside"):
        M.fit_fusion(dev, torch.from_numpy(y).cuda())
    with pytest.raises(ValueError, match="no row"):
        M.fit_fusion([torch.full((5, J), float("nan"), device="cuda")] * members, torch.zeros(5, dtype=torch.int64, device="cuda"))


def test_empty_inputs():
    for members, J in ((3, 2), (2, 17)):
        empty = [np.zeros((0, J), dtype=np.float32)] * members
        out, stats = _device_nll(empty, np.zeros(0, dtype=np.int64), [[0.5] * members])
        assert not out.any() and stats == [0, 0]
        probs, preds, fused, nonfinite = _device_scores(empty, [0.5] * members, K.FUSE_LOGIT)
        assert probs.shape == (0, J) and preds.shape == (0,) and nonfinite == 0


# ------------------------------------------------------------------ fuse_scores
def _within_one_ulp(got: np.ndarray, want: np.ndarray, what: str) -> None:
    """Stored f32 values (positive normals) against the rounded float64 reference: at most 1 ulp apart, on at most 1 element in
    1000.  The kernel's f64 error is about 1e-14 relative, so only a value that close to a rounding tie can land on the other
    side: about 2e-6 of the elements.  tests/test_fuse_cpu.py holds the reference's own two summation orders to this cap."""
    assert np.all(want >= np.finfo(np.float32).tiny) and np.isfinite(got).all(), what
    differ, worst = R.ulp_mismatches(got, want)
    print(f"[fuse] {what}: {differ} of {got.size} elements differ, by at most {worst} ulp")
    assert worst <= 1 and differ * 1000 <= got.size, what


@pytest.mark.parametrize("members,J", R.SHAPES)
def test_scores_at_every_size(members, J):
    sizes = _sizes(members, J)
    zs_all, coef = R.score_case(members, J, sizes[-1])
    weights, betas = R.ramp_weights(members), R.ramp_betas(members)
    want = {K.FUSE_LOGIT: R.scores(zs_all, coef, R.LOGIT), K.FUSE_PROB: R.scores(zs_all, weights, R.PROB, betas)}
    for n in sizes:
        _assert_tier(n, J, members)
        zs = [z[-n:] for z in zs_all]
        for mode, a in ((K.FUSE_LOGIT, coef), (K.FUSE_PROB, weights)):
            probs, preds, fused, nonfinite = _device_scores(zs, a, mode, betas)
            _within_one_ulp(probs, want[mode][0][-n:], f"probs n={n} J={J} K={members} mode={mode}")
            assert nonfinite == 0 and np.array_equal(preds, probs.argmax(axis=1)), (n, mode)       # numpy: the first index that attains it
            # the fused logits: the pooled sum itself (the same products in the same order), or the log of a probability whose
            # relative error (6 A + J + K + 4) u, A = max |beta z| (_calib_ref.nll_per_row), the log turns into an absolute one
            ref_fused = want[mode][2][-n:].astype(np.float64)
            slack = 0.0 if mode == K.FUSE_LOGIT else 2.0 * (6.0 * max(betas) * max(float(np.abs(z).max()) for z in zs) + J + members + 4) * R.U
            assert np.all(np.abs(fused.astype(np.float64) - ref_fused) <= np.spacing(np.abs(ref_fused).astype(np.float32)) + slack), (n, mode)
    zs = [z[-65:] for z in zs_all]
    only_preds = K.fuse_scores(_dev(zs), coef, K.FUSE_LOGIT, want_probs=False, want_logits=False)
    assert only_preds[0] is None and only_preds[2] is None
    assert np.array_equal(only_preds[1].cpu().numpy(), _device_scores(zs, coef, K.FUSE_LOGIT)[1])


@pytest.mark.parametrize("J", [2, 3, EDGE, EDGE + 1, 65, 1000])
def test_one_member_with_coefficient_one_predicts_the_arg_max_of_its_logits(J):
    """Logits on a grid of 1 / 8 within +-9: two that differ are at least a factor e^(1/8) apart as probabilities, none of which
    underflows, so the arg max of the stored probabilities is that of the logits; equal logits tie, and the first index wins."""
    n = 513
    rng = np.random.default_rng(J)
    z = (rng.integers(-72, 73, size=(n, J)) / 8.0).astype(np.float32)
    z[0], z[1, :] = 2.5, -9.0                                                   # every class ties
    z[2] = np.minimum(z[2], 8.0)
    z[2, J - 1] = z[2, J // 2] = 9.0                                            # two tie: the lower index wins
    probs, preds, fused, _ = _device_scores([z], [1.0], K.FUSE_LOGIT)
    assert np.array_equal(preds, z.argmax(axis=1)) and np.array_equal(fused, z) and preds[0] == preds[1] == 0 and preds[2] == J // 2
    _within_one_ulp(probs, R.scores([z], [1.0])[0], f"one member J={J}")


@pytest.mark.parametrize("members,J", [(2, 2), (4, 4), (8, 2), (4, 17), (8, 1000)])
def test_a_linear_pool_of_identical_members_is_the_member(members, J):
    """At weights 1 / K (exact for K = 2, 4, 8) and one temperature the pooled sum is the member's softmax itself."""
    z = R.members_case(J, 300, J, 1)[0][0]
    beta = 0.75
    single = _device_scores([z], [1.0], K.FUSE_PROB, [beta])
    pooled = _device_scores([z] * members, [1.0 / members] * members, K.FUSE_PROB, [beta] * members)
    assert single[0].tobytes() == pooled[0].tobytes() and np.array_equal(single[1], pooled[1])
    _within_one_ulp(single[0], R.scores([z], [1.0], R.PROB, [beta])[0], f"softmax of one member J={J}")
    with pytest.raises(ValueError, match="sum to 1"):
        K.fuse_scores(_dev([z, z]), [0.5, 0.6], K.FUSE_PROB, [1.0, 1.0])
    with pytest.raises(ValueError, match="sum to 1"):
        K.fuse_scores(_dev([z, z]), [0.5, 0.5], K.FUSE_PROB, [1.0, 0.0])


@pytest.mark.parametrize("members,J", [(3, 2), (8, 2), (2, 17), (3, 1000)])
def test_saturated_logits_stay_finite(members, J):
    n = 257
    rng = np.random.default_rng(members + J)
    zs = [(rng.uniform(-1e4, 1e4, size=(n, J))).astype(np.float32) for _ in range(members)]
    coef = rng.uniform(0.2, 1.0, size=members).tolist()
    pooled = R.pool(R.stack(zs), coef)
    top = np.sort(pooled, axis=1)
    clear = top[:, -1] - top[:, -2] > 1.0                                       # the largest pooled logit stands alone
    assert clear.sum() > 0.9 * n
    for mode, a, want in ((K.FUSE_LOGIT, coef, pooled.argmax(axis=1)), (K.FUSE_PROB, R.ramp_weights(members), None)):
        probs, preds, fused, nonfinite = _device_scores(zs, a, mode, [1.0] * members)
        assert nonfinite == 0 and np.isfinite(probs).all() and np.all(np.abs(probs.astype(np.float64).sum(axis=1) - 1.0) <= 1e-6)
        assert np.array_equal(preds, probs.argmax(axis=1))
        if want is not None:
            assert np.array_equal(preds[clear], want[clear]) and np.isfinite(fused).all()


def test_fuse_front_end():
    zs, _ = R.members_case(3, 200, 3, 3)
    dev = _dev(zs)
    probs, preds, fused = M.fuse(dev)
    want = R.scores(zs, [1.0 / 3] * 3)
    _within_one_ulp(probs.cpu().numpy(), want[0], "fuse, equal weights")
    assert np.array_equal(preds.cpu().numpy(), probs.cpu().numpy().argmax(axis=1))
    temps = [2.0, None, 0.5]
    folded = R.scores(zs, [0.2 / 2.0, 0.3, 0.5 / 0.5])
    _within_one_ulp(M.fuse(dev, [0.2, 0.3, 0.5], temperatures=temps)[0].cpu().numpy(), folded[0], "fuse, temperatures folded")
    linear = R.scores(zs, [0.2, 0.3, 0.5], R.PROB, [0.5, 1.0, 2.0])
    _within_one_ulp(M.fuse(dev, [0.2, 0.3, 0.5], mode="prob", temperatures=temps)[0].cpu().numpy(), linear[0], "fuse, linear pool")
    with pytest.raises(ValueError):
        M.fuse(dev, mode="vote")
    with pytest.raises(ValueError):
        M.fuse(dev, [0.5, 0.5])


# ------------------------------------------------------------------ the fit
@pytest.mark.parametrize("members,J,n", [(1, 2, 65), (2, 3, 257), (3, 2, 2049), (8, 17, 257), (3, 65, 65), (8, 2, 2049)])
def test_fit_fusion_reaches_the_minimum_of_the_reference(members, J, n):
    zs, y = R.members_case(members * 1000 + J + n, n, J, members, scale=1.0 if members * J > 100 else 3.0)
    dev, y_dev = _dev(zs), torch.from_numpy(y).cuda()
    fit = M.fit_fusion(dev, y_dev)
    ref = R.fit(zs, y)
    print(f"[fuse] fit K={members} J={J} n={n}: device {fit.coef} in {fit.iterations}, reference {ref.coef} in {ref.iterations}")
    assert fit.converged and not fit.at_bound and fit.iterations <= 30 and fit.valid == n and fit.nonfinite == 0
    at = R.nll(zs, y, [fit.coef])
    factor = R.fuse_per_row(J, members, at.amax[0])
    for k in range(members):                                                    # the reference's gradient at the device's coefficients
        g, bound = at.out[0, 1 + k], R.sum_bound(at.mag[0, 1 + k], n, factor)
        print(f"[fuse] g{k} / n = {g / n:.3e} (1e-10 + {bound / n:.3e})")
        assert abs(g) / n <= 1e-10 + bound / n
    assert ref.converged
    low = (ref.nll_after_sum + R.sum_bound(ref.nll_after_mag, n, R.fuse_per_row(J, members, ref.amax))) / n
    print(f"[fuse] nll_after {fit.nll_after!r}, the reference minimum plus its bound {low!r}")
    assert fit.nll_after <= low and fit.nll_after <= fit.nll_before
    ridge = M.fit_fusion(dev, y_dev, l2=1e-2)
    assert ridge.converged and not ridge.at_bound


def test_fit_fusion_on_separable_data():
    zs, y = R.separable_case(257)
    dev, y_dev = _dev(zs), torch.from_numpy(y).cuda()
    fit = M.fit_fusion(dev, y_dev)
    assert fit.at_bound and not fit.converged and max(abs(c) for c in fit.coef) > 32.0 and fit.nll_after < fit.nll_before
    ridge = M.fit_fusion(dev, y_dev, l2=1e-2)
    assert ridge.converged and not ridge.at_bound and max(abs(c) for c in ridge.coef) <= 32.0


# ------------------------------------------------------------------ end to end
def _config(tmp_path: Path, out: str, models: dict, ensemble) -> Path:
    import yaml

    infer = {"split": "test", "batch_size": 8, "num_workers": 0, "img_size": 64, "gpu_resize": True, "robustness": {"blur_sigma": [2]},
             "device_metrics": True}
    cfg = {"seed": 1, "device": "cuda",
           "data": {"root": str(tmp_path / "data"), "val_split": "val", "test_split": "test", "num_classes": 2, "img_size": 64},
           "models": {key: {"name": arch, "output_dir": str(tmp_path / out / key), "inference": {**infer, **extra}}
                      for key, (arch, extra) in models.items()}}
    if ensemble is not None:
        cfg["ensemble"] = {**ensemble, "output_dir": str(tmp_path / out / "ensemble")}
    path = tmp_path / f"{out}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return path


def _run(base: Path) -> Path:
    (run,) = [p for p in base.iterdir() if p.is_dir()]
    return run


def test_inference_with_an_ensemble(tmp_path, monkeypatch):
    from deepfakedetection_amd.orchestration import orchestrator as O
    from tests.test_plumbing_cpu import _make_dataset

    _make_dataset(tmp_path / "data", classes=("fake", "real"), per_class=4, size=64)
    judged = []
    real = O._split_metrics_device
    monkeypatch.setattr(O, "_split_metrics_device", lambda name, *rest: (judged.append((name, real(name, *rest))), judged[-1][1])[1])

    two = {"efficientnet_b0": ("efficientnet_b0", {}), "efficientnet_b3": ("efficientnet_b3", {})}
    O.orchestrate(_config(tmp_path, "fit", two, {"mode": "logit", "weights": "fit"}), mode="inference")
    run = _run(tmp_path / "fit" / "ensemble")
    rows = [json.loads(s) for s in (run / "logs" / "metrics.jsonl").read_text().splitlines()]
    member_rows = [json.loads(s) for s in (_run(tmp_path / "fit" / "efficientnet_b0") / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert len(rows) == len(member_rows) == 2 and "perturbation" not in rows[0] and rows[1]["perturbation"] == {"blur_sigma": 2.0}
    figures = {"ece", "mce", "brier", "nll"}
    assert set(rows[0]) == set(member_rows[0]) | figures and set(rows[1]) == set(member_rows[1]) | figures
    assert all(row["model"] == "ensemble" and row["split"] == "test" for row in rows) and rows[1]["threshold"] == rows[0]["threshold"]
    assert (run / "logs" / "ensemble.log").stat().st_size > 0 and (run / "plots" / "confusion_matrix.png").stat().st_size > 0
    doc = json.loads((run / "ensemble.json").read_text())
    assert doc["members"] == list(two) and doc["mode"] == "logit" and len(doc["coefficients"]) == 2
    assert set(doc["clean"]) == set(two) | {"ensemble"} and doc["clean"]["ensemble"]["accuracy"] == rows[0]["accuracy"]
    pair = doc["diversity"]["pair"]
    assert all(sum(pair[a][b]) == 8 for a in range(2) for b in range(2)) and sum(doc["diversity"]["hist"]) == 8 == doc["diversity"]["valid"]
    if isinstance(doc["fit"], dict):                                            # an untrained pair may separate eight validation images
        assert set(doc["fit"]) == {"coef", "nll_before", "nll_after", "iterations", "at_bound", "converged", "valid", "nonfinite"}
        assert doc["fit"]["valid"] == 8 and (doc["fit"]["at_bound"] or doc["coefficients"] == doc["fit"]["coef"])
        assert not doc["fit"]["at_bound"] or doc["coefficients"] == [0.5, 0.5]

    # two members of one architecture with one weights file: the ensemble is the member
    weights = tmp_path / "b0.pth"
    torch.manual_seed(3)
    torch.save(O.load_model("efficientnet_b0", 2, None, torch.device("cuda"), 64).state_dict(), weights)
    twins = {key: ("efficientnet_b0", {"weights": str(weights)}) for key in ("first", "second")}
    judged.clear()
    O.orchestrate(_config(tmp_path, "twins", twins, {"weights": "equal"}), mode="inference")
    doc = json.loads((_run(tmp_path / "twins" / "ensemble") / "ensemble.json").read_text())
    assert doc["members"] == ["first", "second"] and doc["coefficients"] == [0.5, 0.5] and doc["fit"] is None
    assert doc["diversity"]["disagreement"] == [[0.0, 0.0], [0.0, 0.0]]
    names = [name for name, _ in judged]
    assert names == ["efficientnet_b0"] * 4 + ["ensemble"] * 2                   # clean and blurred per job
    member_clean, ensemble_clean = judged[0][1], judged[4][1]
    assert torch.equal(ensemble_clean[2], member_clean[2]) and torch.equal(ensemble_clean[3], member_clean[3])     # predictions, targets
    assert torch.equal(judged[5][1][2], judged[1][1][2])                        # under the blur too
    assert doc["clean"]["ensemble"]["accuracy"] == doc["clean"]["first"]["accuracy"] == doc["clean"]["second"]["accuracy"]

    # without the key: no ensemble directory
    O.orchestrate(_config(tmp_path, "plain", two, None), mode="inference")
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == sorted(two)
