"""The calibration kernels (csrc/dfd_calib.hip through kernels.calib_bins / calib_nll / softmax_argmax_t and
deepfakedetection_amd.metrics) against the reference of tests/_calib_ref.py.  The integer outputs are compared with ==.  The f64 sums
are compared at a bound the test computes from the data (see _close_sums).  Every output is an interior slice of a buffer filled with
a canary (-1 for the integers, NaN for the floats), and the canaries around it must survive.  The tier every case names is asserted
through dfd_calib_plan."""

from __future__ import annotations

import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from deepfakedetection_amd import kernels as K
from deepfakedetection_amd import metrics as M
from tests import _calib_ref as R

pytestmark = pytest.mark.gpu

GUARD = 32
EDGE_J = K.CALIB_THREAD_MAX_J                       # the widest row of the one-thread-per-row layout
WIDTHS = [2, 3, EDGE_J, EDGE_J + 1, 65, 1000, 1024]
BETAS = [0.25, 1.0, 3.0]


def _guarded(shape, dtype, canary):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), canary, dtype=dtype, device="cuda")
    return big, big[GUARD:GUARD + n].view(*shape)


def _intact(big: torch.Tensor) -> bool:
    host = big.cpu()
    rest = torch.cat([host[:GUARD], host[-GUARD:]])
    return bool(torch.isnan(rest).all()) if big.dtype.is_floating_point else bool((rest == -1).all())


def _sizes(J: int) -> list[int]:
    """1, the wave width and its neighbours, the rows of one workgroup and its neighbours, two workgroups + 1, and the smallest n
    whose stage-2 loop takes a second trip."""
    rows = K.calib_plan(1, J).rows
    return sorted({1, 63, 64, 65, rows - 1, rows, rows + 1, 2 * rows + 1, K.CALIB_STAGE2_WIDTH * rows + 1})


def _assert_tier(n: int, J: int) -> None:
    plan = K.calib_plan(n, J)
    thread = J <= EDGE_J
    assert plan.layout == (K.CALIB_LAYOUT_THREAD if thread else K.CALIB_LAYOUT_WAVE) and plan.rows == (256 if thread else 32)
    assert plan.blocks == min(-(-n // plan.rows), K.CALIB_MAX_BLOCKS) and plan.trips == -(-plan.blocks // K.CALIB_STAGE2_WIDTH)


def _device_bins(probs: np.ndarray, targets: np.ndarray, M_bins: int):
    """calib_bins into guarded outputs -> (table as Python ints, stats, the Brier sum)."""
    t_big, table = _guarded((M_bins, 3), torch.int64, -1)
    s_big, stats = _guarded((4,), torch.int64, -1)
    b_big, brier = _guarded((1,), torch.float64, float("nan"))
    K.calib_bins(torch.from_numpy(probs).cuda(), torch.from_numpy(targets).cuda(), M_bins, out=(table, stats, brier))
    torch.cuda.synchronize()
    assert _intact(t_big) and _intact(s_big) and _intact(b_big), "a write outside bins / stats / brier"
    return table.cpu().tolist(), stats.cpu().tolist(), float(brier.cpu()[0])


def _device_nll(logits: np.ndarray, targets: np.ndarray, betas):
    o_big, out = _guarded((len(betas), 3), torch.float64, float("nan"))
    s_big, stats = _guarded((2,), torch.int64, -1)
    K.calib_nll(torch.from_numpy(logits).cuda(), torch.from_numpy(targets).cuda(), betas, out=(out, stats))
    torch.cuda.synchronize()
    assert _intact(o_big) and _intact(s_big), "a write outside out / stats"
    return out.cpu().numpy(), stats.cpu().tolist()


def _close_sums(got, want, mag, addends: int, per_row: float, what: str) -> None:
    """|device - fsum reference| <= _calib_ref.sum_bound, which is built from three things only.  (1) The device adds `addends`
    terms in a fixed order, and any order of n floating-point additions is within (n - 1) u / (1 - (n - 1) u) of the exact sum,
    relative to the summed magnitude `mag` of the terms, u = 2^-53.  (2) Each side evaluates a term to within `per_row` u of its
    magnitude: 3 for a Brier term (a difference and a square), _calib_ref.nll_per_row for nll / g / h, which grows with max |beta z|
    because m + log s - a_y cancels and because exp turns the absolute error of beta z - m into a relative one.  (3) fsum rounds
    once.  Nothing is added on top: for n = 16 385 rows the bound is about 2e-12 of the magnitude, while one dropped or doubled row
    moves the sum by about 1 / n = 6e-5 of it."""
    bound = R.sum_bound(float(mag), addends, per_row)
    print(f"[calib] {what}: |diff| {abs(float(got) - float(want)):.3e} (bound {bound:.3e}, magnitude {float(mag):.3e})")
    assert abs(float(got) - float(want)) <= bound, what


def _rows_case(seed: int, n: int, J: int):
    """Probabilities on a grid of 1 / 256 (ties and bin edges are common), the logits they came from, and targets that follow the
    arg max two times in three."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((n, J)) * 3).astype(np.float32)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    probs = (np.round(e / e.sum(axis=1, keepdims=True) * 256) / 256).astype(np.float32)
    targets = np.where(rng.random(n) < 0.66, probs.argmax(axis=1), rng.integers(0, J, size=n)).astype(np.int64)
    return probs, logits, targets


@pytest.mark.parametrize("J", WIDTHS)
def test_bins_and_nll_at_every_size(J):
    sizes = _sizes(J)
    probs_all, logits_all, targets_all = _rows_case(J, sizes[-1], J)
    for n in sizes:
        _assert_tier(n, J)
        probs, logits, targets = probs_all[-n:], logits_all[-n:], targets_all[-n:]
        ref = R.bins(probs, targets, 15)
        table, stats, brier = _device_bins(probs, targets, 15)
        assert table == ref.table and stats == ref.stats, (n, J)
        _close_sums(brier, ref.brier_sum, ref.brier_mag, ref.brier_terms, 3.0, f"brier n={n} J={J}")
        want = R.nll(logits, targets, BETAS)
        got, nstats = _device_nll(logits, targets, BETAS)
        assert nstats == want.stats == [0, 0]
        for k, beta in enumerate(BETAS):
            for c, name in enumerate(("nll", "g", "h")):
                _close_sums(got[k, c], want.out[k, c], want.mag[k, c], n, R.nll_per_row(J, want.amax[k]), f"{name} n={n} J={J} beta={beta}")


@pytest.mark.parametrize("J", [2, EDGE_J + 1])
def test_two_calls_return_the_same_bits(J):
    n = K.CALIB_STAGE2_WIDTH * K.calib_plan(1, J).rows + 1
    probs, logits, targets = _rows_case(90 + J, n, J)
    first, second = _device_bins(probs, targets, 15), _device_bins(probs, targets, 15)
    assert first[:2] == second[:2] and np.float64(first[2]).tobytes() == np.float64(second[2]).tobytes()
    a, b = _device_nll(logits, targets, BETAS)[0], _device_nll(logits, targets, BETAS)[0]
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("J", [2, 3, EDGE_J + 1])
@pytest.mark.parametrize("M_bins", [4, 8, 16])
def test_dyadic_confidences_on_the_edges(J, M_bins):
    """Rows (k / 256, 1 - k / 256, 0, ...): every confidence is a multiple of 1 / 256 and so sits exactly on an edge of 4, 8 and 16
    bins again and again; such a confidence belongs to the bin below (right-closed)."""
    k = np.arange(257)
    probs = np.zeros((257, J), dtype=np.float32)
    probs[:, 0], probs[:, 1] = k / 256.0, 1.0 - k / 256.0
    targets = (k % 2).astype(np.int64)
    _assert_tier(257, J)
    ref = R.bins(probs, targets, M_bins)
    table, stats, _ = _device_bins(probs, targets, M_bins)
    assert table == ref.table and stats == ref.stats
    conf = np.maximum(k, 256 - k)
    assert [row[0] for row in table] == [int(((conf * M_bins > 256 * b) & (conf * M_bins <= 256 * (b + 1))).sum()) for b in range(M_bins)]
    assert sum(row[2] for row in table) == int(conf.sum()) << 24                # q = conf / 256 * 2^32, exactly


@pytest.mark.parametrize("J", [2, EDGE_J + 1])
def test_fifteen_bins_at_the_rounded_edges_and_their_neighbours(J):
    """float32(k / 15) and the f32 values next to it on both sides: the comparison runs in f64 against the f64 quotient k / 15, so on
    which side float32(k / 15) falls is decided by how it was rounded."""
    mid = np.array([np.float32(k / 15) for k in range(1, 16)], dtype=np.float32)
    conf = np.concatenate([np.nextafter(mid, np.float32(0)), mid, np.nextafter(mid, np.float32(2))])
    probs = np.zeros((conf.size, J), dtype=np.float32)                          # the rest of the row is 0: the kernel takes any finite row
    probs[:, 1] = conf
    targets = np.ones(conf.size, dtype=np.int64)
    ref = R.bins(probs, targets, 15)
    table, stats, _ = _device_bins(probs, targets, 15)
    assert table == ref.table and stats == ref.stats
    # 1 / 15 = 0.(0001) in binary: rounding k / 15 to 24 bits always rounds up, so float32(k / 15) lies above the f64 edge and in
    # bin k, its lower neighbour below the edge and in bin k - 1; a comparison in f32 would put float32(k / 15) on the edge itself
    assert all(float(c) > k / 15 for k, c in zip(range(1, 15), mid.tolist()))
    assert R.bin_index(mid, 15).tolist() == list(range(1, 15)) + [14] and R.bin_index(conf[:15], 15).tolist() == list(range(15))


@pytest.mark.parametrize("J", [2, 3, EDGE_J, EDGE_J + 1, 65, 1000])
def test_ties_bad_rows_and_the_ends_of_the_scale(J):
    n = 300
    probs, logits, targets = _rows_case(7 * J, n, J)
    probs[0], targets[0] = 1.0 / 4, J - 1                                       # every class ties: the prediction is 0
    probs[1], targets[1] = 1.0 / 4, 0
    probs[2], probs[2, J - 1], probs[2, J // 2], targets[2] = 0.0, 0.5, 0.5, J // 2    # two tie: the lower index wins
    probs[3], targets[3] = 0.0, 0                                               # conf == 0: bin 0, predicted 0
    probs[4], probs[4, J - 1], targets[4] = 0.0, 1.0, J - 1                     # conf == 1: the last bin
    for i, bad in zip((10, 11, 12), (np.nan, np.inf, -np.inf)):
        probs[i, (i * 7) % J] = bad
        logits[i, (i * 7) % J] = bad
    targets[20], targets[21], targets[22] = -1, J, 2 ** 40 + 1                  # the last one is in range once truncated to 32 bits
    probs[23, 0], logits[23, 0], targets[23] = np.nan, np.nan, -1               # non-finite and out of range: counted as non-finite
    ref = R.bins(probs, targets, 15)
    assert ref.stats[1:3] == [4, 3]
    table, stats, brier = _device_bins(probs, targets, 15)
    assert table == ref.table and stats == ref.stats
    _close_sums(brier, ref.brier_sum, ref.brier_mag, ref.brier_terms, 3.0, f"brier with bad rows J={J}")
    perm = np.random.default_rng(J).permutation(n)                              # the integers do not depend on the order
    table_p, stats_p, _ = _device_bins(probs[perm], targets[perm], 15)
    assert table_p == table and stats_p == stats
    want = R.nll(logits, targets, BETAS)
    got, nstats = _device_nll(logits, targets, BETAS)
    assert nstats == want.stats == [4, 3]
    for k, beta in enumerate(BETAS):
        for c, name in enumerate(("nll", "g", "h")):
            _close_sums(got[k, c], want.out[k, c], want.mag[k, c], n, R.nll_per_row(J, want.amax[k]), f"{name} with bad rows J={J} beta={beta}")
    with pytest.raises(ValueError, match="outside"):
        M.calibration(torch.from_numpy(probs).cuda(), torch.from_numpy(targets).cuda())
    inside = (targets >= 0) & (targets < J)
    res = M.calibration(torch.from_numpy(probs[inside]).cuda(), torch.from_numpy(targets[inside]).cuda())
    ref_in = R.bins(probs[inside], targets[inside], 15)
    assert (res.ece, res.mce) == R.ece_mce(ref_in.table, ref_in.stats[0]) and res.nonfinite == 3 and res.valid == ref_in.stats[0]
    assert res.bins.tolist() == ref_in.table and res.count.tolist() == [row[0] for row in ref_in.table]


def test_empty_and_all_bad_inputs():
    table, stats, brier = _device_bins(np.zeros((0, 3), dtype=np.float32), np.zeros(0, dtype=np.int64), 15)
    assert table == [[0, 0, 0]] * 15 and stats == [0, 0, 0, 0] and brier == 0.0
    out, nstats = _device_nll(np.zeros((0, 3), dtype=np.float32), np.zeros(0, dtype=np.int64), BETAS)
    assert not out.any() and nstats == [0, 0]
    res = M.calibration(torch.full((5, 3), float("nan"), device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda"))
    assert (res.ece, res.mce, res.brier, res.valid, res.nonfinite) == (None, None, None, 0, 5)


@pytest.mark.parametrize("J", [2, EDGE_J, EDGE_J + 1, 1000])
def test_equal_and_saturated_logits(J):
    n = 257
    y = (np.arange(n) % J).astype(np.int64)
    flat, betas = np.full((n, J), 3.25, dtype=np.float32), [0.3, 1.0, 9.0]
    want = R.nll(flat, y, betas)
    got, _ = _device_nll(flat, y, betas)
    for k, beta in enumerate(betas):                                            # every row is log J, and g and h are exactly 0
        assert abs(want.out[k, 0] - n * math.log(J)) <= 1e-12 * n * math.log(J) and got[k, 1] == 0.0 and got[k, 2] == 0.0
        _close_sums(got[k, 0], want.out[k, 0], want.mag[k, 0], n, R.nll_per_row(J, want.amax[k]), f"nll equal logits J={J} beta={beta}")
    z = np.where(np.arange(J)[None, :] == y[:, None], 80.0, -80.0).astype(np.float32)          # an f32 softmax returns 0 and 1 here
    for targets in (y, (y + 1) % J):
        betas = [1.0, 20.0]
        want = R.nll(z, targets, betas)
        got, _ = _device_nll(z, targets, betas)
        assert np.isfinite(got).all()
        for k, beta in enumerate(betas):
            for c, name in enumerate(("nll", "g", "h")):
                _close_sums(got[k, c], want.out[k, c], want.mag[k, c], n, R.nll_per_row(J, want.amax[k]), f"{name} saturated J={J} beta={beta}")
    assert got[0, 0] > 159.0 * n                                                # the wrong label everywhere: 160 per row at beta = 1


# ------------------------------------------------------------------ softmax / arg max at a temperature
def _softmax_case(shape, regime, beta):
    """The logits of tests/test_head_gpu.py's softmax cases under its rule for the arg max: the first seed >= 7500 whose reference
    (float64, on the CPU) leaves at most 2 % of the rows with their two largest probabilities within MARGIN."""
    from tests.test_head_gpu import decided_rows, make_logits

    for seed in range(7500, 7600):
        lg = make_logits(shape[0], shape[1], regime, seed)
        want = torch.softmax(lg.double() * beta, 1)
        decided = decided_rows(want)
        if int((~decided).sum()) <= 0.02 * shape[0]:
            return lg, want, decided
    raise AssertionError(f"no seed satisfies the rule for {shape} {regime} beta={beta}")


@pytest.mark.parametrize("shape", [(1, 1), (300, 2), (7, 3), (5, 257), (6, 1000)])
def test_softmax_argmax_t_at_one_is_softmax_argmax(shape):
    from tests.test_head_gpu import make_logits, same_bits

    for regime in ("normal", "saturated", "offset", "equal"):
        lg = make_logits(shape[0], shape[1], regime, 7500).cuda()
        probs, preds = K.softmax_argmax(lg, True)
        probs_t, preds_t = K.softmax_argmax_t(lg, 1.0, True)
        same_bits(probs_t, probs, f"softmax_argmax_t at beta = 1 {shape} {regime}")
        assert torch.equal(preds_t, preds) and torch.equal(K.softmax_argmax_t(lg, 1.0, False)[1], preds)
    bad = make_logits(shape[0], shape[1], "normal", 7501)
    bad[0, 0] = float("nan")
    probs, preds = K.softmax_argmax(bad.cuda(), True)
    probs_t, preds_t = K.softmax_argmax_t(bad.cuda(), 1.0, True)
    assert torch.equal(preds_t, preds) and int(preds_t[0]) == 0 and bool(torch.isnan(probs_t[0]).all())
    assert torch.equal(torch.isnan(probs_t), torch.isnan(probs))


@pytest.mark.parametrize("beta,regime", [(0.25, "saturated"), (3.0, "normal"), (3.0, "offset")])
@pytest.mark.parametrize("shape", [(1, 1), (300, 2), (7, 3), (5, 257), (6, 1000)])
def test_softmax_argmax_t_against_float64(shape, beta, regime):
    from tests.test_head_gpu import measured

    lg, want, decided = _softmax_case(shape, regime, beta)
    probs, preds = K.softmax_argmax_t(lg.cuda(), beta, True)
    none, preds_alone = K.softmax_argmax_t(lg.cuda(), beta, False)
    assert none is None and torch.equal(preds, preds_alone)
    measured(probs, want, 1e-5, f"softmax_argmax_t {shape} {regime} beta={beta}")
    preds = preds.cpu()
    assert bool(((preds >= 0) & (preds < shape[1])).all()) and torch.equal(preds[decided], want.argmax(1)[decided])
    with pytest.raises(ValueError):
        K.softmax_argmax_t(lg.cuda(), 0.0)


# ------------------------------------------------------------------ the fit
@pytest.mark.parametrize("t0,J", [(0.5, 3), (2.0, 2), (4.0, EDGE_J + 1)])
def test_fit_temperature_equals_the_reference_fit(t0, J):
    """The device fit ends in a bracket of relative width 1e-9 around the root of its own g; the device's g differs from the
    reference's by about 1e-13 of its magnitude (test_bins_and_nll_at_every_size), which moves the root by that over h: far below
    1e-9.  So the two fits agree to 1e-6 with room to spare, and the reference's g changes sign within +-1e-6 of the device's beta."""
    logits, targets = R.planted(5000, J, t0, seed=int(10 * t0) + J)
    fit = M.fit_temperature(torch.from_numpy(logits).cuda(), torch.from_numpy(targets).cuda())
    ref = R.fit_temperature(logits, targets)
    print(f"[calib] fit T0={t0} J={J}: device T {fit.temperature!r} reference T {ref.temperature!r} rounds {fit.rounds}")
    assert not fit.at_bound and 1 <= fit.rounds <= 8 and fit.valid == 5000 and fit.nonfinite == 0
    beta = 1.0 / fit.temperature
    assert R.gradient(logits, targets, beta * (1 - 1e-6)) < 0.0 < R.gradient(logits, targets, beta * (1 + 1e-6))
    assert abs(fit.temperature - ref.temperature) <= 1e-6 * ref.temperature
    # the means: sums that agree to about 1e-12 of their magnitude (above), at betas 1e-9 apart around a minimum
    assert abs(fit.nll_before - ref.nll_before) <= 1e-10 * max(1.0, ref.nll_before)
    assert abs(fit.nll_after - ref.nll_after) <= 1e-10 * max(1.0, ref.nll_after) and fit.nll_after <= fit.nll_before
    got = M.mean_nll(torch.from_numpy(logits).cuda(), torch.from_numpy(targets).cuda(), fit.temperature)
    assert abs(got - fit.nll_after) <= 1e-10 * max(1.0, fit.nll_after)


def test_fit_temperature_at_the_bounds():
    n, J = 300, 3
    y = (np.arange(n) % J).astype(np.int64)
    z = np.where(np.arange(J)[None, :] == y[:, None], 2.0, -1.0).astype(np.float32)
    sharp = M.fit_temperature(torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda())          # separable
    assert sharp.at_bound and sharp.temperature == 0.05 and sharp.rounds == 0
    flat = M.fit_temperature(torch.from_numpy(-z).cuda(), torch.from_numpy(y).cuda())          # labels opposite to the logits
    assert flat.at_bound and flat.temperature == 100.0 and flat.rounds == 0
    with pytest.raises(ValueError, match="outside"):
        M.fit_temperature(torch.from_numpy(z).cuda(), torch.from_numpy(y + 1).cuda())


# ------------------------------------------------------------------ end to end
def _config(tmp_path: Path, out: str, calibration) -> Path:
    import yaml

    infer = {"split": "test", "batch_size": 8, "num_workers": 0, "img_size": 64, "gpu_resize": True, "robustness": {"blur_sigma": [2]},
             "device_metrics": True}
    if calibration is not None:
        infer["calibration"] = calibration
    cfg = {"seed": 1, "device": "cuda",
           "data": {"root": str(tmp_path / "data"), "val_split": "val", "test_split": "test", "num_classes": 2, "img_size": 64},
           "models": {"efficientnet_b0": {"output_dir": str(tmp_path / out), "inference": infer}}, "selection": ["efficientnet_b0"]}
    path = tmp_path / f"{out}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return path


def _run(base: Path) -> Path:
    (run,) = [p for p in base.iterdir() if p.is_dir()]
    return run


def test_inference_with_calibration(tmp_path, monkeypatch):
    from deepfakedetection_amd.orchestration import orchestrator as O
    from tests.test_plumbing_cpu import _make_dataset

    _make_dataset(tmp_path / "data", classes=("fake", "real"), per_class=4, size=64)
    books = []
    real = O._split_metrics_device
    monkeypatch.setattr(O, "_split_metrics_device",
                        lambda name, split, book, J, thr: (books.append((book.probs.clone(), book.targets.clone(), book._logits is not None)),
                                                           real(name, split, book, J, thr))[1])
    O.orchestrate(_config(tmp_path, "calib", {"bins": 10, "temperature": "fit"}), mode="inference")
    O.orchestrate(_config(tmp_path, "fixed", {"temperature": 2.0}), mode="inference")
    O.orchestrate(_config(tmp_path, "plain", None), mode="inference")
    today = {"model", "split", "accuracy", "timestamp", "threshold", "confusion_matrix", "roc_auc", "eer", "balanced_accuracy"}
    new = {"temperature", "ece", "mce", "brier", "nll"}
    rows = {out: [json.loads(s) for s in (_run(tmp_path / out) / "logs" / "metrics.jsonl").read_text().splitlines()]
            for out in ("calib", "fixed", "plain")}
    assert [kept for _, _, kept in books] == [True, True, True, True, False, False]
    for row in rows["plain"]:
        assert set(row) - {"perturbation"} == today
    assert not (_run(tmp_path / "plain") / "calibration.json").exists() and not (_run(tmp_path / "plain") / "plots" / "reliability.png").exists()
    for out, bins in (("calib", 10), ("fixed", 15)):
        run = _run(tmp_path / out)
        clean, blurred = rows[out]
        assert set(clean) - {"temperature_fit"} == today | new | {"uncalibrated"} and set(clean["uncalibrated"]) == {"ece", "mce", "brier", "nll"}
        assert set(blurred) == today | new | {"perturbation"}
        doc = json.loads((run / "calibration.json").read_text())
        assert set(doc) - {"temperature_fit"} == {"temperature", "bins", "fitted_on", "n", "nll_before", "nll_after"} and doc["bins"] == bins
        assert (run / "plots" / "reliability.png").stat().st_size > 0
        assert clean["temperature"] == blurred["temperature"] == doc["temperature"]
        for row, (probs, targets, _) in zip((clean, blurred), books[:2] if out == "calib" else books[2:4]):
            res = M.calibration(probs, targets, bins)
            assert (row["ece"], row["mce"], row["brier"]) == (res.ece, res.mce, res.brier)
            assert 0.0 <= row["ece"] <= row["mce"] <= 1.0 and row["nll"] > 0.0
    doc = json.loads((_run(tmp_path / "calib") / "calibration.json").read_text())
    assert doc["fitted_on"] == "val" and doc["n"] == 8 and doc["nll_before"] > 0.0
    if "temperature_fit" in doc:                                                # an untrained network may put the minimum at a bound
        assert doc["temperature_fit"] == "at_bound" == rows["calib"][0]["temperature_fit"] and doc["temperature"] == 1.0
    else:
        assert 0.05 < doc["temperature"] < 100.0 and doc["nll_after"] <= doc["nll_before"]
    fixed = json.loads((_run(tmp_path / "fixed") / "calibration.json").read_text())
    assert fixed["temperature"] == 2.0 and fixed["fitted_on"] is None and rows["fixed"][0]["temperature"] == 2.0
    assert abs(rows["fixed"][0]["uncalibrated"]["nll"] - rows["calib"][0]["uncalibrated"]["nll"]) <= 1e-6      # T = 1 in both runs
