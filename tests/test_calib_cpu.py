"""No-GPU checks of the calibration feature: the numpy / integer reference (tests/_calib_ref.py) against a brute-force loop over the
samples and against scipy; the reference fitter's sign-change certificate and a planted temperature; the argument checks of the new
entry points through the raw ABI (nothing is launched); dfd_calib_plan at both sides of its boundaries; ScoreBook with and without
logits; and the orchestrator's `inference.calibration` key on a CPU device."""

from __future__ import annotations

import ctypes
import json
import math

import numpy as np
import pytest
import torch

from deepfakedetection_amd import _lib
from deepfakedetection_amd import metrics as M
from tests import _calib_ref as R


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        from deepfakedetection_amd.build import build

        build()
    return _lib.load()


def _probs(seed: int, n: int, J: int, grid: int | None = 256):
    """n rows of f32 probabilities (on a grid of 1 / `grid`, so confidences sit on bin edges and tie; None: continuous) and targets
    that agree with the arg max about two times in three."""
    rng = np.random.default_rng(seed)
    if grid is None:
        p = rng.dirichlet(np.ones(J), size=n)
    else:
        cuts = np.sort(rng.integers(0, grid + 1, size=(n, J - 1)), axis=1)
        p = np.diff(np.concatenate([np.zeros((n, 1)), cuts, np.full((n, 1), grid)], axis=1), axis=1) / grid
    p = p.astype(np.float32)
    y = np.where(rng.random(n) < 0.66, p.argmax(axis=1), rng.integers(0, J, size=n)).astype(np.int64)
    return p, y


def _brute_bins(probs, targets, M_bins):
    table = [[0, 0, 0] for _ in range(M_bins)]
    stats = [0, 0, 0, 0]
    terms = []
    for row, y in zip(probs.tolist(), targets.tolist()):
        if any(math.isnan(v) or math.isinf(v) for v in row):
            stats[1] += 1
            continue
        if not 0 <= y < len(row):
            stats[2] += 1
            continue
        conf = max(row)
        pred = row.index(conf)
        b = sum(1 for k in range(1, M_bins) if conf > k / M_bins)              # Python floats are float64
        q = int(round(conf * 4294967296.0))                                     # round(): ties to even, like llrint
        table[b][0] += 1
        table[b][1] += pred == y
        table[b][2] += q
        stats[0] += 1
        stats[3] += pred == y
        terms += [(v - (j == y)) ** 2 for j, v in enumerate(row)]
    return table, stats, math.fsum(terms)


@pytest.mark.parametrize("n,J,M_bins,grid", [(1, 2, 15, 256), (300, 2, 4, 256), (300, 3, 8, 256), (300, 5, 16, 256), (200, 7, 15, None),
                                            (257, 2, 15, 15)])
def test_bins_reference_equals_brute_force(n, J, M_bins, grid):
    probs, targets = _probs(n, n, J, grid)
    if n > 10:
        probs[3, 0] = np.nan
        probs[5, J - 1] = np.inf
        targets[7], targets[9] = -1, J
        probs[11] = 0.0                                                         # conf == 0
        probs[12] = 0.0
        probs[12, J - 1] = 1.0                                                  # conf == 1
    ref = R.bins(probs, targets, M_bins)
    table, stats, brier = _brute_bins(probs, targets, M_bins)
    assert ref.table == table and ref.stats == stats
    assert abs(ref.brier_sum - brier) <= 4 * R.U * brier                        # two fsums of terms that differ by a rounding each
    ece, mce = R.ece_mce(ref.table, ref.stats[0])
    want = sum(abs(c - q / R.Q_ONE) for _, c, q in table) / stats[0]
    assert abs(ece - want) < 1e-12 and 0.0 <= ece <= mce <= 1.0


def test_bin_edges_are_right_closed():
    for M_bins in (4, 8, 15, 16):
        edges = np.array([np.float32(k / M_bins) for k in range(M_bins + 1)])
        assert R.bin_index(edges, M_bins).tolist() == [0] + [k - 1 if float(edges[k]) <= k / M_bins else k for k in range(1, M_bins)] + [M_bins - 1]
        above = np.nextafter(edges, np.float32(2.0))
        assert R.bin_index(above[:-1], M_bins).tolist() == [0 if k == 0 else (k if float(above[k]) > k / M_bins else k - 1)
                                                            for k in range(M_bins)]
    assert R.bin_index(np.array([-0.5, 0.0, 1.0, 1.5], dtype=np.float32), 15).tolist() == [0, 0, 14, 14]
    assert R.quantise(np.array([0.0, 0.5, 1.0, 2.0 ** -9], dtype=np.float32)).tolist() == [0, 1 << 31, 1 << 32, 1 << 23]


def _brute_nll(logits, targets, beta):
    out = [[], [], []]
    for row, y in zip(logits.tolist(), targets.tolist()):
        if any(math.isnan(v) or math.isinf(v) for v in row) or not 0 <= y < len(row):
            continue
        a = [beta * v for v in row]
        m = max(a)
        e = [math.exp(v - m) for v in a]
        s = math.fsum(e)
        mean1 = math.fsum(ej * zj for ej, zj in zip(e, row)) / s
        mean2 = math.fsum(ej * zj * zj for ej, zj in zip(e, row)) / s
        out[0].append(m + math.log(s) - a[y])
        out[1].append(mean1 - row[y])
        out[2].append(mean2 - mean1 * mean1)
    return [math.fsum(v) for v in out]


@pytest.mark.parametrize("n,J", [(1, 2), (200, 2), (200, 3), (100, 17)])
def test_nll_reference_equals_brute_force(n, J):
    rng = np.random.default_rng(n + J)
    logits = (rng.standard_normal((n, J)) * 3).astype(np.float32)
    targets = rng.integers(0, J, size=n).astype(np.int64)
    if n > 10:
        logits[2, 0], logits[4, J - 1] = np.nan, -np.inf
        targets[6], targets[8] = -1, J
    betas = [0.01, 0.5, 1.0, 3.0, 20.0]
    ref = R.nll(logits, targets, betas)
    assert ref.stats == ([2, 2] if n > 10 else [0, 0]) and ref.valid == n - sum(ref.stats)
    for k, beta in enumerate(betas):
        want = _brute_nll(logits, targets, beta)
        for c in range(3):
            assert abs(ref.out[k, c] - want[c]) <= R.sum_bound(ref.mag[k, c], 1, R.nll_per_row(J, ref.amax[k])), (beta, c)
    eps = 1e-6                                                                  # g and h are the derivatives of nll
    mid = R.nll(logits, targets, [1.0 - eps, 1.0, 1.0 + eps]).out
    assert abs((mid[2, 0] - mid[0, 0]) / (2 * eps) - mid[1, 1]) <= 1e-6 * max(1.0, abs(mid[1, 1]))
    assert abs((mid[2, 1] - mid[0, 1]) / (2 * eps) - mid[1, 2]) <= 1e-6 * max(1.0, abs(mid[1, 2]))


def test_nll_of_equal_and_saturated_logits():
    n, J = 50, 7
    ref = R.nll(np.full((n, J), 3.25, dtype=np.float32), np.arange(n) % J, [0.3, 1.0, 9.0])
    assert np.allclose(ref.out[:, 0], n * math.log(J), rtol=1e-15) and np.all(ref.out[:, 1:] == 0.0)
    z = np.where(np.arange(J)[None, :] == (np.arange(n) % J)[:, None], 80.0, -80.0).astype(np.float32)
    ref = R.nll(z, np.arange(n) % J, [1.0, 20.0])
    assert np.isfinite(ref.out).all() and np.all(ref.out[:, 0] >= 0.0) and np.all(ref.out[:, 0] < 1e-60)


# The planted temperature.  Labels are drawn from softmax(z) and the logits handed over as T0 z, so the expected NLL is minimised at
# T = T0 exactly and the fitted T is a maximum-likelihood estimate of it.  In beta the estimate's variance is 1 / (summed Fisher
# information) = 1 / h(beta*), with h the second derivative the reference itself returns; in T = 1 / beta that is a standard
# deviation of T^2 / sqrt(h) (delta method).  The margin is 5 of those standard deviations: a false alarm rate below 1e-6 per case
# under the normal approximation, which n = 20 000 makes accurate.
@pytest.mark.parametrize("t0", [0.5, 2.0, 4.0])
def test_reference_fitter_recovers_a_planted_temperature(t0):
    logits, targets = R.planted(20_000, 3, t0, seed=int(t0 * 10))
    fit = R.fit_temperature(logits, targets)
    assert not fit.at_bound and 1 <= fit.rounds <= R.MAX_ROUNDS
    assert R.gradient(logits, targets, fit.beta * (1 - 1e-6)) < 0.0 < R.gradient(logits, targets, fit.beta * (1 + 1e-6))
    h = R.nll(logits, targets, [fit.beta]).out[0, 2]
    sigma_t = fit.temperature ** 2 / math.sqrt(h)
    assert abs(fit.temperature - t0) <= 5.0 * sigma_t, (fit.temperature, t0, sigma_t)
    assert sigma_t < 0.05 * t0                                                  # the margin itself is tight: a few per cent of T0
    assert fit.nll_after <= fit.nll_before + 1e-12


def test_reference_fitter_stops_at_the_bounds():
    n, J = 64, 3
    y = np.arange(n) % J
    z = np.where(np.arange(J)[None, :] == y[:, None], 2.0, -1.0).astype(np.float32)
    sharp = R.fit_temperature(z, y)                                             # separable: the NLL falls as beta grows
    assert sharp.at_bound and sharp.temperature == 0.05 and sharp.rounds == 0
    flat = R.fit_temperature(-z, y)                                             # labels opposite to the logits
    assert flat.at_bound and flat.temperature == 100.0 and flat.rounds == 0


def test_reference_fitter_agrees_with_scipy():
    optimize = pytest.importorskip("scipy.optimize")
    logits, targets = R.planted(5000, 4, 1.7, seed=3)
    fit = R.fit_temperature(logits, targets)
    res = optimize.minimize_scalar(lambda b: R.nll(logits, targets, [b]).out[0, 0], bounds=(0.01, 20.0), method="bounded",
                                   options={"xatol": 1e-10})
    assert abs(res.x - fit.beta) <= 1e-5 * fit.beta                             # Brent on the function values: sqrt(eps)-limited


# ------------------------------------------------------------------ the ABI without a device
def test_abi_constants_and_sources(lib):
    from deepfakedetection_amd.build import SOURCES

    assert lib.dfd_version() >= 150 and "dfd_calib.hip" in SOURCES
    header = (_lib.LIB_PATH.parents[1] / "include" / "dfd_hip.h").read_text()
    for name, value in (("DFD_CALIB_MAX_J", _lib.CALIB_MAX_J), ("DFD_CALIB_MAX_BINS", _lib.CALIB_MAX_BINS),
                        ("DFD_CALIB_MAX_BETAS", _lib.CALIB_MAX_BETAS), ("DFD_CALIB_THREAD_MAX_J", _lib.CALIB_THREAD_MAX_J),
                        ("DFD_CALIB_MAX_BLOCKS", _lib.CALIB_MAX_BLOCKS), ("DFD_CALIB_STAGE2_WIDTH", _lib.CALIB_STAGE2_WIDTH),
                        ("DFD_CALIB_LAYOUT_THREAD", _lib.CALIB_LAYOUT_THREAD), ("DFD_CALIB_LAYOUT_WAVE", _lib.CALIB_LAYOUT_WAVE)):
        assert f"#define {name} {value}\n" in header, name
    assert "#define DFD_CALIB_MAX_N (1 << 28)" in header and _lib.CALIB_MAX_N == 1 << 28
    assert (_lib.CALIB_MAX_J, _lib.CALIB_MAX_BINS, _lib.CALIB_MAX_BETAS) == (1024, 64, 64)
    for name in ("CalibrationResult", "TemperatureFit", "calibration", "fit_temperature"):
        assert name in M.__all__ and hasattr(M, name)


def test_bad_arguments_are_rejected_without_a_gpu(lib):
    EINVAL, EWORKSPACE = -1, -4
    one, big = 0x1000, 1 << 30                                      # a non-null address: rejected calls launch nothing
    MAX_N, MAX_J = _lib.CALIB_MAX_N, _lib.CALIB_MAX_J
    # dfd_calib_bins(probs, targets, n, J, M, ws, ws_bytes, bins, stats, brier, stream)
    assert lib.dfd_calib_bins_ws(-1, 2) == 0 and lib.dfd_calib_bins_ws(MAX_N + 1, 2) == 0
    assert lib.dfd_calib_bins_ws(8, 0) == 0 and lib.dfd_calib_bins_ws(8, MAX_J + 1) == 0 and lib.dfd_calib_bins_ws(0, 2) > 0
    for n, J, bins in ((-1, 2, 15), (MAX_N + 1, 2, 15), (8, 0, 15), (8, MAX_J + 1, 15), (8, 2, 0), (8, 2, _lib.CALIB_MAX_BINS + 1)):
        assert lib.dfd_calib_bins(one, one, n, J, bins, one, big, one, one, one, None) == EINVAL, (n, J, bins)
    for hole in range(6):                                           # probs, targets, ws, bins, stats, brier
        ptrs = [one] * 6
        ptrs[hole] = None
        assert lib.dfd_calib_bins(ptrs[0], ptrs[1], 8, 2, 15, ptrs[2], big, ptrs[3], ptrs[4], ptrs[5], None) == EINVAL, hole
    assert lib.dfd_calib_bins(one, one, 8, 2, 15, one, lib.dfd_calib_bins_ws(8, 2) - 1, one, one, one, None) == EWORKSPACE
    # dfd_calib_nll(logits, targets, n, J, betas (host), K, ws, ws_bytes, out, stats, stream)
    good = (ctypes.c_double * 3)(0.01, 1.0, 20.0)
    many = (ctypes.c_double * (_lib.CALIB_MAX_BETAS + 1))(*([1.0] * (_lib.CALIB_MAX_BETAS + 1)))
    assert lib.dfd_calib_nll_ws(-1, 2, 3) == 0 and lib.dfd_calib_nll_ws(MAX_N + 1, 2, 3) == 0 and lib.dfd_calib_nll_ws(8, MAX_J + 1, 3) == 0
    assert lib.dfd_calib_nll_ws(8, 2, 0) == 0 and lib.dfd_calib_nll_ws(8, 2, _lib.CALIB_MAX_BETAS + 1) == 0
    assert lib.dfd_calib_nll_ws(8, 2, 3) == (3 * 3 + 2) * 8 and lib.dfd_calib_nll_ws(0, 2, 1) > 0
    for n, J in ((-1, 2), (MAX_N + 1, 2), (8, 0), (8, MAX_J + 1)):
        assert lib.dfd_calib_nll(one, one, n, J, good, 3, one, big, one, one, None) == EINVAL, (n, J)
    assert lib.dfd_calib_nll(one, one, 8, 2, good, 0, one, big, one, one, None) == EINVAL
    assert lib.dfd_calib_nll(one, one, 8, 2, many, _lib.CALIB_MAX_BETAS + 1, one, big, one, one, None) == EINVAL
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        betas = (ctypes.c_double * 3)(0.5, bad, 2.0)
        assert lib.dfd_calib_nll(one, one, 8, 2, betas, 3, one, big, one, one, None) == EINVAL, bad
    for hole in range(5):                                           # logits, targets, ws, out, stats
        ptrs = [one] * 5
        ptrs[hole] = None
        assert lib.dfd_calib_nll(ptrs[0], ptrs[1], 8, 2, good, 3, ptrs[2], big, ptrs[3], ptrs[4], None) == EINVAL, hole
    assert lib.dfd_calib_nll(one, one, 8, 2, None, 3, one, big, one, one, None) == EINVAL
    assert lib.dfd_calib_nll(one, one, 8, 2, good, 3, one, lib.dfd_calib_nll_ws(8, 2, 3) - 1, one, one, None) == EWORKSPACE
    # dfd_calib_plan(n, J, out)
    out = (ctypes.c_int * 4)()
    for n, J in ((-1, 2), (MAX_N + 1, 2), (8, 0), (8, MAX_J + 1)):
        assert lib.dfd_calib_plan(n, J, out) == EINVAL, (n, J)
    assert lib.dfd_calib_plan(8, 2, None) == EINVAL
    # dfd_softmax_argmax_t(logits, N, J, inv_temperature, probs, preds, stream)
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.dfd_softmax_argmax_t(one, 4, 2, beta, one, one, None) == EINVAL, beta
    assert lib.dfd_softmax_argmax_t(None, 4, 2, 1.0, one, one, None) == EINVAL and lib.dfd_softmax_argmax_t(one, 4, 2, 1.0, one, None, None) == EINVAL
    assert lib.dfd_softmax_argmax_t(one, 0, 2, 1.0, one, one, None) == EINVAL and lib.dfd_softmax_argmax_t(one, 4, 0, 1.0, one, one, None) == EINVAL


def test_plan_on_both_sides_of_every_boundary():
    from deepfakedetection_amd import kernels as K

    T, W = K.CALIB_LAYOUT_THREAD, K.CALIB_LAYOUT_WAVE
    edge = K.CALIB_THREAD_MAX_J
    assert K.calib_plan(100, edge).layout == T and K.calib_plan(100, edge + 1).layout == W             # the layout boundary in J
    assert K.calib_plan(100, 1).layout == T and K.calib_plan(100, K.CALIB_MAX_J).layout == W
    for J, layout in ((2, T), (edge, T), (edge + 1, W), (1000, W)):
        rows = K.calib_plan(1, J).rows
        assert rows == (256 if layout == T else 32)
        assert K.calib_plan(0, J) == K.CalibPlan(layout, rows, 1, 1)                                    # an empty input: one workgroup
        assert K.calib_plan(rows, J).blocks == 1 and K.calib_plan(rows + 1, J).blocks == 2              # a second workgroup
        width = K.CALIB_STAGE2_WIDTH
        assert K.calib_plan(width * rows, J) == K.CalibPlan(layout, rows, width, 1)                     # a second stage-2 trip
        assert K.calib_plan(width * rows + 1, J) == K.CalibPlan(layout, rows, width + 1, 2)
        cap = K.CALIB_MAX_BLOCKS
        assert K.calib_plan(cap * rows, J).blocks == cap and K.calib_plan(cap * rows + 1, J).blocks == cap   # the cap: strides from here
        assert K.calib_plan(K.CALIB_MAX_N, J) == K.CalibPlan(layout, rows, cap, cap // width)
    with pytest.raises(RuntimeError, match="DFD_EINVAL"):
        K.calib_plan(8, K.CALIB_MAX_J + 1)


# ------------------------------------------------------------------ ScoreBook and the orchestrator on the CPU
def test_score_book_with_and_without_logits():
    rng = np.random.default_rng(0)
    plain = M.ScoreBook(10, 3, "cpu")
    assert plain._logits is None and [tuple(t.shape) for t in (plain._probs, plain._preds, plain._targets)] == [(10, 3), (10,), (10,)]
    p = torch.from_numpy(rng.random((4, 3)).astype(np.float32))
    plain.append(p, torch.arange(4), torch.arange(4) % 3)
    assert plain.count == 4 and torch.equal(plain.probs, p)
    with pytest.raises(ValueError, match="keep_logits"):
        plain.logits
    with pytest.raises(ValueError, match="keep_logits"):
        plain.append(p, torch.arange(4), torch.arange(4) % 3, logits=p)
    assert plain.count == 4                                                     # the refused batch left nothing behind

    book = M.ScoreBook(10, 3, "cpu", keep_logits=True)
    z1, z2 = torch.from_numpy(rng.standard_normal((4, 3)).astype(np.float32)), torch.from_numpy(rng.standard_normal((5, 3)).astype(np.float32))
    book.append(p, torch.arange(4), torch.arange(4) % 3, logits=z1)
    book.append(None, None, torch.arange(5) % 3, logits=z2)
    assert book.count == 9 and torch.equal(book.logits, torch.cat([z1, z2])) and book.logits.dtype == torch.float32
    with pytest.raises(ValueError, match="expected shape"):
        book.append(None, None, torch.zeros(1, dtype=torch.int64), logits=torch.zeros(1, 2))
    with pytest.raises(ValueError, match="overflow"):
        book.append(None, None, torch.zeros(2, dtype=torch.int64))
    book.reset()
    assert book.count == 0 and book.logits.shape == (0, 3)


def test_calibration_settings_parse():
    from deepfakedetection_amd.orchestration.orchestrator import calibration_settings

    assert calibration_settings({}) is None and calibration_settings({"calibration": False}) is None
    assert calibration_settings({"calibration": {}}) == (15, "fit") == calibration_settings({"calibration": True})
    assert calibration_settings({"calibration": {"bins": 10, "temperature": "off"}}) == (10, 1.0)
    assert calibration_settings({"calibration": {"temperature": False}}) == (15, 1.0)          # YAML's reading of a bare `off`
    assert calibration_settings({"calibration": {"temperature": 1.5}}) == (15, 1.5) == calibration_settings({"calibration": {"temperature": "1.5"}})
    for bad in ({"bins": 0}, {"bins": 65}, {"temperature": 0}, {"temperature": -2.0}, {"temperature": "warm"}):
        with pytest.raises(ValueError):
            calibration_settings({"calibration": bad})
    with pytest.raises(ValueError):
        calibration_settings({"calibration": 15})


def test_class_probabilities_hands_back_the_logits_on_request():
    from deepfakedetection_amd.orchestration.orchestrator import class_probabilities

    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(12, 3)).eval()
    x = torch.randn(5, 3, 2, 2)
    probs, preds = class_probabilities(model, x, torch.device("cpu"))
    probs2, preds2, logits = class_probabilities(model, x, torch.device("cpu"), return_logits=True)
    assert torch.equal(probs, probs2) and torch.equal(preds, preds2) and logits.dtype == torch.float32
    assert torch.equal(torch.softmax(logits, dim=1), probs)


def test_orchestrator_ignores_the_key_off_device(tmp_path, capsys, monkeypatch):
    """The networks run on a HIP device only, so a small torch model stands in for the checkpoint: what is under test is the job
    around it."""
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
    for out, extra in (("plain", {}), ("calib", {"device_metrics": True, "calibration": {"bins": 15, "temperature": "fit"}})):
        infer = {"split": "test", "batch_size": 4, "num_workers": 0, "img_size": 32, **extra}
        cfg = {"seed": 1, "device": "cpu",
               "data": {"root": str(tmp_path / "data"), "val_split": "val", "test_split": "test", "num_classes": 2, "img_size": 32},
               "models": {"efficientnet_b0": {"output_dir": str(tmp_path / out), "inference": infer}}, "selection": ["efficientnet_b0"]}
        path = tmp_path / f"{out}.yaml"
        path.write_text(yaml.safe_dump(cfg))
        O.orchestrate(path, mode="inference")
        (run,) = [p for p in (tmp_path / out).iterdir() if p.is_dir()]
        rows[out] = [json.loads(s) for s in (run / "logs" / "metrics.jsonl").read_text().splitlines()]
        assert not (run / "calibration.json").exists() and not (run / "plots" / "reliability.png").exists()
        text = capsys.readouterr().out
        assert ("inference.calibration ignored" in text) == (out == "calib")
        assert ("inference.device_metrics ignored" in text) == (out == "calib")
    assert len(rows["plain"]) == len(rows["calib"]) == 1
    assert set(rows["plain"][0]) == set(rows["calib"][0]) and "ece" not in rows["calib"][0] and "temperature" not in rows["calib"][0]
    assert set(rows["plain"][0]) - {"roc_auc"} == {"model", "split", "accuracy", "timestamp", "threshold", "confusion_matrix"}
