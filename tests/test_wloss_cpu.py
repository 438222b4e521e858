"""Class-weighted / focal cross entropy and class-balanced sampling, the parts that need no device: the float64 reference
(tests/_wloss_ref.py) against torch and against independent restatements, the trainer settings, the ABI 147 argument checks and
dp.BalancedShardedSampler."""

from __future__ import annotations

import ctypes
import math

import pytest
import torch

from deepfakedetection_amd import _lib
from tests import _wloss_ref as W

_VARS = ("CLASS_WEIGHTS", "FOCAL_GAMMA", "BALANCED_SAMPLING")


def _case(N: int, J: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((N, J), generator=g, dtype=torch.float64) * 2
    hard = torch.randint(0, J, (N,), generator=g)
    hard[0], hard[-1] = 0, J - 1
    soft = torch.softmax(torch.randn((N, J), generator=g, dtype=torch.float64), 1)
    w = torch.rand(J, generator=g, dtype=torch.float64) * 3.75 + 0.25
    if J > 2:
        w[1] = 0.0
    return logits, hard, soft, w


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("J", [2, 3, 257])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["index", "probability"])
def test_reference_without_focusing_is_torch_cross_entropy(kind, eps, J):
    """gamma = 0: torch.nn.functional.cross_entropy(weight=, label_smoothing=) in float64, value and gradient, to 1e-12.  This pins
    the denominator: sum_n w[t_n] for class indices, N for probabilities."""
    logits, hard, soft, w = _case(9, J, 100 + J)
    target = hard if kind == "index" else soft
    for weight in (w, None):
        ref = logits.clone().requires_grad_(True)
        want = torch.nn.functional.cross_entropy(ref, target, weight=weight, label_smoothing=eps)
        (dwant,) = torch.autograd.grad(want, ref)
        want = want.detach()
        got, dgot = W.loss_and_grad(logits, target, weight, eps, 0.0)
        assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want))), (float(got), float(want))
        assert float((dgot - dwant).abs().max()) <= 1e-12 * max(1.0, float(dwant.abs().max()))


def test_reference_is_nan_where_torch_is_when_the_targets_have_no_weight():
    logits, hard, _, _ = _case(5, 3, 7)
    w = torch.tensor([0.0, 0.0, 0.0], dtype=torch.float64)
    want = torch.nn.functional.cross_entropy(logits, hard, weight=w)
    assert math.isnan(float(want)) and math.isnan(float(W.loss(logits, hard, w, 0.0, 0.0)))
    # label smoothing gives the rows a positive sum through the one class that has weight: torch still answers NaN, not inf
    w = torch.tensor([0.0, 1.5, 0.0], dtype=torch.float64)
    hard = torch.tensor([0, 2, 0, 2, 2])
    want = torch.nn.functional.cross_entropy(logits, hard, weight=w, label_smoothing=0.1)
    assert math.isnan(float(want)) and math.isnan(float(W.loss(logits, hard, w, 0.1, 0.0)))
    assert math.isnan(float(W.loss(logits, hard, w, 0.1, 2.0)))


@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0, 5.0])
def test_reference_is_the_focal_loss_of_the_target(gamma):
    """w = 1, eps = 0, class indices: mean_n (1 - p_t)^gamma * (-log p_t), written out on its own."""
    logits, hard, _, _ = _case(11, 5, 200)
    p = torch.softmax(logits, 1)
    pt = p[torch.arange(11), hard]
    want = ((1 - pt) ** gamma * -pt.log()).mean()
    got = W.loss(logits, hard, None, 0.0, gamma)
    assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))


@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 5.0])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["index", "probability"])
def test_reference_gradient_is_the_closed_form(kind, eps, gamma):
    for J in (1, 2, 3, 17):
        logits, hard, soft, w = _case(6, J, 300 + J)
        target = hard if kind == "index" else soft
        _, grad = W.loss_and_grad(logits, target, w, eps, gamma)
        closed = W.closed_form_grad(logits, target, w, eps, gamma)
        assert float((grad - closed).abs().max()) <= 1e-12 * max(1.0, float(closed.abs().max())), (J, kind, eps, gamma)


def test_reference_stays_finite_beside_minus_infinity_off_the_target():
    logits, hard, _, w = _case(6, 4, 400)
    hole = (hard + 1) % 4
    logits[torch.arange(6), hole] = -float("inf")
    for gamma in (0.0, 2.0):
        loss, grad = W.loss_and_grad(logits, hard, w, 0.0, gamma)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
        assert int(torch.count_nonzero(grad[torch.arange(6), hole])) == 0
        assert bool(torch.isfinite(W.closed_form_grad(logits, hard, w, 0.0, gamma)).all())


# ------------------------------------------------------------------ settings
def _clear(monkeypatch):
    for var in _VARS:
        monkeypatch.delenv(var, raising=False)


def test_settings_are_off_by_default(monkeypatch):
    from deepfakedetection_amd.trainers import _engine as E
    from deepfakedetection_amd.trainers._inputs import balanced_sampling

    _clear(monkeypatch)
    assert E.loss_settings(2) is None and balanced_sampling() is False
    monkeypatch.setenv("FOCAL_GAMMA", "0")
    assert E.loss_settings(2) is None
    crit, _ = E._make_criterion_and_optimizer(False)
    assert isinstance(crit, torch.nn.CrossEntropyLoss) and crit.weight is None and crit.label_smoothing == 0.1


def test_balanced_weights_from_counts():
    from deepfakedetection_amd.trainers import _engine as E

    assert E.balanced_class_weights((10, 40)) == (2.5, 0.625)
    with pytest.raises(ValueError, match="none of: real"):
        E.balanced_class_weights((10, 0), names=("fake", "real"))
    with pytest.raises(ValueError, match="none of: 1"):
        E.balanced_class_weights((10, 0))
    cfg = E.LossSettings(class_weights="balanced", focal_gamma=2.0)
    done = E.resolve_loss_settings(cfg, [0] * 10 + [1] * 40, 2)
    assert done.class_weights == (2.5, 0.625) and done.focal_gamma == 2.0
    with pytest.raises(ValueError, match="none of: c"):         # a class the folder lists and no picture belongs to
        E.resolve_loss_settings(cfg, [0] * 10 + [1] * 40, 3, names=("a", "b", "c"))
    fixed = E.LossSettings(class_weights=(1.0, 3.0), focal_gamma=0.0)
    assert E.resolve_loss_settings(fixed, [0, 1], 2) is fixed and E.resolve_loss_settings(None, [0, 1], 2) is None


def test_settings_from_environment(monkeypatch):
    from deepfakedetection_amd.trainers import _engine as E
    from deepfakedetection_amd.trainers._inputs import balanced_sampling

    _clear(monkeypatch)
    monkeypatch.setenv("CLASS_WEIGHTS", "balanced")
    assert E.loss_settings(2) == E.LossSettings(class_weights="balanced", focal_gamma=0.0)
    monkeypatch.setenv("CLASS_WEIGHTS", "2.5, 0.625")
    monkeypatch.setenv("FOCAL_GAMMA", "2")
    assert E.loss_settings(2) == E.LossSettings(class_weights=(2.5, 0.625), focal_gamma=2.0)
    monkeypatch.setenv("CLASS_WEIGHTS", "[2.5, 0.625]")         # what str() makes of a YAML list
    assert E.loss_settings(2).class_weights == (2.5, 0.625)
    with pytest.raises(ValueError, match="3 classes"):
        E.loss_settings(3)
    monkeypatch.setenv("CLASS_WEIGHTS", "1,2,3")
    with pytest.raises(ValueError, match="2 classes"):
        E.loss_settings(2)
    monkeypatch.setenv("CLASS_WEIGHTS", "1,-2")
    with pytest.raises(ValueError, match=">= 0"):
        E.loss_settings(2)
    monkeypatch.setenv("CLASS_WEIGHTS", "1,inf")
    with pytest.raises(ValueError, match="finite"):
        E.loss_settings(2)
    monkeypatch.setenv("CLASS_WEIGHTS", "1,heavy")
    with pytest.raises(ValueError, match="numbers"):
        E.loss_settings(2)
    monkeypatch.delenv("CLASS_WEIGHTS")
    assert E.loss_settings(2) == E.LossSettings(class_weights=None, focal_gamma=2.0)
    monkeypatch.setenv("FOCAL_GAMMA", "-0.5")
    with pytest.raises(ValueError, match="focal_gamma"):
        E.loss_settings(2)
    monkeypatch.setenv("FOCAL_GAMMA", "nan")
    with pytest.raises(ValueError, match="focal_gamma"):
        E.loss_settings(2)
    for text, want in (("1", True), ("true", True), ("True", True), ("0", False), ("off", False)):
        monkeypatch.setenv("BALANCED_SAMPLING", text)
        assert balanced_sampling() is want


def test_yaml_keys_reach_the_trainers_environment():
    from pathlib import Path

    from deepfakedetection_amd.orchestration.orchestrator import _EXTRA_TRAIN_ENV, RunPaths, build_env_overrides

    pairs = dict(_EXTRA_TRAIN_ENV)
    assert pairs["class_weights"] == "CLASS_WEIGHTS" and pairs["focal_gamma"] == "FOCAL_GAMMA"
    assert pairs["balanced_sampling"] == "BALANCED_SAMPLING"
    run = Path("/nonexistent/run")

    def env(training):
        cfg = {"data": {"root": "."}, "models": {"efficientnet_b0": {"training": training}}}
        return build_env_overrides(config=cfg, model_cfg={"name": "efficientnet_b0", "training": training},
                                   run_paths=RunPaths(run, run / "c", run / "l", run / "p"), training=True)

    got = env({"epochs": 1, "class_weights": [2.5, 0.625], "focal_gamma": 2.0, "balanced_sampling": True})
    assert (got["CLASS_WEIGHTS"], got["FOCAL_GAMMA"], got["BALANCED_SAMPLING"]) == ("[2.5, 0.625]", "2.0", "True")
    assert env({"epochs": 1, "class_weights": "balanced"})["CLASS_WEIGHTS"] == "balanced"
    assert not set(_VARS) & set(env({"epochs": 1}))


def test_cpu_criteria_and_the_plain_evaluation_criterion():
    from deepfakedetection_amd.optim import HipCrossEntropyLoss
    from deepfakedetection_amd.trainers import _engine as E

    cfg = E.LossSettings(class_weights=(2.5, 0.625), focal_gamma=0.0)
    crit, _ = E._make_criterion_and_optimizer(False, cfg)
    assert isinstance(crit, torch.nn.CrossEntropyLoss) and crit.weight.tolist() == [2.5, 0.625] and crit.label_smoothing == 0.1
    with pytest.raises(RuntimeError, match="HIP device"):
        E._make_criterion_and_optimizer(False, E.LossSettings(class_weights=None, focal_gamma=2.0))
    with pytest.raises(ValueError, match="balanced"):
        E._make_criterion_and_optimizer(False, E.LossSettings(class_weights="balanced", focal_gamma=0.0))
    both = E.LossSettings(class_weights=(2.5, 0.625), focal_gamma=2.0)
    train, _ = E._make_criterion_and_optimizer(True, both)       # builds the host-side module only
    assert isinstance(train, HipCrossEntropyLoss) and train.weight.tolist() == [2.5, 0.625]
    assert (train.focal_gamma, train.label_smoothing) == (2.0, 0.1)
    for use_cuda in (True, False):
        ev = E._make_eval_criterion(use_cuda)
        assert ev.weight is None and getattr(ev, "focal_gamma", 0.0) == 0.0 and ev.label_smoothing == 0.1
    assert "class_weights=[2.5, 0.625]" in both.describe() and "focal_gamma=2" in both.describe()


def test_loss_module_arguments():
    from deepfakedetection_amd.optim import HipCrossEntropyLoss

    plain = HipCrossEntropyLoss(0.1)
    assert plain.weight is None and plain.focal_gamma == 0.0 and "weight" not in plain.state_dict()
    crit = HipCrossEntropyLoss(0.1, weight=torch.tensor([1.0, 3.0], dtype=torch.float64), focal_gamma=1.5)
    assert crit.weight.dtype == torch.float32 and dict(crit.named_buffers())["weight"] is crit.weight
    for bad in ([1.0, -1.0], [1.0, float("nan")], [1.0, float("inf")], [], [[1.0, 2.0]], "heavy"):
        with pytest.raises(ValueError):
            HipCrossEntropyLoss(0.1, weight=bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="focal_gamma"):
            HipCrossEntropyLoss(0.1, focal_gamma=bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        crit(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64))


# ------------------------------------------------------------------ the library
def test_abi_147_entry_point_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.dfd_version() >= 147
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    EINVAL = -1
    #        logits targets soft N  J  eps  gamma w  gs   denom rows loss dlogits stream
    good = [p, p, 0, 2, 2, 0.1, 2.0, p, 1.0, p, p, p, p, None]
    for at, value in ((0, None), (1, None), (9, None), (10, None), (11, None),           # null pointers
                      (3, 0), (3, -1), (4, 0), (4, -5),                                   # N < 1, J < 1
                      (6, -0.5), (6, float("nan")), (6, float("inf")),                    # gamma
                      (5, -0.1), (5, 1.0), (5, 1.5), (5, float("nan"))):                  # label smoothing outside [0, 1)
        args = list(good)
        args[at] = value
        for soft in (0, 1):
            args[2] = soft
            assert lib.dfd_ce_loss_w(*args) == EINVAL, (at, value, soft)


# ------------------------------------------------------------------ the sampler
TARGETS = [0] * 900 + [1] * 100
SEEDS = (0, 1, 2, 3, 2024)


def test_balanced_sampler_repeats_its_draw_per_seed_and_epoch():
    from deepfakedetection_amd.dp import BalancedShardedSampler

    a, b = BalancedShardedSampler(TARGETS, 0, 1, seed=5), BalancedShardedSampler(TARGETS, 0, 1, seed=5)
    assert len(a) == 1000 and list(a) == list(b) and list(a) == list(a)
    first = list(a)
    assert all(0 <= i < 1000 for i in first) and len(set(first)) < 1000          # with replacement
    a.set_epoch(1)
    assert list(a) != first
    b.set_epoch(1)
    assert list(a) == list(b)
    assert list(BalancedShardedSampler(TARGETS, 0, 1, seed=6)) == list(a)          # seed + epoch names the draw
    want = torch.multinomial(torch.tensor([1 / 1800] * 900 + [1 / 200] * 100, dtype=torch.float64), 1000, replacement=True,
                             generator=torch.Generator().manual_seed(6)).tolist()
    assert list(a) == want


def test_balanced_sampler_shards_interleave_to_the_common_draw():
    from deepfakedetection_amd.dp import BalancedShardedSampler

    shards = [BalancedShardedSampler(TARGETS, r, 3, seed=2) for r in range(3)]
    for s in shards:
        s.set_epoch(4)
    lists = [list(s) for s in shards]
    assert [len(s) for s in shards] == [334] * 3 and [len(x) for x in lists] == [334] * 3
    common = shards[0].draw()
    assert len(common) == 1002 and common == shards[2].draw()
    assert [lists[i % 3][i // 3] for i in range(1002)] == common
    single = BalancedShardedSampler(TARGETS, 0, 1, seed=2)
    single.set_epoch(4)
    assert common[:1000] == list(single) and common[1000:] == common[:2]          # padded like ShardedSampler(pad=True)


@pytest.mark.parametrize("seed", SEEDS)
def test_balanced_sampler_draws_the_classes_equally_often(seed):
    """1000 draws, each of class 1 with probability 0.5: the share lies within 4 binomial standard deviations, 4 * sqrt(0.25 / 1000)
    = 0.063, of 0.5 (the seeds were checked on the CPU; a uniform draw would give 0.1)."""
    from deepfakedetection_amd.dp import BalancedShardedSampler

    for epoch in (0, 1):
        s = BalancedShardedSampler(TARGETS, 0, 1, seed=seed)
        s.set_epoch(epoch)
        share = sum(TARGETS[i] for i in s) / 1000
        print(f"[balanced sampler] seed {seed} epoch {epoch}: share of class 1 {share:.3f}")
        assert abs(share - 0.5) <= 4 * math.sqrt(0.25 / 1000), share


def test_balanced_sampler_ignores_an_absent_class():
    from deepfakedetection_amd.dp import BalancedShardedSampler

    targets = [0] * 30 + [2] * 10                                # class 1 has no sample
    s = BalancedShardedSampler(targets, 0, 1, seed=0)
    assert bool(torch.isfinite(s.weights).all()) and abs(float(s.weights.sum()) - 1.0) < 1e-12
    assert set(s.weights.tolist()) == {1 / 60, 1 / 20}
    drawn = [targets[i] for i in s]
    assert len(drawn) == 40 and set(drawn) <= {0, 2}


def test_make_loader_uses_the_balanced_sampler_for_training_loaders_only(monkeypatch):
    from deepfakedetection_amd.dp import BalancedShardedSampler, ShardedSampler
    from deepfakedetection_amd.trainers._inputs import make_loader

    class DS(torch.utils.data.Dataset):
        targets = [0] * 6 + [1] * 2

        def __len__(self):
            return 8

        def __getitem__(self, i):
            return torch.zeros(1), self.targets[i]

    _clear(monkeypatch)
    assert not isinstance(make_loader(DS(), 4, 0, shuffle=True).sampler, BalancedShardedSampler)
    assert isinstance(make_loader(DS(), 4, 0, shuffle=True, world=2).sampler, ShardedSampler)
    monkeypatch.setenv("BALANCED_SAMPLING", "1")
    for world in (1, 2):
        train = make_loader(DS(), 4, 0, shuffle=True, rank=world - 1, world=world, seed=3)
        assert isinstance(train.sampler, BalancedShardedSampler) and (train.sampler.rank, train.sampler.seed) == (world - 1, 3)
        assert len(train.sampler) == 8 // world and len(train) == 2 // world
        assert not isinstance(make_loader(DS(), 4, 0, shuffle=False, world=world).sampler, BalancedShardedSampler)
    assert sum(len(y) for _, y in make_loader(DS(), 4, 0, shuffle=True)) == 8
    assert not isinstance(make_loader(DS(), 4, 0, shuffle=True, balanced=False).sampler, BalancedShardedSampler)
