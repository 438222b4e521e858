"""Gradient clipping on the MI355X: dfd_grad_sumsq / dfd_grad_clip_finish against the exactly rounded norm, the coefficient
against the f32 formula, HipAdamW(max_grad_norm=...) against a plain HipAdamW over pre-scaled (or clamped) gradients bit for
bit, the skipped step of a non-finite gradient, the clip inside the replayed optimizer-step graph, the orchestrated run with
`training.clip_grad`, and data parallel."""

from __future__ import annotations

import copy
import datetime
import json
import os
import socket
import traceback
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml

from deepfakedetection_amd import kernels as K
from deepfakedetection_amd._lib import (
    ADAMW_HP_LEN, CLIP_CLIPPED, CLIP_COEF, CLIP_MODE_NORM, CLIP_MODE_VALUE, CLIP_NORM, CLIP_NORM_MAX, CLIP_NORM_SUM, CLIP_SKIP,
    CLIP_SKIPPED, CLIP_STATE_LEN, CLIP_STEPS,
)
from tests import _clip_ref as ref
from tests.test_plumbing_cpu import _make_dataset

pytestmark = pytest.mark.gpu

_F32 = np.float32
_CHUNK = 4096
_FIELDS = ("grad_norm_mean", "grad_norm_max", "clipped_steps", "skipped_steps")


def _bits(a) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8)


def _rows(g: torch.Tensor, shift: int, n: int) -> list[list[int]]:
    """AdamW table rows {param, grad, exp_avg, exp_avg_sq, count} over g[shift : shift + n]; only grad and count are read."""
    return [[0, g.data_ptr() + 4 * (shift + off), 0, 0, min(_CHUNK, n - off)] for off in range(0, n, _CHUNK)]


def _hp(grad_scale: float = 1.0) -> torch.Tensor:
    vals = [1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, grad_scale]
    assert len(vals) == ADAMW_HP_LEN
    return torch.tensor(vals, dtype=torch.float32, device="cuda")


def _cfg(limit: float, mode: int = CLIP_MODE_NORM) -> torch.Tensor:
    return torch.tensor([limit, float(mode)], dtype=torch.float32, device="cuda")


def _norm_data():
    """Host gradients of the issue's sizes: scaled by 1e-3 / 1 / 1e3 per tensor, plus one tensor of 1e-4 values with a single
    1e4 outlier."""
    rng = np.random.default_rng(11)
    sizes = (1, 3, 4095, 4096, 4097, 1_000_003)
    hosts = [(rng.standard_normal(n) * s).astype(_F32) for n, s in zip(sizes, (1.0, 1e-3, 1e3, 1.0, 1e-3, 1.0))]
    outlier = np.full(4097, 1e-4, dtype=_F32)
    outlier[1234] = 1e4
    return hosts + [outlier]


def test_norm_kernels_give_the_exactly_rounded_norm_at_any_alignment_and_in_every_run():
    """state[0] = float32(sqrt(fsum(g^2))) within one f32 ulp: the products are exact in f64 and the f64 sum over <= 2.1e6
    terms is off by at most n * 2^-53 ~ 2e-10 relative, far below the f32 half-ulp, so the one rounding to f32 is the only
    slack.  Every tensor is in the table twice, 16-byte aligned (float4 path) and one float off (scalar path)."""
    hosts = _norm_data()
    dev = torch.device("cuda")
    keep, rows_a, rows_m = [], [], []
    for h in hosts:
        aligned = torch.from_numpy(h).to(dev)
        shifted = torch.from_numpy(np.concatenate([np.zeros(1, _F32), h])).to(dev)
        assert aligned.data_ptr() % 16 == 0 and (shifted.data_ptr() + 4) % 16 == 4
        keep += [aligned, shifted]
        rows_a += _rows(aligned, 0, h.size)
        rows_m += _rows(shifted, 1, h.size)
    table = torch.tensor(rows_a + rows_m, dtype=torch.int64, device=dev)
    n = len(rows_a)
    hp, cfg = _hp(), _cfg(1.0)
    runs = []
    for _ in range(2):
        partials = torch.full((2 * n,), -1.0, dtype=torch.float64, device=dev)
        state = torch.zeros(CLIP_STATE_LEN, dtype=torch.float32, device=dev)
        K.grad_sumsq(table, partials)
        K.grad_clip_finish(partials, hp, cfg, state)
        torch.cuda.synchronize()
        runs.append((partials.cpu().numpy(), state.cpu().numpy()))
    partials, state = runs[0]
    assert np.array_equal(_bits(partials[:n]), _bits(partials[n:])), "aligned and misaligned chunks differ"
    assert np.array_equal(_bits(runs[1][0]), _bits(partials)) and np.array_equal(_bits(runs[1][1]), _bits(state))
    want = ref.total_norm(hosts + hosts)
    print(f"norm: kernel {state[CLIP_NORM]!r}, exact {want!r}")
    assert ref.within_one_ulp(state[CLIP_NORM], want), (state[CLIP_NORM], want)
    # every chunk's partial against its own exact sum: <= 4096 f64 additions, 4096 * 2^-53 relative
    off = 0
    for h in hosts:
        for o in range(0, h.size, _CHUNK):
            exact = ref.exact_sumsq([h[o:o + _CHUNK]])
            got = partials[off]
            assert abs(got - exact) <= exact * _CHUNK * 2.0 ** -53, (h.size, o, got, exact)
            off += 1
    assert off == n
    assert state[CLIP_STEPS] == 1 and state[CLIP_SKIP] == 0 and state[CLIP_SKIPPED] == 0
    assert state[CLIP_NORM_SUM] == state[CLIP_NORM] == state[CLIP_NORM_MAX]


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_coefficient_is_the_f32_formula_and_the_record_accumulates(grad_scale):
    rng = np.random.default_rng(5)
    h = rng.standard_normal(10_001).astype(_F32)
    g = torch.from_numpy(h).cuda()
    table = torch.tensor(_rows(g, 0, h.size), dtype=torch.int64, device="cuda")
    partials = torch.zeros(table.shape[0], dtype=torch.float64, device="cuda")
    state = torch.zeros(CLIP_STATE_LEN, dtype=torch.float32, device="cuda")
    hp = _hp(grad_scale)
    norm = ref.total_norm([h], grad_scale)
    seen = []
    for limit, mode in ((0.25 * float(norm), CLIP_MODE_NORM), (4.0 * float(norm), CLIP_MODE_NORM), (1e-3, CLIP_MODE_VALUE)):
        K.grad_sumsq(table, partials)
        K.grad_clip_finish(partials, hp, _cfg(limit, mode), state)
        torch.cuda.synchronize()
        s = state.cpu().numpy()
        assert ref.within_one_ulp(s[CLIP_NORM], norm)
        want = _F32(1.0) if mode == CLIP_MODE_VALUE else ref.coef(s[CLIP_NORM], limit)
        assert np.array_equal(_bits(s[CLIP_COEF]), _bits(want)), (limit, mode, s[CLIP_COEF], want)
        seen.append(s)
    assert seen[0][CLIP_COEF] < 1.0 and seen[1][CLIP_COEF] == 1.0
    last = seen[-1]
    assert (last[CLIP_STEPS], last[CLIP_CLIPPED], last[CLIP_SKIPPED], last[CLIP_SKIP]) == (3, 1, 0, 0)
    n0 = seen[0][CLIP_NORM]
    assert last[CLIP_NORM_MAX] == n0 and last[CLIP_NORM_SUM] == _F32(_F32(n0 + n0) + n0)


_SIZES = (1, 7, 4096, 4097, 50_001)


def _params(seed: int):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in _SIZES]


def _state_bits(opt) -> list[np.ndarray]:
    out = []
    for group in opt.param_groups:
        for p in group["params"]:
            out += [_bits(p), _bits(opt.state[p]["exp_avg"]), _bits(opt.state[p]["exp_avg_sq"])]
    return out


def _same(a: list[np.ndarray], b: list[np.ndarray]) -> bool:
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _groups(params, two: bool):
    if not two:
        return params
    return [{"params": params[:2], "lr": 1e-3}, {"params": params[2:], "lr": 3e-3, "weight_decay": 0.0}]


@pytest.mark.parametrize("mode,limit,two_groups", [("norm", 1.0, False), ("norm", 1e9, False), ("value", 0.5, False),
                                                    ("norm", 1.0, True), ("value", 0.5, True)])
def test_clipped_step_equals_plain_step_over_prescaled_gradients_bitwise(mode, limit, two_groups):
    """grad_scale = 1: (g * 1) * coef is one f32 rounding, the same as scaling the gradient before a plain step; the value mode's
    fminf(fmaxf(g, -v), v) is g.clamp(-v, v).  The norm is global over both param groups."""
    from deepfakedetection_amd.optim import HipAdamW

    pa, pb = _params(3), _params(3)
    kw = dict(lr=1e-3, weight_decay=5e-2, use_arena=False)
    clip = HipAdamW(_groups(pa, two_groups), max_grad_norm=limit, clip_mode=mode, **kw)
    plain = HipAdamW(_groups(pb, two_groups), **kw)
    gen = torch.Generator().manual_seed(4)
    for step in range(3):
        grads = [torch.randn(n, generator=gen) * (10.0 if i == 4 else 1.0) for i, n in enumerate(_SIZES)]
        for p, g in zip(pa, grads):
            p.grad = g.cuda()
        clip.step()
        state = clip.clip_state.cpu().numpy()
        norm = ref.total_norm([g.numpy() for g in grads])
        assert ref.within_one_ulp(state[CLIP_NORM], norm), (state[CLIP_NORM], norm)       # one norm over every group
        coef = state[CLIP_COEF]
        if mode == "value":
            assert coef == 1.0
            prepared = [g.cuda().clamp(-limit, limit) for g in grads]
            assert any(not torch.equal(q.cpu(), g) for q, g in zip(prepared, grads))
        else:
            assert np.array_equal(_bits(coef), _bits(ref.coef(state[CLIP_NORM], limit)))
            assert (coef < 1.0) == (limit < 1e9)
            prepared = [g.cuda() * torch.tensor(coef, device="cuda") for g in grads]     # unchanged bits when coef == 1
        for p, g in zip(pb, prepared):
            p.grad = g
        plain.step()
        torch.cuda.synchronize()
        assert _same(_state_bits(clip), _state_bits(plain)), (mode, limit, step)
    stats = clip.clip_stats()
    assert stats["steps"] == 3 and stats["skipped_steps"] == 0
    assert stats["clipped_steps"] == (3 if mode == "norm" and limit < 1e9 else 0)
    assert stats["grad_norm_max"] >= stats["grad_norm_mean"] > 0 and clip.clip_stats()["steps"] == 0       # reset


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("mode", ["norm", "value"])
def test_non_finite_gradient_skips_the_step_and_the_next_one_proceeds(bad, mode):
    from deepfakedetection_amd.optim import HipAdamW

    pa = _params(6)
    clip = HipAdamW(pa, lr=1e-3, weight_decay=5e-2, use_arena=False, max_grad_norm=1.0, clip_mode=mode)
    gen = torch.Generator().manual_seed(7)

    def grads():
        return [torch.randn(n, generator=gen) for n in _SIZES]

    for p, g in zip(pa, grads()):
        p.grad = g.cuda()
    clip.step()                                             # a clean step first: non-trivial moments
    torch.cuda.synchronize()
    before = _state_bits(clip)
    poisoned = grads()
    poisoned[3][4096] = bad                                 # the lone element of the second chunk of the 4097 tensor
    for p, g in zip(pa, poisoned):
        p.grad = g.cuda()
    clip.step()
    torch.cuda.synchronize()
    assert _same(_state_bits(clip), before), "a skipped step changed a parameter or a moment"
    state = clip.clip_state.cpu().numpy()
    assert state[CLIP_SKIP] == 1 and not np.isfinite(state[CLIP_NORM])
    stats = clip.clip_stats(reset=False)
    assert (stats["steps"], stats["skipped_steps"]) == (2, 1) and np.isfinite(stats["grad_norm_mean"])
    # the next clean step: a plain optimizer that takes over parameters, moments and the (advanced) step counter does the same
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    plain = HipAdamW(pb, lr=1e-3, weight_decay=5e-2, use_arena=False)
    sd = copy.deepcopy(clip.state_dict())
    plain.load_state_dict(sd)
    clean = grads()
    for p, g in zip(pa, clean):
        p.grad = g.cuda()
    clip.step()
    state = clip.clip_state.cpu().numpy()
    assert state[CLIP_SKIP] == 0 and np.isfinite(state[CLIP_NORM])
    for p, g in zip(pb, clean):
        p.grad = g.cuda().clamp(-1.0, 1.0) if mode == "value" else g.cuda() * torch.tensor(state[CLIP_COEF], device="cuda")
    plain.step()
    torch.cuda.synchronize()
    assert _same(_state_bits(clip), _state_bits(plain))
    assert not _same(_state_bits(clip), before)
    assert float(clip.state[pa[0]]["step"]) == 3.0          # the host-side counter advanced on the skipped step too
    assert clip.clip_stats()["skipped_steps"] == 1


def _b0(seed: int):
    from deepfakedetection_amd.efficientnet import HipEfficientNet

    torch.manual_seed(seed)
    return HipEfficientNet("b0", "timm", 2).cuda()


def _batches(n: int, bs: int = 32, size: int = 64, seed: int = 3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(bs, 3, size, size, generator=g).cuda(), torch.randint(0, 2, (bs,), generator=g).cuda()) for _ in range(n)]


def _cycles(graph: bool, limit, *, change_to=None, with_ema: bool = False, accum: int = 2, cycles: int = 5):
    from deepfakedetection_amd.ema import ModelEma
    from deepfakedetection_amd.graph_step import GraphedTrainStep
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss

    batches = _batches(accum * cycles)
    model = _b0(11).train()
    ema = ModelEma(model, _b0(12), decay=0.9999, warmup=True) if with_ema else None
    opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=5e-2, max_grad_norm=limit)
    step = GraphedTrainStep(model, HipCrossEntropyLoss(0.1), opt, accum_steps=accum, ema=ema)
    if not graph:
        step.failed = True
    coefs = []
    for i, (x, y) in enumerate(batches):
        step.micro_batch(x, y, first=i % accum == 0, last=(i + 1) % accum == 0)
        if (i + 1) % accum == 0:
            if change_to is not None and (i + 1) // accum == 4:
                opt.set_clip(change_to)                      # from the fourth cycle on: a replay, not a capture
            step.optimizer_step()
            if limit is not None:
                coefs.append(opt.clip_state.cpu().numpy()[[CLIP_NORM, CLIP_COEF]])
    torch.cuda.synchronize()
    return model, ema, step, opt, coefs


def _equal_state(a, b) -> None:
    for (name, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("case", ["fixed", "changed", "ema"])
def test_graph_replay_with_clipping_equals_eager(case):
    """The three clip launches are captured with AdamW (and the EMA update); `cfg` is read from device memory, so a limit changed
    between replays reaches the captured launches."""
    kw = {"fixed": {}, "changed": {"change_to": 0.01}, "ema": {"with_ema": True}}[case]
    m_e, ema_e, _, opt_e, coefs_e = _cycles(False, 0.05, **kw)
    m_g, ema_g, step, opt_g, coefs_g = _cycles(True, 0.05, **kw)
    assert not step.failed and step.step_graph is not None and step.replays == 4 * 2, step.replays
    _equal_state(m_e, m_g)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(coefs_e, coefs_g)) and len(coefs_g) == 5
    for k, (norm, coef) in enumerate(coefs_g):
        limit = 0.01 if case == "changed" and k >= 3 else 0.05
        assert np.array_equal(_bits(coef), _bits(ref.coef(norm, limit))), (k, norm, coef)
    print("norm, coef per cycle:", [(float(n), float(c)) for n, c in coefs_g])
    se, sg = opt_e.clip_stats(), opt_g.clip_stats()
    assert se == sg and sg["steps"] == 5 and sg["clipped_steps"] >= 1 and sg["skipped_steps"] == 0      # the clip is active
    if case == "ema":
        assert ema_e.updates == ema_g.updates == 5
        _equal_state(ema_e.module, ema_g.module)


def test_graph_replay_with_a_huge_limit_equals_no_clipping():
    m_off, _, step_off, opt_off, _ = _cycles(True, None)
    m_on, _, step_on, opt_on, coefs = _cycles(True, 1e9)
    assert step_off.step_graph is not None and step_on.step_graph is not None and not step_off.failed and not step_on.failed
    assert opt_off.clip_stats() is None and all(c[1] == 1.0 for c in coefs)
    _equal_state(m_off, m_on)
    assert opt_on.clip_stats()["clipped_steps"] == 0


def test_failed_capture_falls_back_to_the_eager_clipped_step(monkeypatch):
    """GraphedTrainStep's give-up path: the optimizer-step capture raises on the host (before anything is launched), the step
    warns, and every cycle still takes the clipped step eagerly."""
    real = K.grad_sumsq

    def refuse_capture(table, partials):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("no capture today")
        real(table, partials)

    monkeypatch.setattr(K, "grad_sumsq", refuse_capture)
    with pytest.warns(UserWarning, match="running eagerly"):
        model, _, step, opt, coefs = _cycles(True, 0.05)
    assert step.failed and step.step_graph is None
    assert len(coefs) == 5 and all(np.array_equal(_bits(c), _bits(ref.coef(n, 0.05))) for n, c in coefs)
    stats = opt.clip_stats()
    assert (stats["steps"], stats["clipped_steps"], stats["skipped_steps"]) == (5, 5, 0)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


@pytest.mark.parametrize("model_name,img", [("efficientnet_b0", 64), ("efficientformerv2_s0", 64)])
def test_orchestrated_training_with_clip_grad(tmp_path, monkeypatch, model_name, img):
    from deepfakedetection_amd.orchestration.orchestrator import orchestrate

    monkeypatch.chdir(tmp_path)
    _make_dataset(tmp_path / "data", classes=("fake", "real"), per_class=8, size=img + 8)
    base = {"seed": 1, "device": "cuda",
            "data": {"root": str(tmp_path / "data"), "train_split": "train", "val_split": "val", "test_split": "test",
                     "num_classes": 2, "img_size": img}}
    training = {"epochs": 1, "batch_size": 8, "ft_batch_size": 8, "accum_steps": 2, "num_workers": 0, "pretrained": False,
                "img_size": img}

    def run(tag: str, extra: dict):
        out_dir = str(tmp_path / "runs" / tag)
        path = tmp_path / f"{tag}.yaml"
        path.write_text(yaml.safe_dump({**base, "models": {model_name: {"output_dir": out_dir, "training": {**training, **extra}}}}))
        orchestrate(path, mode="training")
        d = sorted(Path(out_dir).iterdir())[0]
        rows = [json.loads(line) for line in (d / "logs" / "throughput.jsonl").read_text().splitlines()]
        return rows, " ".join((d / "logs" / "train.log").read_text().split())

    rows, log = run("clip", {"clip_grad": 0.5})
    assert [r["phase"] for r in rows] == ["warmup", "fine-tune"]
    for r in rows:                                           # the warm-up optimizer clips too
        assert all(f in r for f in _FIELDS), r
        assert r["skipped_steps"] == 0 and r["grad_norm_max"] >= r["grad_norm_mean"] > 0 and r["clipped_steps"] >= 0
    assert log.count("grad_norm=") == 2 and "(clipped " in log
    rows, log = run("plain", {})
    assert [r["phase"] for r in rows] == ["warmup", "fine-tune"]
    assert not any(f in r for r in rows for f in _FIELDS) and "grad_norm" not in log


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank: int, world: int, port: int) -> None:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0", GRAPH_STEP="1")
    from deepfakedetection_amd.dp import GradAllReducer, broadcast_module_state
    from deepfakedetection_amd.efficientnet import HipEfficientNet
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss
    from deepfakedetection_amd.trainers.efficientnet import make_stepper

    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    try:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        torch.manual_seed(10 + rank)                                 # different init: broadcast must fix it
        model = HipEfficientNet("b0", "timm", 2).to(dev).train()
        broadcast_module_state(model)
        opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=1e-2, grad_scale=1.0 / world, max_grad_norm=0.05)
        red = GradAllReducer(model.parameters(), bucket_bytes=2 << 20, arena=opt.arena)
        red.attach()
        step = make_stepper(model, HipCrossEntropyLoss(0.1), opt, accum_steps=1, use_cuda=True, world=world, reducer=red)
        assert step is not None
        g = torch.Generator().manual_seed(70 + rank)                 # each rank its own shard
        for _ in range(3):
            x = torch.randn(8, 3, 64, 64, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
            y = torch.randint(0, 2, (8,), generator=g).to(dev)
            step.micro_batch(x, y, first=True, last=True)
            step.optimizer_step()
        torch.cuda.synchronize()
        red.detach()
        assert step.step_graph is not None and not step.failed
        # the clip ran after the all-reduce: the arena holds the SUM over ranks, grad_scale = 1 / world makes it the mean's norm
        state = opt.clip_state.cpu().numpy()
        want = ref.total_norm([opt.arena.flat.cpu().numpy()], 0.5)
        assert ref.within_one_ulp(state[CLIP_NORM], want), (state[CLIP_NORM], want)
        assert state[CLIP_SKIP] == 0 and state[CLIP_STEPS] == 3
        flat = torch.cat([p.detach().flatten() for p in model.parameters()] + [opt.clip_state[:1]])
        parts = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(parts, flat)
        assert torch.equal(parts[0][:-1], parts[1][:-1]), "parameters differ across ranks"
        assert np.array_equal(_bits(parts[0][-1:]), _bits(parts[1][-1:])), "the ranks computed different norms"
    except BaseException:
        traceback.print_exc()
        os._exit(1)
    dist.destroy_process_group()


def test_two_ranks_clip_by_the_same_norm():
    mp.spawn(_dp_worker, args=(2, _free_port()), nprocs=2, join=True)
