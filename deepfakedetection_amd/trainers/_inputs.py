"""Input pipeline of the three trainers: augmentation-policy settings, the toggleable transform pipelines, the loaders and
the host-to-device batch iterator.  Counterpart of `get_loaders` in the reference's trainers/efficientnet.py:111-234 (and
its two siblings, whose different defaults arrive as `build_transforms` keyword arguments); trainers/_engine.py drives it.
"""

from __future__ import annotations

import os
from dataclasses import dataclass
from pathlib import Path

import torch
from torch.utils.data import DataLoader

from .. import data as D
from ..dp import BalancedShardedSampler, ShardedSampler
from ..orchestration.train_env import as_bool, env_float, env_int, env_str, load_transform_toggles, require_num_classes


def _rgb(image):
    return image if getattr(image, "mode", "RGB") == "RGB" else image.convert("RGB")


@dataclass(frozen=True)
class PolicySettings:
    rand_augment: tuple[int, int] | None        # (num_ops, magnitude bin)
    trivial_augment: bool

    def transform(self):
        return D.RandAugment(*self.rand_augment) if self.rand_augment is not None else D.TrivialAugmentWide()


def policy_settings() -> PolicySettings | None:
    """$RAND_AUGMENT_OPS (YAML training.rand_augment_ops; absent or 0: off), $RAND_AUGMENT_MAGNITUDE (default 9, bins 0..30),
    $TRIVIAL_AUGMENT (YAML training.trivial_augment).  ValueError for both policies at once, more than D.AA_MAX_OPS operations
    or a magnitude outside the bins."""
    num_ops = env_int("RAND_AUGMENT_OPS", 0)
    trivial = env_str("TRIVIAL_AUGMENT", "0").lower() in {"1", "true", "yes", "on"}
    if num_ops and trivial:
        raise ValueError("training.rand_augment_ops and training.trivial_augment exclude each other")
    if num_ops:
        return PolicySettings(D.check_rand_augment(num_ops, env_int("RAND_AUGMENT_MAGNITUDE", 9)), False)
    return PolicySettings(None, True) if trivial else None


def jpeg_settings() -> tuple[float, int, int] | None:
    """(p, quality_min, quality_max) of the JPEG-compression augmentation from $JPEG_P (YAML training.jpeg_p; absent or 0: off),
    $JPEG_QUALITY_MIN (default 60) and $JPEG_QUALITY_MAX (default 100).  ValueError for p outside 0..1 or a quality range outside
    1 <= min <= max <= 100."""
    p = env_float("JPEG_P", 0.0)
    if p == 0:
        return None
    return D.check_jpeg(p, env_int("JPEG_QUALITY_MIN", 60), env_int("JPEG_QUALITY_MAX", 100))


def blur_settings() -> tuple[float, float, float] | None:
    """(p, sigma_min, sigma_max) of the Gaussian-blur augmentation from $BLUR_P (YAML training.blur_p; absent or 0: off),
    $BLUR_SIGMA_MIN (default 0.0) and $BLUR_SIGMA_MAX (default 3.0).  ValueError for p outside 0..1 or a sigma range outside
    0 <= min <= max <= 16."""
    p = env_float("BLUR_P", 0.0)
    if p == 0:
        return None
    return D.check_blur(p, env_float("BLUR_SIGMA_MIN", 0.0), env_float("BLUR_SIGMA_MAX", 3.0))


_POLICY_FROM_ENV = object()


def build_transforms(img_size: int, gpu_tail: bool = False, *, rotation_default: bool | None = None,
                     erasing_default: bool | None = None, jitter=(0.2, 0.2, 0.2, 0.05), rotation_after_flip: bool = False,
                     gpu_resize: bool = False, policy: PolicySettings | None = _POLICY_FROM_ENV,
                     jpeg: tuple[float, int, int] | None = _POLICY_FROM_ENV,
                     blur: tuple[float, float, float] | None = _POLICY_FROM_ENV):
    """(train, val) pipelines from the toggle defaults of the reference + $TRANSFORMS.
    gpu_tail=True: the pipelines end in uint8 HWC tensors and (train, val, train_tail, val_tail) is
    returned, the tails being `D.GpuInputTail`s that do flip / to-float / normalise / erasing on the GPU.
    The keyword arguments carry what differs between the reference's three trainers (efficientnet.py:128-187 vs
    efficientformer_v2.py:105-165 / fastervit.py:119-180): rotation / erasing off by default, ColorJitter 0.1,
    rotation placed after the horizontal flip.
    gpu_resize (with gpu_tail): Resize / CenterCrop / RandomCrop / RandomResizedCrop move onto the device as well
    (D.PlanGeometry + csrc/dfd_resize.hip, bit-exact with PIL): always for the validation pipeline, and for the training
    pipeline too — RandomRotation and ColorJitter, which the reference's DEFAULT toggles at 224 pixels switch on
    (trainers/efficientnet.py:134-135), run on the device as well (csrc/dfd_augment.hip, byte-exact with Pillow) as long as
    one picture fits a CU's LDS (img_size <= 228); larger pictures with rotation / jitter keep those two in the PIL workers.
    policy (default: policy_settings(), i.e. $RAND_AUGMENT_OPS / $TRIVIAL_AUGMENT; None: off): D.RandAugment or
    D.TrivialAugmentWide directly after ColorJitter's slot in the training pipeline, never in the validation one.  It follows
    rotation / jitter: on the device with them (D.GpuInputTail(rand_augment= | trivial_augment=), which then also applies the
    flip, before ColorJitter as the PIL pipeline does), else in the PIL workers — and then the flip stays in the workers too,
    in front of it, because it does not commute with the policy's geometric operations.
    jpeg (default: jpeg_settings(), i.e. $JPEG_P / $JPEG_QUALITY_MIN / $JPEG_QUALITY_MAX; None: off): (p, quality_min, quality_max) of
    the JPEG-compression augmentation, the last operation on bytes of the training pipeline, never in the validation one:
    D.RandomJpeg directly in front of ToTensor without gpu_tail; with gpu_tail always on the device (D.GpuInputTail(jpeg=),
    csrc/dfd_jpeg.hip, byte-exact with Pillow) and never in the workers.
    blur (default: blur_settings(), i.e. $BLUR_P / $BLUR_SIGMA_MIN / $BLUR_SIGMA_MAX; None: off): (p, sigma_min, sigma_max) of the
    Gaussian-blur augmentation, directly behind the policy's slot and directly in front of RandomJpeg in the training pipeline,
    never in the validation one.  It counts like rotation, jitter and a policy: without gpu_tail D.RandomBlur runs in the workers;
    with gpu_tail it runs on the device (D.GpuInputTail(blur=), csrc/dfd_blur.hip, byte-exact with Pillow) whenever one picture
    fits the augment kernel's LDS, and else in the workers in front of ToUint8HWC."""
    if policy is _POLICY_FROM_ENV:
        policy = policy_settings()
    if jpeg is _POLICY_FROM_ENV:
        jpeg = jpeg_settings()
    if blur is _POLICY_FROM_ENV:
        blur = blur_settings()
    small = img_size <= 64
    toggles = load_transform_toggles(
        {
            "ensure_rgb": True, "train_resize": True, "train_random_crop": small, "train_center_crop": False,
            "train_random_resized_crop": not small, "train_random_horizontal_flip": True,
            "train_random_rotation": (not small) if rotation_default is None else rotation_default,
            "train_color_jitter": not small,
            "train_random_erasing": (not small) if erasing_default is None else erasing_default,
            "train_to_tensor": True, "train_normalize": True, "val_resize": True, "val_center_crop": True,
            "val_to_tensor": True, "val_normalize": True,
        },
        required=("train_to_tensor", "train_normalize", "val_to_tensor", "val_normalize"),
    )
    on = toggles.get
    normalize = D.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    enlarged = max(img_size + 32, int(img_size * 1.15))
    train: list = [D.Lambda(_rgb)] if on("ensure_rgb", True) else []
    if small:
        if on("train_resize", True):
            train.append(D.Resize(img_size + 4))
        if on("train_random_crop", True):
            train.append(D.RandomCrop(img_size))
        elif on("train_center_crop", False):
            train.append(D.CenterCrop(img_size))
    else:
        if on("train_random_resized_crop", True):
            train.append(D.RandomResizedCrop(img_size, scale=(0.9, 1.0)))
        else:
            if on("train_resize", True):
                train.append(D.Resize(enlarged))
            if on("train_center_crop", True):
                train.append(D.CenterCrop(img_size))
        if not rotation_after_flip and on("train_random_rotation", True):
            train.append(D.RandomRotation(10))
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    if rotation_after_flip and not gpu_tail:
        # efficientformer_v2.py:157-160 / fastervit.py:166-170: flip, then rotation (also for small images)
        if on("train_random_horizontal_flip", True):
            train.append(D.RandomHorizontalFlip())
        if on("train_random_rotation", False):
            train.append(D.RandomRotation(10))
    want_rot = on("train_random_rotation", False) and (rotation_after_flip or not small)
    want_jit = on("train_color_jitter", False)
    aug_fits = img_size * img_size * 3 <= D.AUGMENT_MAX_BYTES
    train_on_gpu = gpu_tail and gpu_resize and (aug_fits or not (want_rot or want_jit or policy is not None or blur is not None))
    if train_on_gpu:
        # the geometric head of the pipeline as a PLAN (same decisions, same RNG calls), pixels untouched
        train = [D.Lambda(_rgb)] if on("ensure_rgb", True) else []
        if small:
            mode = "random" if on("train_random_crop", True) else "center"
            train.append(D.PlanGeometry(mode, img_size, img_size + 4 if on("train_resize", True) else None))
        elif on("train_random_resized_crop", True):
            train.append(D.PlanGeometry("rrc", img_size, rrc=D.RandomResizedCrop(img_size, scale=(0.9, 1.0))))
        else:
            train.append(D.PlanGeometry("center", img_size, enlarged if on("train_resize", True) else None))
        train_tail = D.GpuInputTail(mean if on("train_normalize", True) else [0.0] * 3,
                                    std if on("train_normalize", True) else [1.0] * 3,
                                    flip_p=0.5 if on("train_random_horizontal_flip", True) else 0.0,
                                    erase_p=0.5 if on("train_random_erasing", False) else 0.0,
                                    rotate_degrees=10.0 if want_rot else 0.0, jitter=jitter if want_jit else None,
                                    rand_augment=policy.rand_augment if policy is not None else None,
                                    trivial_augment=policy is not None and policy.trivial_augment, jpeg=jpeg, blur=blur)
    elif gpu_tail:
        # flip commutes with the per-pixel colour jitter, so it can move behind it onto the device — unless a policy follows
        worker_flip = policy is not None and on("train_random_horizontal_flip", True)
        if worker_flip:
            train.append(D.RandomHorizontalFlip())
        if rotation_after_flip and on("train_random_rotation", False):
            train.append(D.RandomRotation(10))      # rotation by a random angle commutes in distribution with the flip
        if on("train_color_jitter", False):
            train.append(D.ColorJitter(*jitter))
        if policy is not None:
            train.append(policy.transform())
        if blur is not None and not aug_fits:
            train.append(D.RandomBlur(blur[0], (blur[1], blur[2])))
        train.append(D.ToUint8HWC())
        train_tail = D.GpuInputTail(mean if on("train_normalize", True) else [0.0] * 3,
                                    std if on("train_normalize", True) else [1.0] * 3,
                                    flip_p=0.5 if on("train_random_horizontal_flip", True) and not worker_flip else 0.0,
                                    erase_p=0.5 if on("train_random_erasing", False) else 0.0, jpeg=jpeg,
                                    blur=blur if aug_fits else None)
    else:
        if not rotation_after_flip and on("train_random_horizontal_flip", True):
            train.append(D.RandomHorizontalFlip())
        if on("train_color_jitter", False):
            train.append(D.ColorJitter(*jitter))
        if policy is not None:
            train.append(policy.transform())
        if blur is not None:
            train.append(D.RandomBlur(blur[0], (blur[1], blur[2])))
        if jpeg is not None:
            train.append(D.RandomJpeg(jpeg[0], (jpeg[1], jpeg[2])))
        if on("train_to_tensor", True):
            train.append(D.ToTensor())
        if on("train_normalize", True):
            train.append(normalize)
        if on("train_random_erasing", False):
            train.append(D.RandomErasing(p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=0))

    val: list = [D.Lambda(_rgb)] if on("ensure_rgb", True) else []
    if gpu_tail and gpu_resize and on("val_center_crop", True):
        val.append(D.PlanGeometry("center", img_size, (img_size if small else enlarged) if on("val_resize", True) else None))
        val_tail = D.GpuInputTail(mean if on("val_normalize", True) else [0.0] * 3, std if on("val_normalize", True) else [1.0] * 3)
        return D.Compose(train), D.Compose(val), train_tail, val_tail
    if on("val_resize", True):
        val.append(D.Resize(img_size if small else enlarged))
    if on("val_center_crop", True):
        val.append(D.CenterCrop(img_size))
    if gpu_tail:
        val.append(D.ToUint8HWC())
        val_tail = D.GpuInputTail(mean if on("val_normalize", True) else [0.0] * 3, std if on("val_normalize", True) else [1.0] * 3)
        return D.Compose(train), D.Compose(val), train_tail, val_tail
    if on("val_to_tensor", True):
        val.append(D.ToTensor())
    if on("val_normalize", True):
        val.append(normalize)
    return D.Compose(train), D.Compose(val)


def balanced_sampling() -> bool:
    """$BALANCED_SAMPLING (YAML training.balanced_sampling, default off): the training loaders draw class-balanced epochs."""
    return as_bool(env_str("BALANCED_SAMPLING", "0"))


def make_loader(dataset, batch_size: int, num_workers: int, *, shuffle: bool, rank: int = 0, world: int = 1,
                seed: int = 0, balanced: bool | None = None) -> DataLoader:
    """`balanced` (default: balanced_sampling()) gives a training loader (shuffle=True) dp.BalancedShardedSampler over the
    dataset's `targets`, at any `world`; a validation loader (shuffle=False) never gets it."""
    extra = {"prefetch_factor": 2} if num_workers > 0 else {}
    if shuffle and (balanced_sampling() if balanced is None else balanced):
        sampler = BalancedShardedSampler(dataset.targets, rank, world, seed=seed)
    else:
        # training shards are padded to equal length (equal step counts for the all-reduce); validation shards are not
        sampler = ShardedSampler(len(dataset), rank, world, shuffle=shuffle, seed=seed, pad=shuffle) if world > 1 else None
    # pipelines that end in D.PlanGeometry ship variable-size decoded images: packed by D.collate_raw
    tf = getattr(dataset, "transform", None)
    if tf is not None and any(isinstance(op, D.PlanGeometry) for op in getattr(tf, "ops", ())):
        extra["collate_fn"] = D.collate_raw
    return DataLoader(dataset, batch_size=batch_size, shuffle=shuffle and sampler is None, sampler=sampler,
                      num_workers=num_workers, pin_memory=True, persistent_workers=num_workers > 0, **extra)


def get_loaders(data_root: Path, train_split: str, val_split: str, img_size: int, batch_size: int, num_workers: int, *,
                expected_classes: int | None = None, rank: int = 0, world: int = 1, seed: int = 0, gpu_tail: bool = False,
                transform_kwargs: dict | None = None, gpu_resize: bool | None = None):
    """(train loader, val loader); with gpu_tail also (train tail, val tail) to apply to each uint8 batch.
    gpu_resize (default $GPU_RESIZE, YAML training.gpu_resize): resize / crop on the device too (implies the GPU tail)."""
    tails = ()
    tk = transform_kwargs or {}
    if gpu_resize is None:
        gpu_resize = env_str("GPU_RESIZE", "0").lower() in {"1", "true", "yes"}
    if gpu_tail:
        train_t, val_t, *tails = build_transforms(img_size, gpu_tail=True, gpu_resize=gpu_resize, **tk)
    else:
        train_t, val_t = build_transforms(img_size, **tk)
    train_ds = D.ImageFolder(data_root / train_split, transform=train_t)
    if expected_classes is not None:
        require_num_classes(train_ds, expected_classes, split=train_split)
    val_ds = D.ImageFolder(data_root / val_split, transform=val_t)
    return (make_loader(train_ds, batch_size, num_workers, shuffle=True, rank=rank, world=world, seed=seed),
            make_loader(val_ds, batch_size, num_workers, shuffle=False, rank=rank, world=world, seed=seed), *tails)


def _to_device(batch_x: torch.Tensor, device: str, tail) -> torch.Tensor:
    if tail is not None:
        return tail(batch_x, device)                         # uint8 NHWC -> normalised f32 on the GPU
    return batch_x.to(device, non_blocking=True).to(memory_format=torch.channels_last)


def device_batches(dl, device: str, tail, prefetch: bool = False):
    """(inputs, targets) on the device for every batch of `dl`, with the host-to-device copy of batch i+1 issued on a copy
    stream BEFORE the caller enqueues the work of batch i (the reference's loop, trainers/efficientnet.py:283-287, copies
    in-stream: at batch 256 that is 154 MB, ~3 ms of PCIe time the kernels wait for).  Asked for by the hipGraph-replayed
    loop only (`prefetch`): measured on MI355X, B0, 256 x 1: 14.6 k -> 17.1 k images/s, 32 x 4: 5.8 k -> 6.1 k; the eager
    loop is host-bound and loses 2..10 % to the extra stream bookkeeping.  The GPU input tail (`tail`: uint8 batches +
    dfd_image_prep) and CPU runs keep the in-stream path.  PREFETCH_H2D=0 switches the copy stream off."""
    use = prefetch and tail is None and str(device).startswith("cuda") and os.environ.get("PREFETCH_H2D", "1") != "0"
    if not use:
        for batch_x, batch_y in dl:
            yield _to_device(batch_x, device, tail), batch_y.to(device, non_blocking=True)
        return
    copy = torch.cuda.Stream(device=device)

    def stage(batch):
        with torch.cuda.stream(copy):
            x = batch[0].to(device, non_blocking=True)
            y = batch[1].to(device, non_blocking=True)
            done = torch.cuda.Event()
            done.record(copy)
        return x, y, done

    it = iter(dl)
    try:
        nxt = stage(next(it))
    except StopIteration:
        return
    while nxt is not None:
        x, y, done = nxt
        cur = torch.cuda.current_stream()
        cur.wait_event(done)
        x.record_stream(cur)                    # allocated on the copy stream, consumed on this one
        y.record_stream(cur)
        try:
            nxt = stage(next(it))               # requested before the caller enqueues this batch's kernels
        except StopIteration:
            nxt = None
        yield x.to(memory_format=torch.channels_last), y
