"""EfficientNet trainer on the MI355X engine — counterpart of the reference's trainers/efficientnet.py.

Same `main()` contract (no arguments, configuration through the environment), same phases and file outputs:
head-only warm-up epoch (names containing "_fc" or "classifier", :433-437), then everything trainable with micro-batches
of $FT_BATCH_SIZE (default 32, the reference's constant) and $ACCUM_STEPS (default 128 // 32) accumulation steps, cosine
LR, early stop on EARLY_STOP_PATIENCE, evaluation with accuracy and mean CE loss (:237-262), the mean training loss per
epoch (:265-333), `EfficientNetModel.pth` / latest.ckpt / best.ckpt.  The reference hard-codes
`EfficientNet.from_pretrained("efficientnet-b3")`; this trainer builds `get_model_spec($MODEL_NAME).builder`.
The loops live in trainers/_engine.py, the input pipeline in trainers/_inputs.py; `SPEC` below is what this script does
differently from the other two.  The names the reference's module exposes, and those that tests and scripts use from
here, are re-exported.
"""

from __future__ import annotations

from ._engine import (  # noqa: F401  (re-exported)
    ACC, ACC_COUNTS, DATA_ROOT, LOG_EVERY, EvalResult, TrainerSpec, clip_settings, ema_settings, eval_forward, evaluate, make_mixer, make_stepper,
    mix_settings, run, train_one_epoch,
)
from ._inputs import PolicySettings, blur_settings, build_transforms, device_batches, get_loaders, jpeg_settings, make_loader, policy_settings  # noqa: F401

DEFAULT_MODEL = "efficientnet_b3"
DEFAULT_EPOCHS, DEFAULT_BATCH_SIZE, DEFAULT_IMG_SIZE, DEFAULT_NUM_WORKERS = 25, 64, 224, 8
HEAD_LR, HEAD_WD, FT_LR, FT_WD = 3e-4, 5e-2, 1e-4, 5e-2
DEFAULT_PATIENCE = 4
BEST_WEIGHTS_NAME, BEST_CKPT_NAME, LATEST_CKPT_NAME = "EfficientNetModel.pth", "best.ckpt", "latest.ckpt"
FT_BATCH_SIZE, EFFECTIVE_BATCH = 32, 128
DEFAULT_ACCUM_STEPS = max(1, EFFECTIVE_BATCH // FT_BATCH_SIZE)
HEAD_KEYS = ("_fc", "classifier")       # parameter-name substrings of the classification head

SPEC = TrainerSpec(
    model_name=DEFAULT_MODEL, best_weights_name=BEST_WEIGHTS_NAME, default_epochs=DEFAULT_EPOCHS,
    default_batch_size=DEFAULT_BATCH_SIZE, warmup_keys=HEAD_KEYS, unfreeze_keys=None, ft_batch_size=FT_BATCH_SIZE,
    ft_accum_steps=DEFAULT_ACCUM_STEPS, ft_from_env=True, zero_grad_first=False, warmup_zero_grad_first=False, report_loss=True,
    early_stop=True, default_patience=DEFAULT_PATIENCE, default_img_size=DEFAULT_IMG_SIZE, default_num_workers=DEFAULT_NUM_WORKERS,
    head_lr=HEAD_LR, head_wd=HEAD_WD, ft_lr=FT_LR, ft_wd=FT_WD, pass_img_size=False, transform_kwargs=None,
    warmup_task="warmup (head only)", warmup_label=None,
    warmup_line=ACC + " | val_loss={res.loss:.4f} ({res.correct}/{res.total})",
    epoch_line="train_loss={train_loss:.4f} | val_loss={res.loss:.4f} | " + ACC_COUNTS + " | lr={lr:.2e}",
    ema_line="val_loss={res.loss:.4f} | " + ACC_COUNTS,
)


def main() -> None:
    run(SPEC)


if __name__ == "__main__":
    main()
