"""Completeness of the capture journal: every device address libdfd_hip.so receives during a training step, as a direct
argument or inside a job array or a chunk table, belongs to a tensor the journal recorded (kernels.capture_journal).  The
replay guard of a captured step (graph_step) is built from that journal, so an address it misses is memory a replay could
touch after it was freed."""

from __future__ import annotations

import bisect
import ctypes

import pytest
import torch

from deepfakedetection_amd import _lib, kernels as K
from tests.test_train_gpu import _build

pytestmark = pytest.mark.gpu

# entry points whose first argument is an int64 chunk table in device memory -> how many leading columns are addresses
_TABLE_COLS = {"dfd_adamw_step": 4, "dfd_adamw_step_clip": 4, "dfd_grad_sumsq": 4, "dfd_ema_update": 2}
_MUST_RUN = ("dfd_bgemm", "dfd_attn_softmax_bwd", "dfd_coord_mlp_fwd_multi", "dfd_coord_mlp_bwd_multi", "dfd_prep_weights_multi",
             "dfd_bn_eval_coeffs_multi", "dfd_adamw_step", "dfd_ema_update")


def _spans(spans) -> list:
    """The union of [lo, hi) address ranges as sorted disjoint intervals."""
    out: list = []
    for lo, hi in sorted(spans):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        elif hi > lo:
            out.append([lo, hi])
    return out


def _inside(addr: int, spans: list) -> bool:
    i = bisect.bisect_right(spans, [addr, float("inf")]) - 1
    return i >= 0 and spans[i][0] <= addr < spans[i][1]


class _Recorder:
    """A proxy over the loaded library: forwards every call and records (entry point, address) for each argument
    _lib.SIGNATURES types as a pointer: the integer itself, or every c_void_p field of every element of a job array; for
    the chunk-table entry points also the address columns of the table, copied back at the call.

    `late` gets the addresses that belong to no tensor journalled SINCE THE PREVIOUS LIBRARY CALL.  Over a whole step the
    journal's ranges cover most of the allocator's memory (temporaries come and go), so "inside some entry" alone says
    little about an activation; the front ends note what they pass while they build the call, and that is sharp."""

    def __init__(self, lib, notes: dict) -> None:
        self._lib, self._notes, self._recent = lib, notes, []
        self.seen, self.late, self.tables = [], [], []

    def noted(self, t) -> None:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            base = t._base if t._base is not None else t
            self._recent.append((base.data_ptr(), base.data_ptr() + base.numel() * base.element_size()))

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        slots = [i for i, t in enumerate(_lib.SIGNATURES.get(name, (None, []))[1]) if t is _lib.P]

        def call(*args):
            stream = torch.cuda.current_stream().cuda_stream
            addrs = []
            for i in slots:
                a = args[i]
                if isinstance(a, ctypes.Array):
                    addrs += [getattr(job, f) for job in a for f, t in job._fields_ if t is ctypes.c_void_p]
                elif isinstance(a, int) and not (i == len(args) - 1 and a == stream):       # (the stream handle is no address)
                    addrs.append(a)
            if name in _TABLE_COLS:
                # the table is found through its own journal entry and read back now, while its owner is alive
                owner = next((ref() for ref, ptr, *_ in self._notes.values() if ptr == args[0] and ref() is not None), None)
                assert owner is not None and owner.shape[0] == args[1] and owner.dtype == torch.int64, (name, args[0])
                cols = owner.cpu()[:, :_TABLE_COLS[name]].reshape(-1).tolist()
                self.tables.append((name, len(cols)))
                addrs += cols
            recent = _spans(self._recent)
            self._recent.clear()
            self.seen += [(name, a) for a in addrs if a]
            self.late += [(name, a) for a in addrs if a and not _inside(a, recent)]
            return fn(*args)

        return call


def _train_step(family: str, autocast: bool) -> None:
    """forward, loss, backward, HipAdamW.step(), a second HipAdamW that clips, ModelEma.step(), and eval-mode forwards."""
    from deepfakedetection_amd.ema import ModelEma
    from deepfakedetection_amd.optim import HipAdamW, HipCrossEntropyLoss

    torch.manual_seed(4)
    model, size = _build(family)
    model = model.cuda().train()
    shadow = _build(family)[0].cuda()
    opt = HipAdamW(model.parameters(), lr=1e-3, weight_decay=5e-2)
    clipped = HipAdamW(model.parameters(), lr=1e-3, use_arena=False)
    clipped.set_clip(1.0)
    ema = ModelEma(model, shadow)
    n = 4 if family == "fastervit" else 8
    x, y = torch.randn(n, 3, size, size).cuda(), torch.randint(0, 2, (n,)).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        loss = HipCrossEntropyLoss(0.1)(model(x), y)
    loss.backward()
    opt.step()
    clipped.step()
    ema.step()
    model.eval()
    with torch.inference_mode(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        model(x)
        model(x)            # (the second pass of a kernels.BNEvalBatch owner is the batched one)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def journalled():
    """(recorder, the journal's address ranges) of one eager step per family under bf16 autocast and of the two attention
    families in f32 (there the batched-GEMM + softmax-rows attention runs).  The journal does not depend on a stream capture."""
    with pytest.MonkeyPatch.context() as mp, K.capture_journal() as notes:
        rec = _Recorder(_lib.load(), notes)
        note = K.journal_note
        mp.setattr(K, "_L", lambda: rec)
        mp.setattr(K, "journal_note", lambda t: (rec.noted(t), note(t))[1])
        for family, autocast in (("efficientnet", True), ("efficientformer", True), ("fastervit", True),
                                 ("efficientformer", False), ("fastervit", False)):
            _train_step(family, autocast)
    return rec, _spans((ptr, ptr + nbytes) for _, ptr, nbytes, _, _ in notes.values())


def test_the_steps_ran_every_entry_point_the_check_is_about(journalled):
    rec, _ = journalled
    names = {name for name, _ in rec.seen}
    assert not [n for n in _MUST_RUN if n not in names]
    assert {name for name, _ in rec.tables} == set(_TABLE_COLS) and sum(n for _, n in rec.tables) > 300


def test_every_address_the_library_received_is_in_the_journal(journalled):
    rec, spans = journalled
    missing = sorted({name for name, addr in rec.seen if not _inside(addr, spans)})
    print(f"{len(rec.seen)} addresses from {len({n for n, _ in rec.seen})} entry points, {len(spans)} disjoint journalled ranges")
    assert not missing, missing
    assert len(rec.seen) > 300


def test_every_address_was_journalled_by_the_call_that_passed_it(journalled):
    rec, _ = journalled
    assert not rec.late, sorted({name for name, _ in rec.late})
