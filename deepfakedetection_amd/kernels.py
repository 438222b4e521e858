"""Torch-tensor front end of the C ABI (include/dfd_hip.h).

Every function here takes NHWC tensors ([N, H, W, C] contiguous, f32 or bf16) that
live on a HIP device, allocates outputs with torch (device memory is torch's job),
and enqueues exactly the kernels of libdfd_hip.so on torch's current stream.  There
is no fallback: a CPU tensor or a missing library raises.

Only this module loads or calls the library, and a device address reaches it in two
ways: as a direct argument through the gate `_p`, or inside a table of addresses (job
array, chunk table) whose `AddressTable` the launching front end notes.  Both record
the tensor in the open capture journal: a captured graph's replay guard is complete.
"""

from __future__ import annotations

import contextlib
import functools
import ctypes
import math
import threading
import weakref
from dataclasses import dataclass

import os

import torch

from . import _lib
from ._lib import (
    ACT_NONE, ACT_SILU, BF16, CLIP_CFG_LEN, CLIP_STATE_LEN, F32, MAX_PARTIALS, MIX_CUTMIX, MIX_JOB_WORDS, MIX_KEEP, MIX_NCHW, MIX_NHWC, PRO_AFFINE2, PRO_BN_ACT,
    PRO_BN_ACT_GATE, PRO_NONE, DwShape, Prologue, StemShape, check,
)

_scratch: dict[tuple[int, int, str], torch.Tensor] = {}


def _L():
    return _lib.load()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dt(t: torch.Tensor | torch.dtype) -> int:
    """The ABI's dtype code of a tensor or of a torch.dtype."""
    dtype = t.dtype if isinstance(t, torch.Tensor) else t
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported activation dtype {dtype}")


# ---- capture journal (graph_step.GraphedTrainStep / GraphedForward).  A hipGraph records raw addresses.  While a capture
# is open every tensor whose address goes to the library is noted here (weak reference to the tensor — or to its base
# when it is a view — plus the address).  Nothing but `_p` (direct arguments) and `AddressTable.note` (addresses inside a
# job array or a chunk table) hands an address to the library, and both note it.  After the capture the owner keeps the
# entries that (a) are still alive, i.e. are owned by something outside the captured body (parameters, buffers, caches,
# the optimizer's state and tables, the Philox state), and (b) do not sit in the graph's private memory pool; before
# every replay it asserts that each of them still lives at the recorded address (`stale_entries`).  A cache that replaced or dropped a recorded tensor
# (dtype switch, regrown buffer, rebuilt table) then raises instead of letting the replay read or write freed memory.
_journal: dict | None = None


def _root(t: torch.Tensor) -> torch.Tensor:
    """The tensor that owns `t`'s memory: its base when `t` is a view."""
    return t._base if t._base is not None else t


def journal_note(t) -> None:
    """Record `t` (tensor, or an iterable of tensors / None) in the open capture journal; no-op when none is open."""
    j = _journal
    if j is None or t is None:
        return
    if not isinstance(t, torch.Tensor):
        for u in t:
            journal_note(u)
        return
    if not t.is_cuda:
        return
    base = _root(t)
    key = id(base)
    seen = j.get(key)
    if seen is None or seen[0]() is not base:
        if seen is not None:
            j[(key, len(j))] = seen             # the id() of a tensor that died was reused: its record moves aside
        try:
            j[key] = (weakref.ref(base), base.data_ptr(), base.numel() * base.element_size(), tuple(base.shape), base.dtype)
        except TypeError:
            pass


@contextlib.contextmanager
def capture_journal():
    """`with capture_journal() as notes:` around a stream capture; `notes` is filled while the body runs."""
    global _journal
    if _journal is not None:
        raise RuntimeError("nested capture journals")
    notes: dict = {}
    _journal = notes
    try:
        yield notes
    finally:
        _journal = None


def _pool_ranges(device) -> list[tuple[int, int]]:
    """Address ranges of the caching allocator's private (graph) pools on `device`."""
    out = []
    idx = torch.device(device).index
    for seg in torch.cuda.memory_snapshot():
        if seg.get("device") == (idx if idx is not None else torch.cuda.current_device()) and tuple(seg.get("segment_pool_id", (0, 0))) != (0, 0):
            out.append((seg["address"], seg["address"] + seg["total_size"]))
    return out


def journal_guard(notes: dict, device) -> list[tuple]:
    """The journal entries a replay depends on: still referenced after the capture, outside the graph pools."""
    pools = _pool_ranges(device)
    keep = []
    for ref, ptr, nbytes, shape, dtype in notes.values():
        if ref() is None or nbytes == 0:
            continue
        if any(lo <= ptr < hi for lo, hi in pools):
            continue
        keep.append((ref, ptr, nbytes, shape, dtype))
    return keep


def stale_entries(guard: list[tuple]) -> list[str]:
    """Descriptions of the guarded tensors that are gone or have moved (empty list: the graph may replay)."""
    bad = []
    for ref, ptr, nbytes, shape, dtype in guard:
        t = ref()
        if t is None:
            bad.append(f"{dtype} {shape} at {ptr:#x} was freed")
        elif t.data_ptr() != ptr or t.numel() * t.element_size() != nbytes:
            bad.append(f"{dtype} {shape} moved {ptr:#x} -> {t.data_ptr():#x}")
    return bad


def _p(t: torch.Tensor | None, strided: bool = False):
    """The gate: the device address of `t` as a library argument, noted in the open capture journal.  strided: the
    entry point takes the strides next to the address (dfd_bgemm), so `t` may be any view."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("dfd kernels need tensors on a HIP device (no CPU fallback)")
    if not strided and not t.is_contiguous():
        raise ValueError(f"dfd kernels need contiguous tensors, got shape {tuple(t.shape)} strides {t.stride()}")
    if _journal is not None:
        journal_note(t)
    return t.data_ptr()


class AddressTable:
    """What the owner of a table of raw addresses (a ctypes job array, an int64 chunk table `dev` in device memory) keeps
    beside its rows: the tensors the rows point at (weakly, by the tensor that owns the memory, like the journal) with the
    addresses they had when it was built, and the table's own device storage.  The launching front end calls note()."""

    def __init__(self, tensors, own=()) -> None:
        tensors = [t for t in tensors if t is not None]
        self.refs = [weakref.ref(_root(t)) for t in tensors]
        self.ptrs = [t.data_ptr() for t in tensors]
        self.own = [t for t in own if t is not None]
        self.host = self.dev = None

    def valid_for(self, tensors) -> bool:
        """Do `tensors` live where the rows say?  The table then refers to them (equal addresses, maybe new tensor objects)."""
        tensors = [t for t in tensors if t is not None]
        if len(tensors) != len(self.ptrs) or any(t.data_ptr() != p for t, p in zip(tensors, self.ptrs)):
            return False
        self.refs = [weakref.ref(_root(t)) for t in tensors]
        return True

    def upload(self, rows: list, device, old: "AddressTable | None" = None) -> None:
        """int64 `rows` -> `dev` through pinned memory, into `old`'s device storage when the shape is unchanged."""
        self.host = torch.tensor(rows, dtype=torch.int64).pin_memory()
        reuse = old is not None and old.dev is not None and old.dev.shape == self.host.shape
        self.dev = old.dev if reuse else torch.empty_like(self.host, device=device)
        self.dev.copy_(self.host, non_blocking=True)        # pinned + async: legal under stream capture

    def note(self) -> None:
        if _journal is not None:
            journal_note(r() for r in self.refs)
            journal_note(self.own)
            journal_note(self.dev)


def _table(table) -> tuple:
    """(address, rows) of an int64 chunk table for a launch: an AddressTable (noted) or a bare device tensor."""
    if isinstance(table, AddressTable):
        table.note()
        table = table.dev
    return _p(table), table.shape[0]


def _chk_nhwc(t: torch.Tensor) -> None:
    if t.dim() != 4 or not t.is_contiguous():
        raise ValueError("expected a contiguous [N, H, W, C] tensor")


def scratch(device: torch.device, name: str, nbytes: int) -> torch.Tensor:
    """A grow-only f32 scratch buffer per (device, stream, purpose): reuse is ordered by the stream it belongs to,
    so two models / threads on different streams never share a buffer (the C ABI itself is re-entrant).

    While the stream is being captured into a hipGraph the buffer is a fresh allocation instead: it comes from the
    graph's private pool, which lives exactly as long as the graph.  A cached buffer would be recorded by address and
    could later be replaced (grown) and freed by code outside the graph while replays still write to it."""
    need = (nbytes + 3) // 4
    if torch.cuda.is_current_stream_capturing():
        buf = torch.empty(max(need, 1), dtype=torch.float32, device=device)
        if _sum_batch.open:
            _sum_batch.keep.append(buf)                     # the recorded sums read it at sum_batch's exit
        return buf
    if _sum_batch.open:
        # every weight gradient of an open batch keeps its own workspace until the batch is summed; with the sums riding along as
        # passengers of later launches (sum_batch) that is up to two batches later: three generations of names
        name = f"{name}#{_sum_batch.gen}#{_sum_batch.count}"
        _sum_batch.count += 1
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream, name)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.empty(max(need, 1), dtype=torch.float32, device=device)
        _scratch[key] = buf
    return buf


class _SumBatchState(threading.local):
    """Per host thread, like the library's own batch state (dfd_sum_batch_begin is thread-local)."""

    def __init__(self) -> None:
        self.open, self.count, self.keep, self.gen, self.temp_dest = False, 0, [], 0, False


_sum_batch = _SumBatchState()
_DEFER_SUMS = os.environ.get("DFD_DEFER_SUMS", "1") != "0"      # A/B switch: 0 = every weight gradient sums its slab at once


@contextlib.contextmanager
def sum_batch():
    """Weight gradients computed inside the block leave their final partial-row summation to the block's exit, where
    one pair of launches adds them all (dfd_sum_batch_begin / _end): the returned gradient tensors are valid only after
    the block.  Nothing inside may read them, and nothing else that sums partial rows may run inside.  No-op when
    nested."""
    if _sum_batch.open or not _DEFER_SUMS:
        yield
        return
    check(_L().dfd_sum_batch_begin(), "dfd_sum_batch_begin")
    _sum_batch.open, _sum_batch.count, _sum_batch.temp_dest = True, 0, False
    try:
        yield
    finally:
        _sum_batch.open = False
        # (only when every gradient of the batch went straight into its arena slot, which autograd adopts as .grad without reading it)
        if PASSENGER_SUMS and passenger_sums_enabled and not _sum_batch.temp_dest and _register_backward_flush():
            # the sums are read by the optimizer only: instead of two launches at the end of every block they ride along as extra
            # workgroups of the next two act_bn_bwd launches (one per block) and whatever is left is launched at the end of the
            # backward pass (csrc/dfd_dwconv.hip, dfd_sum_batch_end_deferred)
            rc = _L().dfd_sum_batch_end_deferred()
            with _passenger_lock:
                _passenger_keep.extend(_sum_batch.keep)     # (captured runs: the slabs live until the flush)
            deferred_ends[0] += 1
            _sum_batch.gen = (_sum_batch.gen + 1) % 3
        else:
            rc = _L().dfd_sum_batch_end()
        _sum_batch.keep.clear()
        check(rc, "dfd_sum_batch_end")


# ---- sums as passengers (see sum_batch).  DFD_PASSENGER_SUMS=0: two launches at the end of every block (A/B switch);
# passenger_sums_enabled is cleared by dp.GradAllReducer: a gradient bucket may be handed to RCCL as soon as its last backward kernel
# has been launched, which a sum still waiting for its carrier would not be part of.
PASSENGER_SUMS = os.environ.get("DFD_PASSENGER_SUMS", "1") != "0"
passenger_sums_enabled = True
_passenger_lock = threading.Lock()
_passenger_keep: list = []
# the autograd graph task (torch._C._current_graph_task_id) whose end-of-backward callback will flush what is parked; None: no flush is
# queued.  A backward that dies in an exception never runs its callbacks, so a bool set here and cleared by the flush would stay set and
# every later backward would park its last batches without a flush: keyed by the task, the next backward sees a different id
_passenger_task: int | None = None
deferred_ends = [0]                                 # batches handed to dfd_sum_batch_end_deferred (a counter for tests)


def flush_passengers() -> None:
    """Launch every sum that still waits for a carrier on the current stream (the end of a backward pass; also safe to call at any
    time on the stream the backward ran on)."""
    global _passenger_task
    with _passenger_lock:
        _passenger_task = None
        keep = list(_passenger_keep)
        _passenger_keep.clear()
    check(_L().dfd_sum_passengers_flush(_stream()), "dfd_sum_passengers_flush")
    del keep


def drop_passengers() -> None:
    """Forget every parked sum and its workspaces without launching anything (a backward pass or a capture that failed: the parked jobs
    point at memory that may no longer be theirs)."""
    global _passenger_task
    with _passenger_lock:
        check(_L().dfd_sum_passengers_discard(), "dfd_sum_passengers_discard")
        _passenger_keep.clear()
        _passenger_task = None


def _register_backward_flush() -> bool:
    """flush_passengers as an end-of-backward callback of the autograd engine, once per backward pass; False outside of one (the caller
    then sums at once)."""
    global _passenger_task
    task = torch._C._current_graph_task_id()
    if task < 0:
        return False
    with _passenger_lock:
        if _passenger_task == task:
            return True
    try:
        torch.autograd.Variable._execution_engine.queue_callback(flush_passengers)
    except RuntimeError:
        return False
    # the first batch of this backward pass: nothing may be waiting (the previous pass flushed); after a pass that died in an exception
    # something is — drop it, its workspaces may be gone
    with _passenger_lock:
        check(_L().dfd_sum_passengers_discard(), "dfd_sum_passengers_discard")
        _passenger_keep.clear()
        _passenger_task = task
    return True


def batched_sums(fn):
    """Decorator for a block's `backward`: runs it inside sum_batch()."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        with sum_batch():
            return fn(*args, **kwargs)
    return wrapper


def _nbytes(t: torch.Tensor | None) -> int:
    return 0 if t is None else t.numel() * t.element_size()


def _dst(out: torch.Tensor | None, shape, device, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """A caller-provided destination (gradient-arena slot) or a fresh tensor (f32 unless `dtype` says otherwise)."""
    if out is None:
        # a fresh tensor is handed to autograd, which adds it to (or clones it into) .grad as soon as the Function returns: the open
        # batch's sums may then not wait for a carrier launch (sum_batch)
        _sum_batch.temp_dest = True
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"bad gradient destination {tuple(out.shape)} for {tuple(shape)}")
    return out


def partials_buf(device: torch.device, C: int) -> torch.Tensor:
    # + 40 rows: room for the second stage of dfd_sum_rows when a slab is summed in place
    return scratch(device, "partials", (MAX_PARTIALS + 40) * 2 * C * 4)


@dataclass
class BNParams:
    """The tensors of one BatchNorm2d plus its hyper-parameters."""

    weight: torch.Tensor
    bias: torch.Tensor
    running_mean: torch.Tensor
    running_var: torch.Tensor
    momentum: float
    eps: float
    conv_bias: torch.Tensor | None = None      # bias of the producing convolution (timm ConvNorm), folded into the BN
    ls: torch.Tensor | None = None             # LayerScale gamma applied to the BN output, folded into (scale, shift)


# ------------------------------------------------------------------ BatchNorm
def bn_finalize(partials: torch.Tensor, nparts: int, count: int, bn: BNParams, update_running: bool = True) -> torch.Tensor:
    C = bn.weight.numel()
    state = torch.empty((4, C), dtype=torch.float32, device=partials.device)
    rm = bn.running_mean if update_running else None
    rv = bn.running_var if update_running else None
    check(_L().dfd_bn_finalize_ex(_p(partials), nparts, C, float(count), _p(bn.weight), _p(bn.bias), _p(bn.conv_bias),
                                  _p(bn.ls), _p(rm), _p(rv), bn.momentum, bn.eps, _p(state), _stream()), "dfd_bn_finalize_ex")
    return state


def bn_eval_coeffs(bn: BNParams) -> torch.Tensor:
    C = bn.weight.numel()
    state = torch.empty((4, C), dtype=torch.float32, device=bn.weight.device)
    check(_L().dfd_bn_eval_coeffs_ex(_p(bn.weight), _p(bn.bias), _p(bn.conv_bias), _p(bn.ls), _p(bn.running_mean),
                                     _p(bn.running_var), bn.eps, C, _p(state), _stream()), "dfd_bn_eval_coeffs_ex")
    return state


def bn_bwd_finalize(partials: torch.Tensor, nparts: int, count: int, gamma: torch.Tensor, beta: torch.Tensor | None,
                    ls: torch.Tensor | None, state: torch.Tensor, train: bool, want_bn: bool = True, want_ls: bool = False,
                    want_bias: bool = False, outs=(None, None, None, None)):
    """BatchNorm backward coefficients with LayerScale / convolution-bias gradients.
    Returns (coef, dgamma, dbeta, dls, dbias); outs: optional gradient-arena slots in that order."""
    C = gamma.numel()
    dev = gamma.device
    coef = torch.empty((3, C), dtype=torch.float32, device=dev)
    dgamma = _dst(outs[0], (C,), dev) if want_bn else None
    dbeta = _dst(outs[1], (C,), dev) if want_bn else None
    dls = _dst(outs[2], (C,), dev) if (want_ls and ls is not None) else None
    dbias = _dst(outs[3], (C,), dev) if want_bias else None
    check(_L().dfd_bn_bwd_finalize_ex(_p(partials), nparts, C, float(count), _p(gamma), _p(beta), _p(ls), _p(state), int(train),
                                      _p(dgamma), _p(dbeta), _p(dls), _p(dbias), 0, _p(coef), _stream()), "dfd_bn_bwd_finalize_ex")
    return coef, dgamma, dbeta, dls, dbias


def bn_act_apply(y: torch.Tensor, state: torch.Tensor, act: int, residual: torch.Tensor | None = None,
                 row_scale: torch.Tensor | None = None) -> torch.Tensor:
    _chk_nhwc(y)
    N, H, W, C = y.shape
    out = torch.empty_like(y)
    check(_L().dfd_bn_act_apply(_dt(y), _p(y), _p(state), act, _p(residual), _p(row_scale), _p(out), N, H * W, C,
                                _stream()), "dfd_bn_act_apply", str(tuple(y.shape)))
    return out


def bn_bwd_reduce(g: torch.Tensor, y: torch.Tensor, state: torch.Tensor, row_scale: torch.Tensor | None = None):
    _chk_nhwc(y)
    N, H, W, C = y.shape
    parts = partials_buf(y.device, C)
    n = ctypes.c_int(0)
    check(_L().dfd_bn_bwd_reduce(_dt(y), _p(g), _p(y), _p(state), _p(row_scale), N, H * W, C, _p(parts), MAX_PARTIALS,
                                 ctypes.byref(n), _stream()), "dfd_bn_bwd_reduce", str(tuple(y.shape)))
    return parts, n.value


_UNSUPPORTED = -2


def gemm_bias_act(x: torch.Tensor, w_nk, state: torch.Tensor, act: int, residual: torch.Tensor | None = None,
                  row_scale: torch.Tensor | None = None, want_raw: bool = False):
    """Linear layer without statistics in one kernel: act(scale * (x w^T) + shift) [* row_scale] [+ residual] -> (out, raw y or
    None), bit-identical to pwconv + bn_act_apply; None when the shape is not the fused kernel's (the caller runs the pair)."""
    if x.dtype != torch.bfloat16 or isinstance(w_nk, MxWeight):
        return None
    _chk_nhwc(x)
    N_, H, W, Kd = x.shape
    M, Nout = N_ * H * W, w_nk.shape[0]
    out = torch.empty((N_, H, W, Nout), dtype=x.dtype, device=x.device)
    raw = torch.empty_like(out) if want_raw else None
    rc = _L().dfd_gemm_bias_act(_dt(x), _p(x), _p(w_nk), M, Kd, Nout, _p(state), act, _p(residual), _p(row_scale), H * W,
                                _p(raw), _p(out), _stream())
    if rc == _UNSUPPORTED:
        return None
    check(rc, "dfd_gemm_bias_act", f"{tuple(x.shape)} -> {Nout}")
    return out, raw


def bias_grad(g: torch.Tensor, row_scale: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Sum of g [N,H,W,C] over its rows (times row_scale[n]) -> f32 [C]: the bias gradient of a Linear layer.  Inside
    sum_batch() the final summation is deferred to the block's batch like a weight gradient's (valid after the block)."""
    _chk_nhwc(g)
    N, H, W, C = g.shape
    nbytes = _L().dfd_bias_grad_ws(N, H * W, C)
    ws = scratch(g.device, "bias_ws", nbytes)
    db = _dst(out, (C,), g.device)
    check(_L().dfd_bias_grad(_dt(g), _p(g), _p(row_scale), N, H * W, C, _p(db), 0, _p(ws), ws.numel() * 4, _stream()),
          "dfd_bias_grad", str(tuple(g.shape)))
    return db


def act_bn_bwd(D: torch.Tensor | None, y: torch.Tensor, gate: torch.Tensor | None, dpool: torch.Tensor | None,
               state: torch.Tensor, act: int, se_job: tuple | None = None, want_dz: bool = True):
    """se_job: what se_bwd(defer_wgrad=True) returned — the block's squeeze-excite FC weight gradients then ride along as extra
    workgroups of this launch (dfd_act_bn_bwd_se) instead of being a launch of their own.
    want_dz=False (not with se_job): the partial sums only, dz is None and is not written (its consumer recomputes it: stem_bwd_fused)."""
    _chk_nhwc(y)
    N, H, W, C = y.shape
    if _passenger_task is not None and torch._C._current_graph_task_id() != _passenger_task:
        drop_passengers()               # parked by a backward pass that never reached its flush: this launch must not carry them
    dz = torch.empty_like(y) if want_dz or se_job is not None else None
    parts = partials_buf(y.device, C)
    n = ctypes.c_int(0)
    if se_job is not None:
        pooled, ws, R, dw1, db1, dw2, db2 = se_job
        check(_L().dfd_act_bn_bwd_se(_dt(y), _p(D), _p(y), _p(gate), _p(dpool), _p(state), act, _p(dz), N, H * W, C, _p(parts),
                                     MAX_PARTIALS, ctypes.byref(n), _p(pooled), _p(ws), R, _p(dw1), _p(db1), _p(dw2), _p(db2), 0,
                                     _stream()), "dfd_act_bn_bwd_se", str(tuple(y.shape)))
        return dz, parts, n.value
    check(_L().dfd_act_bn_bwd(_dt(y), _p(D), _p(y), _p(gate), _p(dpool), _p(state), act, _p(dz), N, H * W, C, _p(parts),
                              MAX_PARTIALS, ctypes.byref(n), _stream()), "dfd_act_bn_bwd", str(tuple(y.shape)))
    return dz, parts, n.value




def _pool_workspace(y: torch.Tensor, N: int, HW: int, C: int) -> torch.Tensor | None:
    """The pooling workspace (partial vectors of the H*W splits) as a tensor the caller keeps alive across the launch;
    None when the shape needs none."""
    nbytes = int(_L().dfd_pool_ws(_dt(y), N, HW, C))
    if nbytes == 0:
        return None
    return scratch(y.device, "pool_ws", nbytes)


def pool_act(y: torch.Tensor, state: torch.Tensor, act: int) -> torch.Tensor:
    _chk_nhwc(y)
    N, H, W, C = y.shape
    pooled = torch.empty((N, C), dtype=torch.float32, device=y.device)
    ws = _pool_workspace(y, N, H * W, C)
    check(_L().dfd_pool_act(_dt(y), _p(y), _p(state), act, _p(pooled), N, H * W, C, _p(ws), _nbytes(ws), _stream()), "dfd_pool_act")
    return pooled


def pool_bwd_reduce(D: torch.Tensor, y: torch.Tensor, state: torch.Tensor, act: int) -> torch.Tensor:
    _chk_nhwc(y)
    N, H, W, C = y.shape
    dgate = torch.empty((N, C), dtype=torch.float32, device=y.device)
    ws = _pool_workspace(y, N, H * W, C)
    check(_L().dfd_pool_bwd_reduce(_dt(y), _p(D), _p(y), _p(state), act, _p(dgate), N, H * W, C, _p(ws), _nbytes(ws), _stream()),
          "dfd_pool_bwd_reduce")
    return dgate


def scale_rows(x: torch.Tensor, row_scale: torch.Tensor) -> torch.Tensor:
    _chk_nhwc(x)
    N, H, W, C = x.shape
    out = torch.empty_like(x)
    check(_L().dfd_scale_rows(_dt(x), _p(x), _p(row_scale), _p(out), N, H * W, C, _stream()), "dfd_scale_rows")
    return out


# ------------------------------------------------------------------ input tail
def resize_crop_u8(flat_u8: torch.Tensor, jobs_u8: torch.Tensor, n: int, oh: int, ow: int, max_shrink: int) -> torch.Tensor:
    """Decoded uint8 RGB images packed back to back (`flat_u8`) + n 56-byte dfd_resize_job descriptors (`jobs_u8`, uint8 view)
    -> uint8 [n, oh, ow, 3]: Pillow-exact bilinear resize of each image's box, cropped to the output window."""
    if flat_u8.dtype != torch.uint8 or jobs_u8.dtype != torch.uint8 or jobs_u8.numel() != 56 * n:
        raise ValueError("resize_crop_u8: expected uint8 pixel bytes and n 56-byte job descriptors")
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=flat_u8.device)
    check(_L().dfd_resize_crop_u8(_p(flat_u8), _p(jobs_u8), _p(out), n, oh, ow, int(max_shrink), _stream()), "dfd_resize_crop_u8",
          f"n={n} out={oh}x{ow} shrink<={max_shrink}")
    return out


def augment_u8(src_u8: torch.Tensor, jobs_i32: torch.Tensor) -> torch.Tensor:
    """uint8 [N, H, W, 3] on the device + one 16-int job per picture (data.GpuInputTail.sample_augment) -> the rotated and
    colour-jittered uint8 batch, byte-exact with the PIL transforms of data.py (csrc/dfd_augment.hip)."""
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3 or not src_u8.is_contiguous():
        raise ValueError("expected a contiguous uint8 [N, H, W, 3] tensor")
    N, H, W, _ = src_u8.shape
    if jobs_i32.dtype != torch.int32 or jobs_i32.numel() != 16 * N or not jobs_i32.is_contiguous():
        raise ValueError("augment_u8: expected N jobs of 16 int32 each")
    out = torch.empty_like(src_u8)
    check(_L().dfd_augment_u8(_p(src_u8), _p(jobs_i32), _p(out), N, H, W, _stream()), "dfd_augment_u8", f"{tuple(src_u8.shape)}")
    return out


def augment_policy_u8(src_u8: torch.Tensor, jobs_i32: torch.Tensor) -> torch.Tensor:
    """uint8 [N, H, W, 3] on the device + one dfd_augment_policy_job per picture as a HOST int32 [N, data.AA_JOB_WORDS] tensor
    (data.pack_policy_jobs / GpuInputTail.sample_policy) -> flip, rotation, colour jitter and the RandAugment /
    TrivialAugmentWide operations in one launch, byte-exact with the PIL transforms of data.py (csrc/dfd_augment.hip, ABI 139).
    The entry point checks the host jobs before it launches anything; the upload does not block when the tensor is pinned."""
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3 or not src_u8.is_contiguous():
        raise ValueError("expected a contiguous uint8 [N, H, W, 3] tensor")
    N, H, W, _ = src_u8.shape
    if jobs_i32.is_cuda or jobs_i32.dtype != torch.int32 or tuple(jobs_i32.shape) != (N, _lib.AUG_POLICY_JOB_WORDS) \
            or not jobs_i32.is_contiguous():
        raise ValueError(f"augment_policy_u8: expected a host int32 [{N}, {_lib.AUG_POLICY_JOB_WORDS}] job tensor")
    out = torch.empty_like(src_u8)
    jobs_dev = jobs_i32.to(src_u8.device, non_blocking=True)
    check(_L().dfd_augment_policy_u8(_p(src_u8), jobs_i32.data_ptr(), _p(jobs_dev), _p(out), N, H, W, _stream()),
          "dfd_augment_policy_u8", f"{tuple(src_u8.shape)}")
    return out


def jpeg_u8(src_u8: torch.Tensor, jobs_i32: torch.Tensor, ws: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 [N, H, W, 3] on the device + one {quality, flip} pair per picture as a HOST int32 [N, 2] tensor -> each picture after
    a baseline JPEG encode at its quality and a decode, byte-exact with Pillow (csrc/dfd_jpeg.hip, ABI 142).  Quality 0 copies the
    picture through; flip 1 mirrors it in x first, copied or compressed.  `ws`: at least dfd_jpeg_ws bytes of uint8 scratch on the
    device (allocated when None).  The jobs are checked here; the upload does not block when the tensor is pinned."""
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3 or not src_u8.is_contiguous():
        raise ValueError("expected a contiguous uint8 [N, H, W, 3] tensor")
    N, H, W, _ = src_u8.shape
    if W < 5:
        raise ValueError(f"jpeg_u8: pictures must be at least 5 pixels wide, got {W}")
    if jobs_i32.is_cuda or jobs_i32.dtype != torch.int32 or tuple(jobs_i32.shape) != (N, 2) or not jobs_i32.is_contiguous():
        raise ValueError(f"jpeg_u8: expected a host int32 [{N}, 2] job tensor of (quality, flip)")
    if N and (int(jobs_i32[:, 0].min()) < 0 or int(jobs_i32[:, 0].max()) > 100 or int(jobs_i32[:, 1].min()) < 0
              or int(jobs_i32[:, 1].max()) > 1):
        raise ValueError("jpeg_u8: quality must be 0..100 and flip 0 or 1")
    need = _L().dfd_jpeg_ws(N, H, W)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=src_u8.device)
    elif ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need or ws.device != src_u8.device:
        raise ValueError(f"jpeg_u8: ws must be a contiguous uint8 tensor of at least {need} bytes on {src_u8.device}")
    out = torch.empty_like(src_u8)
    jobs_dev = jobs_i32.to(src_u8.device, non_blocking=True)
    check(_L().dfd_jpeg_u8(_p(src_u8), _p(jobs_dev), _p(ws), _p(out), N, H, W, _stream()), "dfd_jpeg_u8", f"{tuple(src_u8.shape)}")
    return out


def blur_u8(src_u8: torch.Tensor, jobs_i32: torch.Tensor) -> torch.Tensor:
    """uint8 [N, H, W, 3] on the device + one {r, ww, fw, 0} job per picture as a HOST int32 [N, 4] tensor (data.blur_plan;
    GpuInputTail._blur_jobs) -> each picture after Pillow's GaussianBlur, byte-exact, in one launch (csrc/dfd_blur.hip, ABI 144).
    A job with ww == 0, or with r outside 0.._lib.BLUR_MAX_RADIUS, copies its picture through.  H * W may not exceed
    _lib.BLUR_MAX_PIXELS.  The upload does not block when the tensor is pinned."""
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3 or not src_u8.is_contiguous():
        raise ValueError("expected a contiguous uint8 [N, H, W, 3] tensor")
    N, H, W, _ = src_u8.shape
    if H * W > _lib.BLUR_MAX_PIXELS:
        raise ValueError(f"blur_u8: pictures may have at most {_lib.BLUR_MAX_PIXELS} pixels, got {H}x{W}")
    if jobs_i32.is_cuda or jobs_i32.dtype != torch.int32 or tuple(jobs_i32.shape) != (N, 4) or not jobs_i32.is_contiguous():
        raise ValueError(f"blur_u8: expected a host int32 [{N}, 4] job tensor of (r, ww, fw, 0)")
    out = torch.empty_like(src_u8)
    jobs_dev = jobs_i32.to(src_u8.device, non_blocking=True)
    check(_L().dfd_blur_u8(_p(src_u8), _p(jobs_dev), _p(out), N, H, W, _stream()), "dfd_blur_u8", f"{tuple(src_u8.shape)}")
    return out


def image_prep(src_u8: torch.Tensor, mean, std, flip: torch.Tensor | None, erase: torch.Tensor | None) -> torch.Tensor:
    """uint8 [N, H, W, 3] on the device -> f32, returned as an [N, 3, H, W] channels_last view of the
    NHWC result (zero-copy: exactly what HipEfficientNet.forward turns back into NHWC)."""
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[3] != 3 or not src_u8.is_contiguous():
        raise ValueError("expected a contiguous uint8 [N, H, W, 3] tensor")
    N, H, W, _ = src_u8.shape
    dst = torch.empty((N, H, W, 3), dtype=torch.float32, device=src_u8.device)
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
    if flip is not None and (flip.dtype != torch.uint8 or flip.numel() != N):
        raise ValueError("flip must be uint8 [N]")
    if erase is not None and (erase.dtype != torch.int32 or erase.numel() != 4 * N):
        raise ValueError("erase must be int32 [N, 4]")
    check(_L().dfd_image_prep(_p(src_u8), _p(dst), N, H, W, m3, s3, _p(flip), _p(erase), _stream()), "dfd_image_prep")
    return dst.permute(0, 3, 1, 2)


# ------------------------------------------------------------------ squeeze-excite
def se_fc_fwd(pooled: torch.Tensor, w1, b1, w2, b2, act: int, w2t: torch.Tensor | None = None):
    """w2t given: the [R, C] copy of w2 is already up to date (DerivedWeights) and the transpose is skipped."""
    N, C = pooled.shape
    R = w1.shape[0]
    hpre = torch.empty((N, R), dtype=torch.float32, device=pooled.device)
    gate = torch.empty((N, C), dtype=torch.float32, device=pooled.device)
    ready = w2t is not None
    if not ready:
        w2t = torch.empty((R, C), dtype=torch.float32, device=pooled.device)
    check(_L().dfd_se_fc_fwd(_p(pooled), _p(w1), _p(b1), None if ready else _p(w2), _p(b2), N, C, R, act, _p(hpre), _p(gate),
                             _p(w2t), _stream()), "dfd_se_fc_fwd", f"C={C} R={R}")
    return hpre, gate, w2t


def se_fc_bwd(dgate, gate, hpre, pooled, w1, w2t, act: int, want_param_grads: bool = True, outs=(None, None, None, None)):
    """w2t: the [R, C] transpose returned by se_fc_fwd."""
    N, C = pooled.shape
    R = w1.shape[0]
    dev = pooled.device
    dpooled = torch.empty((N, C), dtype=torch.float32, device=dev)
    ws = scratch(dev, "se_ws", (N * C + 2 * N * R) * 4)
    if want_param_grads:
        dw1 = _dst(outs[0], (R, C), dev)
        db1 = _dst(outs[1], (R,), dev)
        dw2 = _dst(outs[2], (C, R), dev)
        db2 = _dst(outs[3], (C,), dev)
    else:
        dw1 = db1 = dw2 = db2 = None
    check(_L().dfd_se_fc_bwd(_p(dgate), _p(gate), _p(hpre), _p(pooled), _p(w1), _p(w2t), N, C, R, act, _p(dpooled),
                             _p(dw1), _p(db1), _p(dw2), _p(db2), 0, _p(ws), _stream()), "dfd_se_fc_bwd")
    return dpooled, dw1, db1, dw2, db2


def se_fwd(y: torch.Tensor, state: torch.Tensor, act_in: int, w1, b1, w2, b2, act: int, w2t: torch.Tensor | None = None):
    """pool_act + se_fc_fwd in two launches (dfd_se_fwd): returns pooled, hpre, gate, w2t."""
    _chk_nhwc(y)
    N, H, W, C = y.shape
    R = w1.shape[0]
    dev = y.device
    pooled = torch.empty((N, C), dtype=torch.float32, device=dev)
    hpre = torch.empty((N, R), dtype=torch.float32, device=dev)
    gate = torch.empty((N, C), dtype=torch.float32, device=dev)
    ready = w2t is not None
    if not ready:
        w2t = torch.empty((R, C), dtype=torch.float32, device=dev)
    ws = _pool_workspace(y, N, H * W, C)
    check(_L().dfd_se_fwd(_dt(y), _p(y), _p(state), act_in, N, H * W, C, _p(w1), _p(b1), None if ready else _p(w2), _p(b2), R,
                          act, _p(pooled), _p(hpre), _p(gate), _p(w2t), _p(ws), _nbytes(ws), _stream()), "dfd_se_fwd", f"C={C} R={R}")
    return pooled, hpre, gate, w2t


def se_bwd(D, y, state, act_in: int, gate, hpre, pooled, w1, w2t, act: int, want_param_grads: bool = True,
           outs=(None, None, None, None), defer_wgrad: bool = False):
    """pool_bwd_reduce + se_fc_bwd in three launches (dfd_se_bwd): returns dpooled, dw1, db1, dw2, db2.
    defer_wgrad (with want_param_grads): the third launch — the FC weight gradients, which only the optimizer reads — is left out
    and a sixth value is returned, the job for act_bn_bwd(se_job=...), whose launch then carries it; dw1 .. db2 are valid after
    that call.  The caller must make it its NEXT launch (the job points into this call's scratch workspace)."""
    _chk_nhwc(y)
    N, H, W, C = y.shape
    R = w1.shape[0]
    dev = y.device
    dpooled = torch.empty((N, C), dtype=torch.float32, device=dev)
    dgate = scratch(dev, "se_dgate", N * C * 4)
    ws = scratch(dev, "se_ws", (N * C + 2 * N * R) * 4)
    if want_param_grads:
        dw1 = _dst(outs[0], (R, C), dev)
        db1 = _dst(outs[1], (R,), dev)
        dw2 = _dst(outs[2], (C, R), dev)
        db2 = _dst(outs[3], (C,), dev)
    else:
        dw1 = db1 = dw2 = db2 = None
    pws = _pool_workspace(y, N, H * W, C)
    defer = defer_wgrad and want_param_grads
    check(_L().dfd_se_bwd(_dt(y), _p(D), _p(y), _p(state), act_in, N, H * W, C, _p(gate), _p(hpre), _p(pooled), _p(w1), _p(w2t),
                          R, act, _p(dgate), _p(dpooled), None if defer else _p(dw1), None if defer else _p(db1),
                          None if defer else _p(dw2), None if defer else _p(db2), 0, _p(pws), _nbytes(pws), _p(ws),
                          _stream()), "dfd_se_bwd")
    if defer_wgrad:
        return dpooled, dw1, db1, dw2, db2, ((pooled, ws, R, dw1, db1, dw2, db2) if defer else None)
    return dpooled, dw1, db1, dw2, db2


# ------------------------------------------------------------------ depthwise
def _dw_shape(x_shape, Ho: int, Wo: int, k: int, stride: int, pad_top: int, pad_left: int) -> DwShape:
    N, H, W, C = x_shape
    return DwShape(N, H, W, C, Ho, Wo, k, stride, pad_top, pad_left)


def dwconv_fwd(x: torch.Tensor, in_state: torch.Tensor | None, in_act: int, w: torch.Tensor, k: int, stride: int,
               pad_top: int, pad_left: int, Ho: int, Wo: int, stats: bool = True):
    """y = dwconv(act(bn(x))); w is torch's [C,1,k,k] f32 weight. Returns (y, partials, nparts)."""
    _chk_nhwc(x)
    N, H, W, C = x.shape
    y = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    shp = _dw_shape(x.shape, Ho, Wo, k, stride, pad_top, pad_left)
    parts = partials_buf(x.device, C) if stats else None
    n = ctypes.c_int(0)
    check(_L().dfd_dwconv_fwd(_dt(x), _p(x), _p(in_state), in_act, _p(w), _p(y), ctypes.byref(shp), _p(parts),
                              MAX_PARTIALS, ctypes.byref(n), _stream()), "dfd_dwconv_fwd", f"{tuple(x.shape)} k{k}s{stride}")
    return y, parts, n.value


def dwconv_bwd_data(dz: torch.Tensor, y: torch.Tensor | None, coef: torch.Tensor | None, w: torch.Tensor,
                    xin: torch.Tensor | None, in_state: torch.Tensor | None, in_act: int, in_shape, k: int, stride: int,
                    pad_top: int, pad_left: int):
    """Returns (dzin, partials, nparts); xin=None: plain input gradient, no statistics."""
    N, H, W, C = in_shape
    Ho, Wo = dz.shape[1], dz.shape[2]
    dzin = torch.empty((N, H, W, C), dtype=dz.dtype, device=dz.device)
    shp = _dw_shape(in_shape, Ho, Wo, k, stride, pad_top, pad_left)
    parts = partials_buf(dz.device, C) if xin is not None else None
    n = ctypes.c_int(0)
    check(_L().dfd_dwconv_bwd_data(_dt(dz), _p(dz), _p(y), _p(coef), _p(w), _p(xin), _p(in_state), in_act, _p(dzin),
                                   ctypes.byref(shp), _p(parts), MAX_PARTIALS, ctypes.byref(n), _stream()),
          "dfd_dwconv_bwd_data", f"{tuple(in_shape)} k{k}s{stride}")
    return dzin, parts, n.value


def dwconv_bwd_weight(dz: torch.Tensor, y: torch.Tensor | None, coef: torch.Tensor | None, xin: torch.Tensor,
                      in_state: torch.Tensor | None, in_act: int, k: int, stride: int, pad_top: int, pad_left: int,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    N, H, W, C = xin.shape
    Ho, Wo = dz.shape[1], dz.shape[2]
    shp = _dw_shape(xin.shape, Ho, Wo, k, stride, pad_top, pad_left)
    nbytes = _L().dfd_dwconv_bwd_weight_ws(ctypes.byref(shp))
    ws = scratch(dz.device, "wgrad_ws", nbytes)
    dw = _dst(out, (C, 1, k, k), dz.device)
    check(_L().dfd_dwconv_bwd_weight(_dt(dz), _p(dz), _p(y), _p(coef), _p(xin), _p(in_state), in_act, _p(dw),
                                     ctypes.byref(shp), 0, _p(ws), ws.numel() * 4, _stream()), "dfd_dwconv_bwd_weight")
    return dw


# ------------------------------------------------------------------ pointwise
def _pro(mode: int = PRO_NONE, act: int = ACT_NONE, HW: int = 1, a2=None, coef=None, gate=None) -> Prologue:
    pr = Prologue(mode, act, HW, 0, _p(a2), _p(coef), _p(gate))
    pr._keep = (a2, coef, gate)       # the struct holds raw pointers: keep the tensors alive with it
    pr._nbytes = sum(t.numel() * t.element_size() for t in pr._keep if t is not None)
    return pr


def pro_bn_act(state: torch.Tensor, act: int) -> Prologue:
    return _pro(PRO_BN_ACT, act, 1, None, state, None)


def pro_bn_act_gate(state: torch.Tensor, act: int, gate: torch.Tensor, HW: int) -> Prologue:
    return _pro(PRO_BN_ACT_GATE, act, HW, None, state, gate)


_identity_states: dict = {}


def identity_state(device: torch.device, C: int) -> torch.Tensor:
    """float[4][C] BatchNorm state of the identity map (scale 1, shift 0, mean 0, rstd 1): turns the BN_ACT_GATE prologue into
    a gate-only one for operands that were stored activated."""
    key = (device.type, device.index, C)
    st = _identity_states.get(key)
    if st is None:
        with torch.inference_mode(False):               # a plain tensor: the cache outlives the caller's inference_mode block
            st = torch.zeros((4, C), dtype=torch.float32, device=device)
            st[0].fill_(1.0)
            st[3].fill_(1.0)
        if not (device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            _identity_states[key] = st          # a tensor born inside a capture belongs to that graph's pool: not cached
    return st


def pro_affine2(a2: torch.Tensor, coef: torch.Tensor) -> Prologue:
    return _pro(PRO_AFFINE2, ACT_NONE, 1, a2, coef, None)


def prep_weights(w: torch.Tensor, dtype: torch.dtype, want_nk: bool = True, want_kn: bool = True):
    """f32 master [Nout, K(,1,1)] -> (w_nk, w_kn) in the activation dtype."""
    Nn, K = w.shape[0], w.shape[1]
    w_nk = torch.empty((Nn, K), dtype=dtype, device=w.device) if want_nk else None
    w_kn = torch.empty((K, Nn), dtype=dtype, device=w.device) if want_kn else None
    check(_L().dfd_pw_prep_weights(_dt(dtype), _p(w), _p(w_nk), _p(w_kn), Nn, K, _stream()), "dfd_pw_prep_weights")
    return w_nk, w_kn


class DerivedWeights:
    """Every per-step derived weight of a network, refreshed by ONE batched launch per forward pass:
    the activation-dtype copies [N][K] / [K][N] of the 1x1 convolution weights and the [R][C] copies of the
    squeeze-excite expand weights.  `items`: (f32 source, want_nk, want_kn, is_se) in a fixed order; the
    destination buffers are allocated once and handed out by index."""

    def __init__(self, items: list[tuple[torch.Tensor, bool, bool, bool]], dtype: torch.dtype) -> None:
        self.dtype = dtype
        self.out: list[tuple[torch.Tensor | None, torch.Tensor | None]] = []
        jobs = (_lib.PrepJob * len(items))()
        for i, (src, want_nk, want_kn, is_se) in enumerate(items):
            n, kdim = src.shape[0], src.shape[1]
            dt = torch.float32 if is_se else dtype
            nk = torch.empty((n, kdim), dtype=dt, device=src.device) if want_nk else None
            kn = torch.empty((kdim, n), dtype=dt, device=src.device) if want_kn else None
            self.out.append((nk, kn))
            jobs[i] = _lib.PrepJob(src.data_ptr(), nk.data_ptr() if nk is not None else None,
                                   kn.data_ptr() if kn is not None else None, n, kdim, _dt(dt), 0)
        self._jobs = jobs
        self.table = AddressTable([src for src, _, _, _ in items], own=[t for pair in self.out for t in pair])

    def valid_for(self, sources: list[torch.Tensor], dtype: torch.dtype) -> bool:
        return dtype == self.dtype and self.table.valid_for(sources)

    def refresh(self) -> None:
        self.table.note()
        check(_L().dfd_prep_weights_multi(self._jobs, len(self._jobs), _stream()), "dfd_prep_weights_multi")


# ---- MX fp8 weights (include/dfd_hip.h "MX fp8"): FasterViT's Linear layers with `fp8_weights` on ------------------------
class MxWeight:
    """One Linear weight in OCP MX fp8: q [N][K] e4m3fn bytes + scale [N][K/32] e8m0 bytes.  kernels.pwconv() takes it in
    place of the bf16 [N][K] copy and then runs quantise-activations + dfd_mx_gemm."""

    __slots__ = ("q", "scale", "N", "K")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor) -> None:
        self.q, self.scale = q, scale
        self.N, self.K = q.shape

    @property
    def shape(self):
        return (self.N, self.K)

    @property
    def dtype(self):
        return torch.uint8


class MxWeights:
    """Every fp8 weight of a network, re-quantised from the f32 masters by ONE batched launch per forward pass
    (dfd_mx_quant_weights_multi) together with the dequantised [K][N] copies the bf16 backward multiplies by."""

    def __init__(self, sources: list[torch.Tensor], dtype: torch.dtype) -> None:
        self.dtype = dtype
        self.out: list[tuple[MxWeight, torch.Tensor]] = []
        jobs = (_lib.MxJob * len(sources))()
        for i, src in enumerate(sources):
            n, kdim = src.shape
            if kdim % 128:
                raise ValueError(f"MX fp8 weights need K % 128 == 0, got {tuple(src.shape)}")
            q = torch.empty((n, kdim), dtype=torch.uint8, device=src.device)
            sc = torch.empty((n, kdim // 32), dtype=torch.uint8, device=src.device)
            kn = torch.empty((kdim, n), dtype=dtype, device=src.device)
            self.out.append((MxWeight(q, sc), kn))
            jobs[i] = _lib.MxJob(src.data_ptr(), q.data_ptr(), sc.data_ptr(), kn.data_ptr(), n, kdim, _dt(dtype), 0)
        self._jobs = jobs
        self.table = AddressTable(sources, own=[t for w, kn in self.out for t in (w.q, w.scale, kn)])

    def valid_for(self, sources: list[torch.Tensor], dtype: torch.dtype) -> bool:
        return dtype == self.dtype and self.table.valid_for(sources)

    def refresh(self) -> None:
        self.table.note()
        check(_L().dfd_mx_quant_weights_multi(self._jobs, len(self._jobs), _stream()), "dfd_mx_quant_weights_multi")


def mx_quant_weight(w: torch.Tensor, dtype: torch.dtype = torch.bfloat16):
    """(MxWeight, dequantised [K][N] copy) of one f32 [N][K] weight."""
    mw = MxWeights([w], dtype)
    mw.refresh()
    return mw.out[0]


def mx_quant_rows(a: torch.Tensor, pro: Prologue | None = None):
    """a [..., K] (bf16 / f32) -> (q uint8 [M][K], scale uint8 [M][K/32]) after the optional BN+activation prologue."""
    Kd = a.shape[-1]
    M = a.numel() // Kd
    q = torch.empty((M, Kd), dtype=torch.uint8, device=a.device)
    sc = torch.empty((M, Kd // 32), dtype=torch.uint8, device=a.device)
    check(_L().dfd_mx_quant_rows(_dt(a), _p(a), ctypes.byref(pro) if pro is not None else None, _p(q), _p(sc), M, Kd, _stream()),
          "dfd_mx_quant_rows", f"M={M} K={Kd}")
    return q, sc


def mx_gemm(aq: torch.Tensor, ascale: torch.Tensor, w: MxWeight, out_dtype: torch.dtype, out_shape=None) -> torch.Tensor:
    M, Kd = aq.shape
    if Kd != w.K:
        raise ValueError(f"mx_gemm: K mismatch {Kd} vs {w.K}")
    out = torch.empty(out_shape if out_shape is not None else (M, w.N), dtype=out_dtype, device=aq.device)
    check(_L().dfd_mx_gemm(_p(aq), _p(ascale), _p(w.q), _p(w.scale), _dt(out_dtype), _p(out), M, Kd, w.N, _stream()),
          "dfd_mx_gemm", f"M={M} K={Kd} N={w.N}")
    return out


def _bn_eval_jobs(bns: list):
    """(coefficient blocks [4][C] cut from one buffer, BnEvalJob array, AddressTable) for a list of BNParams."""
    tens = [(bn.weight, bn.bias, bn.conv_bias, bn.ls, bn.running_mean, bn.running_var) for bn in bns]
    with torch.inference_mode(False):
        flat = torch.empty(sum(4 * ts[4].numel() for ts in tens), dtype=torch.float32, device=tens[0][4].device)
    states, jobs, at = [], (_lib.BnEvalJob * len(bns))(), 0
    for i, (bn, ts) in enumerate(zip(bns, tens)):
        C = ts[4].numel()
        states.append(flat[at:at + 4 * C].view(4, C))
        at += 4 * C
        jobs[i] = _lib.BnEvalJob(*(None if t is None else t.data_ptr() for t in ts), states[i].data_ptr(), float(bn.eps), C)
    return states, jobs, AddressTable([t for ts in tens for t in ts], own=[flat])


class BNEvalBatch:
    """The eval-mode BatchNorm coefficient requests of one forward pass of a network (kernels.bn_eval_coeffs: real
    BatchNorms in eval mode, and the identity statistics that carry a Linear layer's bias / LayerScale), recorded in call
    order on the first pass and from then on computed by ONE batched launch at the start of the pass and handed out in
    the same order.  Every hand-out is checked against the recorded pointers; any mismatch falls back to the per-layer
    kernel and re-records.  Use through functions.bn_eval_batch()."""

    def __init__(self) -> None:
        self.keys: list[tuple] | None = None
        self.states, self._jobs, self.table = [], None, None
        self._rec: list[tuple[tuple, BNParams]] = []
        self.pos, self.ok = 0, True

    @staticmethod
    def _key(p: "BNParams") -> tuple:
        return (_p(p.weight), _p(p.bias), _p(p.conv_bias), _p(p.ls), _p(p.running_mean), _p(p.running_var), float(p.eps),
                int(p.running_mean.numel()))

    def begin(self) -> None:
        self.pos, self.ok, self._rec = 0, True, []
        if self.keys is not None:
            self.table.note()
            check(_L().dfd_bn_eval_coeffs_multi(self._jobs, len(self._jobs), _stream()), "dfd_bn_eval_coeffs_multi")

    def request(self, p: "BNParams") -> torch.Tensor:
        key = self._key(p)
        if self.keys is None:
            self._rec.append((key, p))
            return bn_eval_coeffs(p)
        if self.ok and self.pos < len(self.keys) and self.keys[self.pos] == key:
            st = self.states[self.pos]
            self.pos += 1
            return st
        self.ok = False
        return bn_eval_coeffs(p)

    def end(self) -> None:
        if self.keys is None:
            if self._rec:
                self.states, self._jobs, self.table = _bn_eval_jobs([p for _, p in self._rec])
                self.keys = [k for k, _ in self._rec]
        elif not self.ok or self.pos != len(self.keys):
            self.keys, self.states, self._jobs, self.table = None, [], None, None      # the pass changed: record again
        self._rec = []


def pwconv(a: torch.Tensor, pro: Prologue | None, w_nk: torch.Tensor, residual: torch.Tensor | None = None,
           stats: bool = False):
    """out[..., Nout] = P(a)[..., K] @ w_nk[Nout, K]^T (+ residual). Returns (out, partials, nparts).
    w_nk may be an MxWeight (fp8 weights): activations are then quantised to MX fp8 behind the prologue and the product
    runs on the block-scaled fp8 MFMA (no residual / statistics in that form)."""
    if isinstance(w_nk, MxWeight):
        if residual is not None or stats:
            raise ValueError("the MX fp8 GEMM has no residual / statistics epilogue")
        aq, asc = mx_quant_rows(a, pro)
        return mx_gemm(aq, asc, w_nk, a.dtype, (*a.shape[:-1], w_nk.N)), None, 0
    K = a.shape[-1]
    M = a.numel() // K
    Nout = w_nk.shape[0]
    out = torch.empty((*a.shape[:-1], Nout), dtype=a.dtype, device=a.device)
    parts = partials_buf(a.device, Nout) if stats else None
    n = ctypes.c_int(0)
    check(_L().dfd_pwconv_fwd(_dt(a), _p(a), ctypes.byref(pro) if pro is not None else None, _p(w_nk), _p(out),
                              _p(residual), M, K, Nout, _p(parts), MAX_PARTIALS, ctypes.byref(n), _stream()),
          "dfd_pwconv_fwd", f"M={M} K={K} N={Nout}")
    return out, parts, n.value


# ---- eval / inference form of the MBConv block (include/dfd_hip.h "eval / inference form") ---------------------
def pwconv_eval(a: torch.Tensor, w_nk: torch.Tensor, out_state: torch.Tensor, out_act: int) -> torch.Tensor:
    """out = act(scale * (a @ w_nk^T) + shift) with this layer's own BatchNorm coefficients, stored activated."""
    K = a.shape[-1]
    M = a.numel() // K
    Nout = w_nk.shape[0]
    out = torch.empty((*a.shape[:-1], Nout), dtype=a.dtype, device=a.device)
    check(_L().dfd_pwconv_fwd_eval(_dt(a), _p(a), _p(w_nk), _p(out_state), out_act, _p(out), M, K, Nout, _stream()),
          "dfd_pwconv_fwd_eval", f"M={M} K={K} N={Nout}")
    return out


def dwconv_eval(x: torch.Tensor, w: torch.Tensor, out_state: torch.Tensor, out_act: int, k: int, stride: int, pad_top: int,
                pad_left: int, Ho: int, Wo: int):
    """y = act(bn(dwconv(x))) stored activated + per-(tile, image) channel sums of y. Returns (y, pool_parts, ntiles)."""
    _chk_nhwc(x)
    N, H, W, C = x.shape
    y = torch.empty((N, Ho, Wo, C), dtype=x.dtype, device=x.device)
    shp = _dw_shape(x.shape, Ho, Wo, k, stride, pad_top, pad_left)
    tiles = _L().dfd_dwconv_fwd_eval_tiles(_dt(x), ctypes.byref(shp))
    if tiles < 1:
        raise ValueError(f"dfd_dwconv_fwd_eval: unsupported shape {tuple(x.shape)} k{k}s{stride}")
    parts = torch.empty((tiles, N, C), dtype=torch.float32, device=x.device)
    n = ctypes.c_int(0)
    check(_L().dfd_dwconv_fwd_eval(_dt(x), _p(x), _p(w), _p(out_state), out_act, _p(y), ctypes.byref(shp), _p(parts),
                                   ctypes.byref(n), _stream()), "dfd_dwconv_fwd_eval", f"{tuple(x.shape)} k{k}s{stride}")
    assert n.value == tiles
    return y, parts, tiles


def se_fwd_parts(parts: torch.Tensor, HW: int, w1, b1, w2, b2, act: int, w2t: torch.Tensor | None = None):
    """The squeeze-excite branch from the producer's per-tile channel sums (no pooling pass): returns pooled, gate, w2t."""
    tiles, N, C = parts.shape
    R = w1.shape[0]
    dev = parts.device
    pooled = torch.empty((N, C), dtype=torch.float32, device=dev)
    hpre = torch.empty((N, R), dtype=torch.float32, device=dev)
    gate = torch.empty((N, C), dtype=torch.float32, device=dev)
    ready = w2t is not None
    if not ready:
        w2t = torch.empty((R, C), dtype=torch.float32, device=dev)
    check(_L().dfd_se_fwd_parts(_p(parts), tiles, N, HW, C, _p(w1), _p(b1), None if ready else _p(w2), _p(b2), R, act,
                                _p(pooled), _p(hpre), _p(gate), _p(w2t), _stream()), "dfd_se_fwd_parts", f"C={C} R={R}")
    return pooled, gate, w2t


def pwconv_wgrad(p: torch.Tensor, pro_p: Prologue | None, q: torch.Tensor, pro_q: Prologue | None,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """dw[Ni, Nj] = sum_m P(p)[m, i] * Q(q)[m, j]."""
    Ni, Nj = p.shape[-1], q.shape[-1]
    M = p.numel() // Ni
    nbytes = _L().dfd_pwconv_wgrad_ws(M, Ni, Nj)
    ws = scratch(p.device, "wgrad_ws", nbytes)
    dw = _dst(None if out is None else out.view(Ni, Nj), (Ni, Nj), p.device)
    check(_L().dfd_pwconv_wgrad(_dt(p), _p(p), ctypes.byref(pro_p) if pro_p is not None else None, Ni, _p(q),
                                ctypes.byref(pro_q) if pro_q is not None else None, Nj, M, _p(dw), 0, _p(ws),
                                ws.numel() * 4, _stream()), "dfd_pwconv_wgrad", f"M={M} Ni={Ni} Nj={Nj}")
    return dw


def pwconv_bwd_fused_ok(dz: torch.Tensor, x: torch.Tensor) -> bool:
    """Shapes dfd_pwconv_bwd_fused serves (include/dfd_hip.h).  Asked BEFORE the caller takes the weight gradient's arena slot:
    a slot handed to a call that then declines would be lost to the fallback (its gradient would land outside the arena)."""
    Cm, Cin = dz.shape[-1], x.shape[-1]
    M = dz.numel() // Cm
    if not (dz.dtype == torch.bfloat16 and M >= 2048 * 32 * 3 and Cin <= Cm and Cin % 8 == 0 and Cm % 8 == 0):
        return False
    return Cin <= 32 and (Cm <= 128 or (Cm <= 144 and Cm % 16 == 0))


def pwconv_bwd_fused(dz: torch.Tensor, y: torch.Tensor, coef: torch.Tensor, x: torch.Tensor, w_kn: torch.Tensor,
                     residual: torch.Tensor | None, out_w: torch.Tensor | None = None):
    """The expand layer's data AND weight gradient from one pass over (dz, y) (csrc/dfd_pwtnw.hip, DG): returns (dx, dw [Cm, Cin])
    or None when the shape is not the fused kernel's (the caller runs pwconv + pwconv_wgrad; see pwconv_bwd_fused_ok)."""
    if not pwconv_bwd_fused_ok(dz, x):
        return None
    Cm, Cin = dz.shape[-1], x.shape[-1]
    M = dz.numel() // Cm
    nbytes = _L().dfd_pwconv_wgrad_ws(M, Cm, Cin)
    ws = scratch(dz.device, "wgrad_ws", nbytes)
    dx = torch.empty_like(x)
    dw = _dst(None if out_w is None else out_w.view(Cm, Cin), (Cm, Cin), dz.device)
    rc = _L().dfd_pwconv_bwd_fused(_dt(dz), _p(dz), _p(y), _p(coef), _p(x), _p(w_kn), _p(residual), M, Cm, Cin, _p(dx), _p(dw), 0,
                                   _p(ws), ws.numel() * 4, _stream())
    check(rc, "dfd_pwconv_bwd_fused", f"M={M} Cm={Cm} Cin={Cin}")       # (declining here would have cost the caller its arena slot)
    return dx, dw


# ------------------------------------------------------------------ stem
def _stem_shape(x_shape, Cout: int, Ho: int, Wo: int, k: int, stride: int, pt: int, pl: int) -> StemShape:
    N, H, W, _ = x_shape
    return StemShape(N, H, W, Cout, Ho, Wo, k, stride, pt, pl)


def stem_conv_fwd(x: torch.Tensor, w: torch.Tensor, out_dtype: torch.dtype, stride: int, pad_top: int, pad_left: int,
                  Ho: int, Wo: int, stats: bool = True):
    """x: [N,H,W,3] f32; w: [Cout,3,k,k] f32."""
    _chk_nhwc(x)
    if x.dtype != torch.float32 or x.shape[3] != 3:
        raise ValueError("stem input must be f32 [N,H,W,3]")
    Cout, k = w.shape[0], w.shape[2]
    y = torch.empty((x.shape[0], Ho, Wo, Cout), dtype=out_dtype, device=x.device)
    shp = _stem_shape(x.shape, Cout, Ho, Wo, k, stride, pad_top, pad_left)
    parts = partials_buf(x.device, Cout) if stats else None
    n = ctypes.c_int(0)
    check(_L().dfd_stem_conv_fwd(_dt(y), _p(x), _p(w), _p(y), ctypes.byref(shp), _p(parts), MAX_PARTIALS,
                                 ctypes.byref(n), _stream()), "dfd_stem_conv_fwd")
    return y, parts, n.value


def stem_conv_wgrad(x: torch.Tensor, dz: torch.Tensor, y: torch.Tensor | None, coef: torch.Tensor | None, k: int,
                    stride: int, pad_top: int, pad_left: int, out: torch.Tensor | None = None) -> torch.Tensor:
    Cout, Ho, Wo = dz.shape[3], dz.shape[1], dz.shape[2]
    shp = _stem_shape(x.shape, Cout, Ho, Wo, k, stride, pad_top, pad_left)
    nbytes = _L().dfd_stem_conv_wgrad_ws(ctypes.byref(shp))
    ws = scratch(dz.device, "wgrad_ws", nbytes)
    dw = _dst(out, (Cout, 3, k, k), dz.device)
    check(_L().dfd_stem_conv_wgrad(_dt(dz), _p(x), _p(dz), _p(y), _p(coef), _p(dw), ctypes.byref(shp), 0, _p(ws),
                                   ws.numel() * 4, _stream()), "dfd_stem_conv_wgrad")
    return dw


def stem_bwd_fused_ok(x: torch.Tensor, y: torch.Tensor, k: int, stride: int, pad_top: int, pad_left: int) -> bool:
    """Whether stem_bwd_fused serves this stem (bf16, 16 or 32 output channels, the matrix-core weight-gradient shapes)."""
    if y.dtype != torch.bfloat16 or y.dim() != 4 or not y.is_contiguous():
        return False
    shp = _stem_shape(x.shape, y.shape[3], y.shape[1], y.shape[2], k, stride, pad_top, pad_left)
    return bool(_L().dfd_stem_bwd_fused_ok(_dt(y), ctypes.byref(shp), _p(x)))


def stem_bwd_fused(x: torch.Tensor, g: torch.Tensor, y: torch.Tensor, state: torch.Tensor, act: int, coef: torch.Tensor, k: int,
                   stride: int, pad_top: int, pad_left: int, out: torch.Tensor | None = None, max_rows: int = 0) -> torch.Tensor:
    """The stem's weight gradient straight from the incoming gradient g (dfd_stem_bwd_fused): the kernel recomputes the dz that
    act_bn_bwd(g, y, state, act) would have stored, so that tensor never exists; same bits as act_bn_bwd + stem_conv_wgrad.
    coef: bn_bwd_finalize over the partial rows of act_bn_bwd(..., want_dz=False).  Only where stem_bwd_fused_ok says so."""
    _chk_nhwc(y)
    if g.shape != y.shape or g.dtype != y.dtype or not g.is_contiguous():
        raise ValueError("stem_bwd_fused: g must be a contiguous tensor of y's shape and dtype")
    Cout, Ho, Wo = y.shape[3], y.shape[1], y.shape[2]
    shp = _stem_shape(x.shape, Cout, Ho, Wo, k, stride, pad_top, pad_left)
    nbytes = _L().dfd_stem_conv_wgrad_ws(ctypes.byref(shp))
    ws = scratch(y.device, "wgrad_ws", nbytes)
    dw = _dst(out, (Cout, 3, k, k), y.device)
    check(_L().dfd_stem_bwd_fused(_dt(y), _p(x), _p(g), _p(y), _p(state), act, _p(coef), _p(dw), ctypes.byref(shp), 0, _p(ws),
                                  ws.numel() * 4, max_rows, _stream()), "dfd_stem_bwd_fused", str(tuple(y.shape)))
    return dw


# ------------------------------------------------------------------ head / loss / optimizer
def dropout(x: torch.Tensor, u: torch.Tensor, p: float) -> torch.Tensor:
    out = torch.empty_like(x)
    check(_L().dfd_dropout(_p(x), _p(u), p, _p(out), x.numel(), _stream()), "dfd_dropout")
    return out


def linear_fwd(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None) -> torch.Tensor:
    N, K = x.shape
    J = w.shape[0]
    out = torch.empty((N, J), dtype=torch.float32, device=x.device)
    check(_L().dfd_linear_fwd(_p(x), _p(w), _p(b), _p(out), N, K, J, _stream()), "dfd_linear_fwd")
    return out


def linear_bwd(dout: torch.Tensor, x: torch.Tensor, w: torch.Tensor, need_dx: bool, need_dw: bool, has_bias: bool,
               out_dw: torch.Tensor | None = None, out_db: torch.Tensor | None = None):
    N, K = x.shape
    J = w.shape[0]
    dev = x.device
    dx = torch.empty((N, K), dtype=torch.float32, device=dev) if need_dx else None
    dw = _dst(out_dw, (J, K), dev) if need_dw else None
    db = _dst(out_db, (J,), dev) if (need_dw and has_bias) else None
    check(_L().dfd_linear_bwd(_p(dout), _p(x), _p(w), _p(dx), _p(dw), _p(db), N, K, J, 0, _stream()), "dfd_linear_bwd")
    return dx, dw, db


def ce_loss(logits: torch.Tensor, targets: torch.Tensor, label_smoothing: float, grad_scale: float = 1.0,
            want_grad: bool = True):
    N, J = logits.shape
    dev = logits.device
    row_loss = torch.empty(N, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dlogits = torch.empty_like(logits) if want_grad else None
    check(_L().dfd_ce_loss(_p(logits), _p(targets), N, J, label_smoothing, grad_scale, _p(row_loss), _p(loss),
                           _p(dlogits), _stream()), "dfd_ce_loss")
    return loss, dlogits


def ce_loss_soft(logits: torch.Tensor, targets: torch.Tensor, label_smoothing: float, grad_scale: float = 1.0,
                 want_grad: bool = True):
    """ce_loss with probability targets, f32 [N, J] (torch's cross_entropy with a floating target; ABI 138)."""
    if targets.dtype != torch.float32 or targets.shape != logits.shape:
        raise ValueError(f"ce_loss_soft: targets must be f32 {tuple(logits.shape)}, got {targets.dtype} {tuple(targets.shape)}")
    N, J = logits.shape
    dev = logits.device
    row_loss = torch.empty(N, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dlogits = torch.empty_like(logits) if want_grad else None
    check(_L().dfd_ce_loss_soft(_p(logits), _p(targets), N, J, label_smoothing, grad_scale, _p(row_loss), _p(loss),
                                _p(dlogits), _stream()), "dfd_ce_loss_soft")
    return loss, dlogits


def ce_loss_w(logits: torch.Tensor, targets: torch.Tensor, label_smoothing: float, focal_gamma: float = 0.0,
              class_weight: torch.Tensor | None = None, grad_scale: float = 1.0, want_grad: bool = True,
              row_loss: torch.Tensor | None = None, dlogits: torch.Tensor | None = None):
    """Class-weighted and focal cross entropy (ABI 147): `targets` are class indices (int64 [N]) or probabilities (f32 [N, J]),
    `class_weight` is f32 [J] or None for all ones.  The mean follows torch: over sum_n w[t_n] with indices, over N with
    probabilities.  `row_loss` / `dlogits`: caller-owned destinations, every element is overwritten."""
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError(f"ce_loss_w: logits must be f32 [N, J], got {logits.dtype} {tuple(logits.shape)}")
    N, J = logits.shape
    soft = targets.is_floating_point()
    if soft and (targets.dtype != torch.float32 or targets.shape != logits.shape):
        raise ValueError(f"ce_loss_w: probability targets must be f32 {tuple(logits.shape)}, got {targets.dtype} {tuple(targets.shape)}")
    if not soft and (targets.dtype != torch.int64 or tuple(targets.shape) != (N,)):
        raise ValueError(f"ce_loss_w: index targets must be int64 [{N}], got {targets.dtype} {tuple(targets.shape)}")
    if class_weight is not None and (class_weight.dtype != torch.float32 or tuple(class_weight.shape) != (J,)):
        raise ValueError(f"ce_loss_w: class_weight must be f32 [{J}], got {class_weight.dtype} {tuple(class_weight.shape)}")
    if not (math.isfinite(focal_gamma) and focal_gamma >= 0.0) or not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"ce_loss_w: focal_gamma must be finite and >= 0 and label_smoothing in [0, 1), got {focal_gamma!r}, {label_smoothing!r}")
    dev = logits.device
    for out, shape in ((row_loss, (N,)), (dlogits, (N, J))):
        if out is not None and (tuple(out.shape) != shape or out.dtype != torch.float32):
            raise ValueError(f"ce_loss_w: bad destination {out.dtype} {tuple(out.shape)} for f32 {shape}")
    if row_loss is None:
        row_loss = torch.empty(N, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    denom = torch.empty(1, dtype=torch.float32, device=dev)
    if not want_grad:
        dlogits = None
    elif dlogits is None:
        dlogits = torch.empty_like(logits)
    check(_L().dfd_ce_loss_w(_p(logits), _p(targets), int(soft), N, J, label_smoothing, focal_gamma, _p(class_weight), grad_scale,
                             _p(denom), _p(row_loss), _p(loss), _p(dlogits), _stream()), "dfd_ce_loss_w")
    return loss, dlogits


def softmax_argmax(logits: torch.Tensor, want_probs: bool = True):
    N, J = logits.shape
    probs = torch.empty_like(logits) if want_probs else None
    preds = torch.empty(N, dtype=torch.int64, device=logits.device)
    check(_L().dfd_softmax_argmax(_p(logits), N, J, _p(probs), _p(preds), _stream()), "dfd_softmax_argmax")
    return probs, preds


# ------------------------------------------------------------------ evaluation metrics (ABI 146, csrc/dfd_metrics.hip)
ROC_TILE, ROC_SCAN_WIDTH = _lib.ROC_TILE, _lib.ROC_SCAN_WIDTH
ROC_MAX_N, ROC_MAX_CUTS, ROC_STATS_LEN = _lib.ROC_MAX_N, _lib.ROC_MAX_CUTS, _lib.ROC_STATS_LEN
CONFUSION_LDS_MAX_J, CONFUSION_MAX_J = _lib.CONFUSION_LDS_MAX_J, _lib.CONFUSION_MAX_J


# What the evaluation front ends (from here to group pooling) share
def _ws(op: str, ws: torch.Tensor | None, need: int, device, align: int = 1, least: int | None = None) -> torch.Tensor:
    """The caller's workspace if it is a uint8 tensor of at least `least` bytes (default: `need`) on `device` at an address that
    is a multiple of `align`, or a new one of `need` bytes rounded up to whole 8-byte words."""
    if ws is None:
        return torch.empty((need + 7) // 8, dtype=torch.float64, device=device).view(torch.uint8)
    least = need if least is None else least
    if ws.dtype != torch.uint8 or ws.numel() < least or ws.device != device or ws.data_ptr() % align:
        raise ValueError(f"{op}: ws must be a uint8 tensor of at least {least} bytes on {device}, its address a multiple of {align}")
    return ws


def _plan(cls, name: str, *args):
    """A four-int planner of the library (host code) -> its answer as `cls`."""
    out = (ctypes.c_int * 4)()
    check(getattr(_L(), name)(*map(int, args), out), name, f"args={args}")
    return cls(*out)


def _outs(out, count: int):
    """The `out=` destinations of a front end with `count` results: the caller's, or None for each."""
    return out if out is not None else (None,) * count


def _ptrs(tensors):
    """The array of the members' addresses, every one through the gate."""
    return (ctypes.c_void_p * len(tensors))(*[_p(t) for t in tensors])


def roc_ws(n: int) -> int:
    """Bytes of workspace roc_curve needs for n scores."""
    if not 0 <= n <= ROC_MAX_N:
        raise ValueError(f"roc_curve takes 0..{ROC_MAX_N} scores, got {n}")
    return _L().dfd_roc_ws(n)


def roc_curve(scores: torch.Tensor, labels: torch.Tensor, positive: int = 1, ws: torch.Tensor | None = None, out=None):
    """f32 [n] scores sorted ascending and their int64 labels in the same order -> (thr f32 [n], cum_pos int64 [n], cum_neg
    int64 [n], stats int64 [ROC_STATS_LEN] = P, N, G, nonfinite, two_u): the ROC curve by tie group, compacted to the first G
    entries (the rest is not written), and twice the Mann-Whitney U (include/dfd_hip.h).  Four launches, no host sync: G is read
    by whoever reads `stats`.  `ws`: at least roc_ws(n) bytes of uint8 scratch; `out`: the four destinations."""
    if scores.dim() != 1 or scores.dtype != torch.float32 or labels.shape != scores.shape or labels.dtype != torch.int64:
        raise ValueError("roc_curve: expected f32 [n] scores and int64 [n] labels")
    n, device = scores.numel(), scores.device
    ws = _ws("roc_curve", ws, roc_ws(n), device)
    o_thr, o_pos, o_neg, o_stats = _outs(out, 4)
    thr = _dst(o_thr, (n,), device)
    cum_pos = _dst(o_pos, (n,), device, torch.int64)
    cum_neg = _dst(o_neg, (n,), device, torch.int64)
    stats = _dst(o_stats, (ROC_STATS_LEN,), device, torch.int64)
    check(_L().dfd_roc_curve(_p(scores), _p(labels), n, int(positive), _p(ws), ws.numel(), _p(thr), _p(cum_pos), _p(cum_neg),
                             _p(stats), _stream()), "dfd_roc_curve", f"n={n}")
    return thr, cum_pos, cum_neg, stats


def roc_sweep(thr: torch.Tensor, cum_pos: torch.Tensor, cum_neg: torch.Tensor, stats: torch.Tensor, cuts: torch.Tensor, out=None):
    """roc_curve's outputs + T <= ROC_MAX_CUTS ascending f64 cut points on the device -> (tp, fp) int64 [T]: the positives /
    negatives with score >= cut, compared in f64.  One launch; G, P and N are read from `stats` on the device."""
    if cuts.dim() != 1 or cuts.dtype != torch.float64 or not 1 <= cuts.numel() <= ROC_MAX_CUTS:
        raise ValueError(f"roc_sweep: expected 1..{ROC_MAX_CUTS} f64 cut points")
    if thr.dtype != torch.float32 or cum_pos.dtype != torch.int64 or cum_neg.dtype != torch.int64 or stats.dtype != torch.int64 \
            or cum_pos.numel() != thr.numel() or cum_neg.numel() != thr.numel() or stats.numel() != ROC_STATS_LEN:
        raise ValueError("roc_sweep: expected roc_curve's (thr, cum_pos, cum_neg, stats)")
    T, device = cuts.numel(), cuts.device
    o_tp, o_fp = _outs(out, 2)
    tp = _dst(o_tp, (T,), device, torch.int64)
    fp = _dst(o_fp, (T,), device, torch.int64)
    check(_L().dfd_roc_sweep(_p(thr), _p(cum_pos), _p(cum_neg), _p(stats), thr.numel(), _p(cuts), T, _p(tp), _p(fp), _stream()),
          "dfd_roc_sweep", f"T={T}")
    return tp, fp


def confusion_counts(truth: torch.Tensor, pred: torch.Tensor, num_classes: int, out=None):
    """int64 [n] truth and predictions -> (counts int64 [J, J] with row = truth and column = prediction, oob int64 [1] = the
    pairs with a label outside [0, J), which the matrix leaves out).  J <= CONFUSION_LDS_MAX_J counts in LDS, above that (up to
    CONFUSION_MAX_J) with global integer adds."""
    J = int(num_classes)
    if not 1 <= J <= CONFUSION_MAX_J:
        raise ValueError(f"confusion_counts: num_classes must be 1..{CONFUSION_MAX_J}, got {J}")
    if truth.dim() != 1 or truth.dtype != torch.int64 or pred.shape != truth.shape or pred.dtype != torch.int64:
        raise ValueError("confusion_counts: expected int64 [n] truth and predictions")
    n, device = truth.numel(), truth.device
    if n >= 1 << 31:
        raise ValueError("confusion_counts: at most 2^31 - 1 samples")
    o_counts, o_oob = _outs(out, 2)
    counts = _dst(o_counts, (J, J), device, torch.int64)
    oob = _dst(o_oob, (1,), device, torch.int64)
    check(_L().dfd_confusion(_p(truth), _p(pred), n, J, _p(counts), _p(oob), _stream()), "dfd_confusion", f"n={n} J={J}")
    return counts, oob


# ------------------------------------------------------------------ calibration (ABI 150, csrc/dfd_calib.hip)
CALIB_MAX_N, CALIB_MAX_J, CALIB_MAX_BINS, CALIB_MAX_BETAS = _lib.CALIB_MAX_N, _lib.CALIB_MAX_J, _lib.CALIB_MAX_BINS, _lib.CALIB_MAX_BETAS
CALIB_THREAD_MAX_J, CALIB_MAX_BLOCKS, CALIB_STAGE2_WIDTH = _lib.CALIB_THREAD_MAX_J, _lib.CALIB_MAX_BLOCKS, _lib.CALIB_STAGE2_WIDTH
CALIB_LAYOUT_THREAD, CALIB_LAYOUT_WAVE = _lib.CALIB_LAYOUT_THREAD, _lib.CALIB_LAYOUT_WAVE


@dataclass(frozen=True)
class RowPlan:
    """dfd_calib_plan's and dfd_fuse_plan's answer (csrc/dfd_rowred.h): the row layout, the rows a workgroup takes per trip, the
    stage-1 workgroups and the trips of the stage-2 loop."""

    layout: int
    rows: int
    blocks: int
    trips: int


CalibPlan = FusePlan = RowPlan


def _calib_shape(op: str, n: int, J: int, K: int | None = None) -> None:
    if not 0 <= n <= CALIB_MAX_N or not 1 <= J <= CALIB_MAX_J:
        raise ValueError(f"{op}: takes 0..{CALIB_MAX_N} rows of 1..{CALIB_MAX_J} classes, got [{n}, {J}]")
    if K is not None and not 1 <= K <= CALIB_MAX_BETAS:
        raise ValueError(f"{op}: takes 1..{CALIB_MAX_BETAS} betas, got {K}")


def _calib_rows(op: str, rows: torch.Tensor, targets: torch.Tensor) -> tuple[int, int]:
    if rows.dim() != 2 or rows.dtype != torch.float32 or targets.dtype != torch.int64 or tuple(targets.shape) != (rows.shape[0],):
        raise ValueError(f"{op}: expected f32 [n, J] rows and int64 [n] targets, got {rows.dtype} {tuple(rows.shape)} and "
                         f"{targets.dtype} {tuple(targets.shape)}")
    _calib_shape(op, *rows.shape)
    return rows.shape


def calib_bins_ws(n: int, J: int) -> int:
    """Bytes of workspace calib_bins needs for n rows of J classes."""
    _calib_shape("calib_bins", n, J)
    return _L().dfd_calib_bins_ws(n, J)


def calib_nll_ws(n: int, J: int, K: int) -> int:
    """Bytes of workspace calib_nll needs for n rows of J classes at K betas; it covers calib_bins_ws(n, J) too."""
    _calib_shape("calib_nll", n, J, K)
    return _L().dfd_calib_nll_ws(n, J, K)


def calib_plan(n: int, J: int) -> RowPlan:
    """Which layout and launch shape calib_bins / calib_nll use for n rows of J classes (host code)."""
    return _plan(RowPlan, "dfd_calib_plan", n, J)


def calib_bins(probs: torch.Tensor, targets: torch.Tensor, bins: int = 15, ws: torch.Tensor | None = None, out=None):
    """f32 [n, J] probabilities and int64 [n] targets -> (bins int64 [M, 3] = rows / right predictions / sum of llrint(conf 2^32)
    per confidence bin, stats int64 [4] = valid / nonfinite / out-of-range / right rows, brier f64 [1] = the summed squared
    error of the valid rows): include/dfd_hip.h.  Three launches, no host sync.  `ws`: uint8 scratch of calib_bins_ws bytes."""
    n, J = _calib_rows("calib_bins", probs, targets)
    M = int(bins)
    if not 1 <= M <= CALIB_MAX_BINS:
        raise ValueError(f"calib_bins: bins must be 1..{CALIB_MAX_BINS}, got {M}")
    device = probs.device
    ws = _ws("calib_bins", ws, calib_bins_ws(n, J), device, align=8)          # f64 partials
    o_bins, o_stats, o_brier = _outs(out, 3)
    table = _dst(o_bins, (M, 3), device, torch.int64)
    stats = _dst(o_stats, (4,), device, torch.int64)
    brier = _dst(o_brier, (1,), device, torch.float64)
    check(_L().dfd_calib_bins(_p(probs), _p(targets), n, J, M, _p(ws), ws.numel(), _p(table), _p(stats), _p(brier), _stream()),
          "dfd_calib_bins", f"n={n} J={J} M={M}")
    return table, stats, brier


def calib_nll(logits: torch.Tensor, targets: torch.Tensor, betas, ws: torch.Tensor | None = None, out=None):
    """f32 [n, J] logits, int64 [n] targets and K <= CALIB_MAX_BETAS host floats beta = 1 / T (finite, > 0) -> (out f64 [K, 3] =
    the summed negative log-likelihood of softmax(beta z) and its first and second derivative in beta, stats int64 [2] =
    nonfinite / out-of-range rows, which the sums leave out): include/dfd_hip.h.  One pass over the logits for all K; two
    launches, no host sync.  The betas travel by value in the launch."""
    n, J = _calib_rows("calib_nll", logits, targets)
    values = [float(b) for b in betas]
    K = len(values)
    if not 1 <= K <= CALIB_MAX_BETAS or not all(math.isfinite(b) and b > 0.0 for b in values):
        raise ValueError(f"calib_nll: expected 1..{CALIB_MAX_BETAS} finite betas > 0, got {values}")
    device = logits.device
    ws = _ws("calib_nll", ws, calib_nll_ws(n, J, K), device, align=8)         # f64 and int64 partials
    o_out, o_stats = _outs(out, 2)
    sums = _dst(o_out, (K, 3), device, torch.float64)
    stats = _dst(o_stats, (2,), device, torch.int64)
    check(_L().dfd_calib_nll(_p(logits), _p(targets), n, J, (ctypes.c_double * K)(*values), K, _p(ws), ws.numel(), _p(sums), _p(stats),
                             _stream()), "dfd_calib_nll", f"n={n} J={J} K={K}")
    return sums, stats


def softmax_argmax_t(logits: torch.Tensor, inv_temperature: float, want_probs: bool = True):
    """softmax_argmax of inv_temperature * logits (f32 [N, J]); inv_temperature finite and > 0.  At 1.0 the same bits."""
    beta = float(inv_temperature)
    if not (math.isfinite(beta) and beta > 0.0):
        raise ValueError(f"softmax_argmax_t: inv_temperature must be finite and > 0, got {inv_temperature!r}")
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"softmax_argmax_t: logits must be f32 [N, J], got {logits.dtype} {tuple(logits.shape)}")
    N, J = logits.shape
    probs = torch.empty_like(logits) if want_probs else None
    preds = torch.empty(N, dtype=torch.int64, device=logits.device)
    check(_L().dfd_softmax_argmax_t(_p(logits), N, J, beta, _p(probs), _p(preds), _stream()), "dfd_softmax_argmax_t")
    return probs, preds


# ------------------------------------------------------------------ the ensemble (ABI 151, csrc/dfd_fuse.hip)
FUSE_MAX_MODELS, FUSE_MAX_CANDS, FUSE_MAX_J, FUSE_MAX_N = _lib.FUSE_MAX_MODELS, _lib.FUSE_MAX_CANDS, _lib.FUSE_MAX_J, _lib.FUSE_MAX_N
FUSE_THREAD_MAX_KJ, FUSE_MAX_BLOCKS, FUSE_STAGE2_WIDTH = _lib.FUSE_THREAD_MAX_KJ, _lib.FUSE_MAX_BLOCKS, _lib.FUSE_STAGE2_WIDTH
FUSE_LAYOUT_THREAD, FUSE_LAYOUT_WAVE, FUSE_LOGIT, FUSE_PROB = _lib.FUSE_LAYOUT_THREAD, _lib.FUSE_LAYOUT_WAVE, _lib.FUSE_LOGIT, _lib.FUSE_PROB


def fuse_terms(K: int) -> int:
    """The f64 results per candidate of fuse_nll: the NLL, K gradient entries and the upper triangle of the Hessian."""
    return 1 + K + K * (K + 1) // 2


def _fuse_shape(op: str, n: int, J: int, K: int, C: int = 1) -> None:
    if not 0 <= n <= FUSE_MAX_N or not 1 <= J <= FUSE_MAX_J or not 1 <= K <= FUSE_MAX_MODELS or not 1 <= C <= FUSE_MAX_CANDS:
        raise ValueError(f"{op}: takes 0..{FUSE_MAX_N} rows of 1..{FUSE_MAX_J} classes from 1..{FUSE_MAX_MODELS} members at "
                         f"1..{FUSE_MAX_CANDS} candidates, got [{n}, {J}], {K}, {C}")


def _fuse_members(op: str, members, dtype: torch.dtype, dim: int):
    """The K buffers of one shape, dtype and device -> (the list, the array of their addresses through the gate)."""
    members = list(members)
    K = len(members)
    if not 1 <= K <= FUSE_MAX_MODELS:
        raise ValueError(f"{op}: takes 1..{FUSE_MAX_MODELS} members, got {K}")
    first = members[0]
    for m in members:
        if m.dim() != dim or m.dtype != dtype or m.shape != first.shape or m.device != first.device:
            raise ValueError(f"{op}: every member must be {dtype} with {dim} dimensions, one shape and one device, got "
                             f"{[(m.dtype, tuple(m.shape)) for m in members]}")
    _fuse_shape(op, first.shape[0], first.shape[1] if dim == 2 else 1, K)
    return members, _ptrs(members)


def _fuse_targets(op: str, targets: torch.Tensor, n: int) -> None:
    if targets.dtype != torch.int64 or tuple(targets.shape) != (n,):
        raise ValueError(f"{op}: expected int64 [{n}] targets, got {targets.dtype} {tuple(targets.shape)}")


def fuse_plan(n: int, J: int, K: int) -> RowPlan:
    """Which layout and launch shape fuse_scores / fuse_nll use for n rows of J classes from K members (host code)."""
    return _plan(RowPlan, "dfd_fuse_plan", n, J, K)


def fuse_nll_ws(n: int, J: int, K: int, C: int) -> int:
    """Bytes of workspace fuse_nll needs for n rows of J classes from K members at C candidates."""
    _fuse_shape("fuse_nll", n, J, K, C)
    return _L().dfd_fuse_nll_ws(n, J, K, C)


def fuse_scores(logits_list, coef, mode: int = FUSE_LOGIT, beta=None, want_probs: bool = True, want_logits: bool = True, out=None):
    """K f32 [n, J] logit buffers, K host coefficients (and, in FUSE_PROB mode, K inverse temperatures beta > 0) -> (probs f32
    [n, J] or None, preds int64 [n], fused logits f32 [n, J] or None, stats int64 [1] = rows with a non-finite logit, which
    hold NaN and pred 0): include/dfd_hip.h.  FUSE_LOGIT: softmax(sum_k coef_k z_k); FUSE_PROB: sum_k coef_k softmax(beta_k z_k),
    coef_k >= 0 summing to 1.  f64 arithmetic, rounded once on store; two launches, no host sync.  `out`: (probs, preds, logits,
    stats) destinations, a None among the first three taken by want_probs / want_logits."""
    members, ptrs = _fuse_members("fuse_scores", logits_list, torch.float32, 2)
    K = len(members)
    n, J = members[0].shape
    values = [float(c) for c in coef]
    betas = [1.0] * K if beta is None else [float(b) for b in beta]
    if mode not in (FUSE_LOGIT, FUSE_PROB) or len(values) != K or len(betas) != K or not all(math.isfinite(v) for v in values + betas):
        raise ValueError(f"fuse_scores: expected mode 0 or 1 and {K} finite coefficients (and betas), got {mode}, {values}, {betas}")
    if mode == FUSE_PROB and (min(values) < 0.0 or abs(math.fsum(values) - 1.0) > 1e-12 or min(betas) <= 0.0):
        raise ValueError(f"fuse_scores: the probability pool takes coefficients >= 0 that sum to 1 and betas > 0, got {values}, {betas}")
    device = members[0].device
    o_probs, o_preds, o_logits, o_stats = _outs(out, 4)
    probs = _dst(o_probs, (n, J), device) if want_probs or o_probs is not None else None
    fused = _dst(o_logits, (n, J), device) if want_logits or o_logits is not None else None
    preds = _dst(o_preds, (n,), device, torch.int64)
    stats = _dst(o_stats, (1,), device, torch.int64)
    check(_L().dfd_fuse_scores(ptrs, K, n, J, mode, (ctypes.c_double * K)(*values), (ctypes.c_double * K)(*betas), _p(probs), _p(fused),
                               _p(preds), _p(stats), _stream()), "dfd_fuse_scores", f"n={n} J={J} K={K} mode={mode}")
    return probs, preds, fused, stats


def fuse_nll(logits_list, targets: torch.Tensor, cands, ws: torch.Tensor | None = None, out=None):
    """K f32 [n, J] logit buffers, int64 [n] targets and C <= FUSE_MAX_CANDS host coefficient vectors of length K -> (out f64
    [C, fuse_terms(K)] = per candidate the summed NLL of softmax(sum_k a_k z_k), its gradient in a and the upper triangle of its
    Hessian, row by row, stats int64 [2] = nonfinite / out-of-range rows, which the sums leave out): include/dfd_hip.h.  Two
    launches, no host sync.  The addresses and the candidates travel by value in the launch."""
    members, ptrs = _fuse_members("fuse_nll", logits_list, torch.float32, 2)
    K = len(members)
    n, J = members[0].shape
    _fuse_targets("fuse_nll", targets, n)
    rows = [[float(v) for v in cand] for cand in cands]
    C = len(rows)
    if not 1 <= C <= FUSE_MAX_CANDS or any(len(r) != K or not all(math.isfinite(v) for v in r) for r in rows):
        raise ValueError(f"fuse_nll: expected 1..{FUSE_MAX_CANDS} candidates of {K} finite coefficients, got {rows}")
    device = members[0].device
    ws = _ws("fuse_nll", ws, fuse_nll_ws(n, J, K, C), device, align=8)        # f64 and int64 partials
    o_out, o_stats = _outs(out, 2)
    sums = _dst(o_out, (C, fuse_terms(K)), device, torch.float64)
    stats = _dst(o_stats, (2,), device, torch.int64)
    flat = [v for r in rows for v in r]
    check(_L().dfd_fuse_nll(ptrs, K, _p(targets), n, J, (ctypes.c_double * len(flat))(*flat), C, _p(ws), ws.numel(), _p(sums), _p(stats),
                            _stream()), "dfd_fuse_nll", f"n={n} J={J} K={K} C={C}")
    return sums, stats


def fuse_agree(preds_list, targets: torch.Tensor, num_classes: int, out=None):
    """K int64 [n] prediction buffers and int64 [n] targets -> (pair int64 [K, K, 4] = rows where members (a, b) are both right /
    a right and b wrong / a wrong and b right / both wrong, hist int64 [K + 1] = rows by the number of members that are right,
    stats int64 [2] = valid rows / rows whose target is outside [0, num_classes)).  Integers only; two launches, no host sync."""
    members, ptrs = _fuse_members("fuse_agree", preds_list, torch.int64, 1)
    K, n, J = len(members), members[0].shape[0], int(num_classes)
    _fuse_targets("fuse_agree", targets, n)
    _fuse_shape("fuse_agree", n, J, K)
    device = members[0].device
    o_pair, o_hist, o_stats = _outs(out, 3)
    pair = _dst(o_pair, (K, K, 4), device, torch.int64)
    hist = _dst(o_hist, (K + 1,), device, torch.int64)
    stats = _dst(o_stats, (2,), device, torch.int64)
    check(_L().dfd_fuse_agree(ptrs, K, _p(targets), n, J, _p(pair), _p(hist), _p(stats), _stream()), "dfd_fuse_agree", f"n={n} J={J} K={K}")
    return pair, hist, stats


# ------------------------------------------------------------------ the bootstrap (ABI 153, csrc/dfd_boot.hip)
BOOT_STREAM, BOOT_MAX_N, BOOT_MAX_REPLICATES, BOOT_MAX_MEMBERS = _lib.BOOT_STREAM, _lib.BOOT_MAX_N, _lib.BOOT_MAX_REPLICATES, _lib.BOOT_MAX_MEMBERS
BOOT_STATS_LEN, BOOT_LDS_MAX_N, BOOT_DRAW_TILE = _lib.BOOT_STATS_LEN, _lib.BOOT_LDS_MAX_N, _lib.BOOT_DRAW_TILE
BOOT_TIER_LDS, BOOT_TIER_GLOBAL = _lib.BOOT_TIER_LDS, _lib.BOOT_TIER_GLOBAL
(BOOT_P, BOOT_N, BOOT_TWO_U, BOOT_TP, BOOT_FP, BOOT_HITS, BOOT_F0, BOOT_T0, BOOT_F1, BOOT_T1) = range(BOOT_STATS_LEN)
BOOT_WS_CAP = 1 << 30               # the largest workspace boot_stats allocates by itself: more resamples mean more passes


@dataclass(frozen=True)
class BootPlan:
    """dfd_boot_plan's answer: the tier, the resamples per pass, the passes and the draw tiles per resample."""

    tier: int
    per_pass: int
    passes: int
    draw_tiles: int


def _boot_shape(op: str, n: int, B: int, M: int = 1) -> None:
    if not 0 <= n <= BOOT_MAX_N or not 1 <= B <= BOOT_MAX_REPLICATES or not 1 <= M <= BOOT_MAX_MEMBERS:
        raise ValueError(f"{op}: takes 0..{BOOT_MAX_N} samples, 1..{BOOT_MAX_REPLICATES} resamples and 1..{BOOT_MAX_MEMBERS} members, "
                         f"got {n}, {B}, {M}")


def _boot_seed(op: str, seed: int) -> int:
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{op}: the seed is an unsigned 64-bit integer, got {seed}")
    return seed


def boot_ws(n: int, B: int) -> int:
    """Bytes of workspace with which boot_stats runs B resamples of n samples in one pass (0 in the LDS tier)."""
    _boot_shape("boot_ws", n, B)
    return _L().dfd_boot_ws(int(n), int(B))


def boot_plan(n: int, B: int, M: int = 1, ws_bytes: int | None = None) -> BootPlan:
    """Which tier boot_stats runs for B resamples of n samples from M members in a workspace of ws_bytes (default: what boot_stats
    allocates by itself), and in how many passes (host code)."""
    _boot_shape("boot_plan", n, B, M)
    if ws_bytes is None:
        ws_bytes = _boot_default_ws(boot_ws(n, B), n)
    return _plan(BootPlan, "dfd_boot_plan", n, B, M, ws_bytes)


def _boot_default_ws(need: int, count: int) -> int:
    """The workspace boot_stats takes by itself when one pass needs `need` bytes for `count` counts per resample: all of it, or
    the whole resamples that fit in BOOT_WS_CAP."""
    return need if need <= BOOT_WS_CAP else max(BOOT_WS_CAP // (4 * count), 1) * 4 * count


def boot_counts(n: int, b0: int, R: int, seed: int, device, out: torch.Tensor | None = None) -> torch.Tensor:
    """int32 [R, n] (the bits of the kernel's uint32): how often each of n samples is drawn in resamples b0 .. b0 + R - 1 under
    `seed` (the resampling rule of include/dfd_hip.h), by the global tier's zero and draw launches."""
    n, b0, R = int(n), int(b0), int(R)
    if not 0 <= n <= BOOT_MAX_N or b0 < 0 or R < 1 or b0 + R > BOOT_MAX_REPLICATES:
        raise ValueError(f"boot_counts: takes 0..{BOOT_MAX_N} samples and resamples inside 0..{BOOT_MAX_REPLICATES}, got {n}, {b0}, {R}")
    counts = _dst(out, (R, n), torch.device(device), torch.int32)
    check(_L().dfd_boot_counts(n, b0, R, _boot_seed("boot_counts", seed), _p(counts), _stream()), "dfd_boot_counts", f"n={n} b0={b0} R={R}")
    return counts


def _boot_inputs(op: str, sorted_scores, perms, is_positive: torch.Tensor, hit, cuts, groups: torch.Tensor | None = None):
    """What boot_stats and boot_stats_grouped check alike -> (the members, their permutations, one cut or NaN per member)."""
    members, perm_list = list(sorted_scores), list(perms)
    M = len(members)
    if not 1 <= M <= BOOT_MAX_MEMBERS or len(perm_list) != M:
        raise ValueError(f"{op}: takes 1..{BOOT_MAX_MEMBERS} members with one permutation each, got {M} and {len(perm_list)}")
    n, device = members[0].numel(), members[0].device
    for many, dtype in ((members, torch.float32), (perm_list, torch.int32), ([groups] if groups is not None else [], torch.int32)):
        for t in many:
            if t.dtype != dtype or tuple(t.shape) != (n,) or t.device != device:
                raise ValueError(f"{op}: expected f32 [{n}] scores and int32 [{n}] permutations (and group ids) on {device}, got {t.dtype} "
                                 f"{tuple(t.shape)}")
    for name, t in (("is_positive", is_positive), ("hit", hit)):
        if t is not None and (t.dtype != torch.uint8 or tuple(t.shape) != (n,) or t.device != device):
            raise ValueError(f"{op}: {name} must be uint8 [{n}] on {device}, got {t.dtype} {tuple(t.shape)}")
    values = [float("nan")] * M if cuts is None else [float("nan") if c is None else float(c) for c in cuts]
    if len(values) != M:
        raise ValueError(f"{op}: {M} members need {M} cuts, got {len(values)}")
    return members, perm_list, values


def boot_stats(sorted_scores, perms, is_positive: torch.Tensor, replicates: int, seed: int = 0, cuts=None, hit: torch.Tensor | None = None,
               ws: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """M members' f32 [n] scores sorted ascending and the int32 [n] permutations that sorted them, uint8 [n] is_positive (and
    optionally uint8 [n] hit) in sample order -> int64 [M, B, BOOT_STATS_LEN] = P, N, two_u, tp, fp, hits, f0, t0, f1, t1 of
    every bootstrap resample (include/dfd_hip.h).  cuts: one float or None per member (None: no cut).  `ws`: uint8 scratch for the
    global tier, at least 4 n bytes (one resample per pass); by default boot_ws(n, B) bytes capped at BOOT_WS_CAP.  No host sync."""
    return _boot_stats("boot_stats", sorted_scores, perms, is_positive, replicates, seed, cuts, hit, ws, out)


def _boot_stats(op: str, sorted_scores, perms, is_positive, replicates, seed, cuts, hit, ws, out, grouped=None):
    """The body of boot_stats (a resample holds n counts) and of boot_stats_grouped (grouped = (groups, G, max_size): G counts)."""
    groups, G, max_size = grouped or (None, 0, 0)
    members, perm_list, values = _boot_inputs(op, sorted_scores, perms, is_positive, hit, cuts, groups)
    M, B, n, device = len(members), int(replicates), members[0].numel(), members[0].device
    if grouped is None:
        _boot_shape(op, n, B, M)
        count, need = n, boot_ws(n, B)
    else:
        _boot_grouped_shape(op, n, G, max_size, B, M)
        count, need = G, boot_ws_grouped(n, G, B)
    seed = _boot_seed(op, seed)
    # only the global tier reads the workspace: one resample's counts at least
    ws = _ws(op, ws, _boot_default_ws(need, count), device, least=4 * count if count > BOOT_LDS_MAX_N else 0)
    stats = _dst(out, (M, B, BOOT_STATS_LEN), device, torch.int64)
    shape = (n,) if grouped is None else (_p(groups), n, G, max_size)
    check(getattr(_L(), "dfd_" + op)(_ptrs(members), _ptrs(perm_list), M, _p(is_positive), _p(hit), (ctypes.c_double * M)(*values),
                                     *shape, B, seed, _p(ws) if ws.numel() else None, ws.numel(), _p(stats), _stream()),
          "dfd_" + op, f"n={n} B={B} M={M}" + (f" G={G} max_size={max_size}" if grouped else ""))
    return stats


# ------------------------------------------------------------------ the cluster bootstrap (ABI 154, csrc/dfd_boot.hip)
BOOT_GROUPED_MAX_WEIGHT = _lib.BOOT_GROUPED_MAX_WEIGHT


def _boot_grouped_shape(op: str, n: int, G: int, max_size: int, B: int, M: int = 1) -> None:
    _boot_shape(op, n, B, M)
    if not 1 <= G <= n or not 1 <= max_size <= n or G * max_size > BOOT_GROUPED_MAX_WEIGHT:
        raise ValueError(f"{op}: takes 1..n groups of at most max_size <= n samples with groups * max_size <= {BOOT_GROUPED_MAX_WEIGHT}, "
                         f"got n={n}, groups={G}, max_size={max_size}")


def boot_ws_grouped(n: int, num_groups: int, B: int) -> int:
    """Bytes of workspace with which boot_stats_grouped runs B resamples of num_groups groups in one pass (0 in the LDS tier)."""
    _boot_grouped_shape("boot_ws_grouped", n, num_groups, 1, B)
    return _L().dfd_boot_ws_grouped(int(n), int(num_groups), int(B))


def boot_plan_grouped(n: int, num_groups: int, max_size: int, B: int, M: int = 1, ws_bytes: int | None = None) -> BootPlan:
    """boot_plan of the cluster bootstrap: the tier boundary is on num_groups (host code)."""
    n, G, max_size = int(n), int(num_groups), int(max_size)
    _boot_grouped_shape("boot_plan_grouped", n, G, max_size, B, M)
    if ws_bytes is None:
        ws_bytes = _boot_default_ws(boot_ws_grouped(n, G, B), G)
    return _plan(BootPlan, "dfd_boot_plan_grouped", n, G, max_size, B, M, ws_bytes)


def boot_stats_grouped(sorted_scores, perms, is_positive: torch.Tensor, groups: torch.Tensor, num_groups: int, max_size: int,
                       replicates: int, seed: int = 0, cuts=None, hit: torch.Tensor | None = None, ws: torch.Tensor | None = None,
                       out: torch.Tensor | None = None) -> torch.Tensor:
    """boot_stats of the cluster bootstrap (include/dfd_hip.h): a resample draws num_groups whole groups, and sample i counts as
    often as its group groups[i] (int32 [n], sample order; an id outside [0, num_groups) counts for nothing) was drawn.  max_size:
    the caller's bound on the largest group; num_groups * max_size <= BOOT_GROUPED_MAX_WEIGHT.  `ws`: uint8 scratch for the global
    tier (num_groups > BOOT_LDS_MAX_N), at least 4 num_groups bytes.  No host sync."""
    return _boot_stats("boot_stats_grouped", sorted_scores, perms, is_positive, replicates, seed, cuts, hit, ws, out,
                       (groups, int(num_groups), int(max_size)))


# ------------------------------------------------------------------ group pooling (ABI 154, csrc/dfd_group.hip)
GROUP_MEAN, GROUP_VOTE, GROUP_MAX = _lib.GROUP_MEAN, _lib.GROUP_VOTE, _lib.GROUP_MAX
GROUP_MAX_N, GROUP_MAX_J, GROUP_LDS_BYTES = _lib.GROUP_MAX_N, _lib.GROUP_MAX_J, _lib.GROUP_LDS_BYTES
GROUP_TIER_LDS, GROUP_TIER_GLOBAL = _lib.GROUP_TIER_LDS, _lib.GROUP_TIER_GLOBAL
(GROUP_INVALID, GROUP_OOB, GROUP_MIXED, GROUP_EMPTY) = range(4)


@dataclass(frozen=True)
class GroupPlan:
    """dfd_group_plan's answer: the tier, the accumulate workgroups, the LDS bytes of each (0 in the global tier) and the finish
    workgroups."""

    tier: int
    workgroups: int
    lds_bytes: int
    finish_workgroups: int


def _group_shape(op: str, n: int, G: int, J: int) -> None:
    if not 1 <= G <= n <= GROUP_MAX_N or not 1 <= J <= GROUP_MAX_J:
        raise ValueError(f"{op}: takes 1 <= groups <= rows <= {GROUP_MAX_N} and 1..{GROUP_MAX_J} classes, got rows={n}, groups={G}, J={J}")


def group_ws(n: int, num_groups: int, J: int) -> int:
    """Bytes of workspace group_pool needs."""
    _group_shape("group_ws", n, num_groups, J)
    return _L().dfd_group_ws(int(n), int(num_groups), int(J))


def group_plan(n: int, num_groups: int, J: int) -> GroupPlan:
    """Which tier group_pool runs for n rows of J classes in num_groups groups, and its launch shape (host code)."""
    _group_shape("group_plan", n, num_groups, J)
    return _plan(GroupPlan, "dfd_group_plan", n, num_groups, J)


def group_pool(probs: torch.Tensor, groups: torch.Tensor, targets: torch.Tensor, num_groups: int, mode: int = GROUP_MEAN,
               positive: int = 1, ws: torch.Tensor | None = None, out=None):
    """f32 [n, J] probabilities, int32 [n] group ids in [0, num_groups) and int64 [n] targets -> (probs f32 [G, J], preds int64 [G],
    targets int64 [G], sizes int32 [G], info int64 [4] = invalid rows / ids out of range / groups with mixed targets / empty
    groups): include/dfd_hip.h.  GROUP_MEAN and GROUP_VOTE sum integers, GROUP_MAX copies the member row with the largest
    probs[:, positive]; the bits do not depend on the order of the rows.  Three launches, no host sync.  `ws`: uint8 scratch of
    group_ws bytes; `out`: the five destinations."""
    if probs.dim() != 2 or probs.dtype != torch.float32 or targets.dtype != torch.int64 or groups.dtype != torch.int32 or \
            tuple(targets.shape) != (probs.shape[0],) or tuple(groups.shape) != (probs.shape[0],):
        raise ValueError(f"group_pool: expected f32 [n, J] rows, int32 [n] groups and int64 [n] targets, got {probs.dtype} "
                         f"{tuple(probs.shape)}, {groups.dtype} {tuple(groups.shape)} and {targets.dtype} {tuple(targets.shape)}")
    n, J = probs.shape
    G, mode, positive = int(num_groups), int(mode), int(positive)
    _group_shape("group_pool", n, G, J)
    if mode not in (GROUP_MEAN, GROUP_VOTE, GROUP_MAX) or not 0 <= positive < J:
        raise ValueError(f"group_pool: mode must be 0..2 and positive a class below {J}, got {mode}, {positive}")
    device = probs.device
    ws = _ws("group_pool", ws, group_ws(n, G, J), device, align=8)      # uint64 cells
    o = _outs(out, 5)
    pooled = _dst(o[0], (G, J), device)
    preds = _dst(o[1], (G,), device, torch.int64)
    tgt = _dst(o[2], (G,), device, torch.int64)
    sizes = _dst(o[3], (G,), device, torch.int32)
    info = _dst(o[4], (4,), device, torch.int64)
    check(_L().dfd_group_pool(_p(probs), _p(groups), _p(targets), n, G, J, mode, positive, _p(ws), ws.numel(), _p(pooled), _p(preds),
                              _p(tgt), _p(sizes), _p(info), _stream()), "dfd_group_pool", f"n={n} G={G} J={J} mode={mode}")
    return pooled, preds, tgt, sizes, info


# ------------------------------------------------------------------ Grad-CAM (ABI 136)
def gradcam_map(act: torch.Tensor, grad: torch.Tensor) -> torch.Tensor:
    """Target-layer activation and its gradient, NHWC [N, h, w, C] (f32 or bf16) -> the ReLU'd Grad-CAM map f32 [N, h, w]:
    max(0, sum_c mean_hw(grad) * act)."""
    if act.dim() != 4 or act.shape != grad.shape or act.dtype != grad.dtype:
        raise ValueError(f"gradcam_map: act {tuple(act.shape)} {act.dtype} and grad {tuple(grad.shape)} {grad.dtype} must be equal NHWC")
    N, h, w, C = act.shape
    cam = torch.empty((N, h, w), dtype=torch.float32, device=act.device)
    check(_L().dfd_gradcam_map(_p(act), _p(grad), _dt(act), N, h * w, C, _p(cam), _stream()), "dfd_gradcam_map",
          f"{tuple(act.shape)}")
    return cam


def cam_render(cam: torch.Tensor, size: tuple[int, int], image: torch.Tensor | None = None, mean_std: torch.Tensor | None = None,
               lut: torch.Tensor | None = None, image_weight: float = 0.5) -> tuple[torch.Tensor, torch.Tensor | None]:
    """Low-resolution map f32 [N, h, w] -> (heatmap f32 [N, H, W], overlay uint8 [N, H, W, 3] or None).  The overlay is drawn
    when `image` (the normalised model input, f32 [N, 3, H, W]), `mean_std` (f32 [6] on the device) and `lut` (uint8 [256, 3])
    are given."""
    N, h, w = cam.shape
    H, W = size
    heat = torch.empty((N, H, W), dtype=torch.float32, device=cam.device)
    overlay = None
    if image is not None:
        if image.dtype != torch.float32 or tuple(image.shape) != (N, 3, H, W):
            raise ValueError(f"cam_render: image must be f32 [{N}, 3, {H}, {W}], got {tuple(image.shape)} {image.dtype}")
        if lut is None or mean_std is None or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3) or mean_std.numel() != 6:
            raise ValueError("cam_render: an overlay needs a uint8 [256, 3] lut and f32 [6] mean_std")
        image = image.contiguous()
        overlay = torch.empty((N, H, W, 3), dtype=torch.uint8, device=cam.device)
    ws_bytes = _L().dfd_cam_render_ws(N, h, w, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=cam.device)
    check(_L().dfd_cam_render(_p(cam), N, h, w, H, W, _p(image), _p(mean_std if image is not None else None),
                              _p(lut if image is not None else None), float(image_weight), _p(heat), _p(overlay), _p(ws), ws_bytes,
                              _stream()), "dfd_cam_render", f"{N}x{h}x{w} -> {H}x{W}")
    return heat, overlay


def adamw_step(table, hp: torch.Tensor) -> None:
    """One dfd_adamw_step launch over an AdamW chunk table (an AddressTable, or the bare device int64 tensor)."""
    check(_L().dfd_adamw_step(*_table(table), _p(hp), _stream()), "dfd_adamw_step")


def grad_sumsq(table, partials: torch.Tensor) -> None:
    """One dfd_grad_sumsq launch over an AdamW chunk table: partials[row] (f64, device) = sum of the squares of the row's gradients."""
    ptr, rows = _table(table)
    if partials.dtype != torch.float64 or partials.numel() < rows:
        raise ValueError("grad_sumsq needs one f64 partial per table row")
    check(_L().dfd_grad_sumsq(ptr, rows, _p(partials), _stream()), "dfd_grad_sumsq")


def grad_clip_finish(partials: torch.Tensor, hp: torch.Tensor, cfg: torch.Tensor, state: torch.Tensor) -> None:
    """One dfd_grad_clip_finish launch: the f64 partials become the norm, the coefficient and the skip flag in `state` (f32,
    CLIP_STATE_LEN); `hp` is the AdamW record (grad_scale), `cfg` = {limit, mode} in device memory."""
    if partials.dtype != torch.float64 or state.numel() != CLIP_STATE_LEN or cfg.numel() != CLIP_CFG_LEN:
        raise ValueError("grad_clip_finish needs f64 partials, a CLIP_CFG_LEN cfg and a CLIP_STATE_LEN state")
    check(_L().dfd_grad_clip_finish(_p(partials), partials.numel(), _p(hp), _p(cfg), _p(state), _stream()), "dfd_grad_clip_finish")


def adamw_step_clip(table, hp: torch.Tensor, cfg: torch.Tensor, state: torch.Tensor) -> None:
    """dfd_adamw_step with the gradient clipped as `cfg` and `state` (written by grad_clip_finish on this stream) say."""
    check(_L().dfd_adamw_step_clip(*_table(table), _p(hp), _p(cfg), _p(state), _stream()), "dfd_adamw_step_clip")


def ema_update(table, w: torch.Tensor) -> None:
    """One dfd_ema_update launch over a device int64 table [nchunks][EMA_TABLE_COLS] (an AddressTable, or the bare tensor);
    `w` is the f32 weight in device memory."""
    check(_L().dfd_ema_update(*_table(table), _p(w), _stream()), "dfd_ema_update")


# ------------------------------------------------------------------ Mixup / CutMix (ABI 138)
def check_mix_jobs(jobs: torch.Tensor, N: int, H: int, W: int) -> None:
    """The host job table int32 [N, MIX_JOB_WORDS] {mode, w0, w1, y0, y1, x0, x1, 0}: known modes, every box inside the
    H x W picture, and the middle sample of an odd N kept."""
    if jobs.is_cuda or jobs.dtype != torch.int32 or tuple(jobs.shape) != (N, MIX_JOB_WORDS):
        raise ValueError(f"mix_batch: the job table must be a host int32 [{N}, {MIX_JOB_WORDS}] tensor, got "
                         f"{jobs.dtype} {tuple(jobs.shape)} on {jobs.device}")
    mode, y0, y1, x0, x1 = (jobs[:, c] for c in (0, 3, 4, 5, 6))
    if bool(((mode < MIX_KEEP) | (mode > MIX_CUTMIX)).any()):
        raise ValueError("mix_batch: unknown mode in the job table")
    bad = (y0 < 0) | (y0 > y1) | (y1 > H) | (x0 < 0) | (x0 > x1) | (x1 > W)
    if bool(bad.any()):
        n = int(bad.nonzero()[0])
        raise ValueError(f"mix_batch: job {n}: box rows [{int(y0[n])}, {int(y1[n])}) columns [{int(x0[n])}, {int(x1[n])}) "
                         f"leaves the {H} x {W} picture")
    if N % 2 == 1 and int(mode[N // 2]) != MIX_KEEP:
        raise ValueError("mix_batch: the middle sample of an odd batch is its own partner and must be kept")


def mix_batch(x: torch.Tensor, labels: torch.Tensor, jobs: torch.Tensor, num_classes: int) -> torch.Tensor:
    """One dfd_mix_batch launch: mixes the f32 batch `x` [N, 3, H, W] (channels_last or contiguous) IN PLACE with the partner
    N - 1 - i of every sample as the HOST job table says, and returns the soft targets f32 [N, num_classes].  The table is
    checked here (check_mix_jobs) and uploaded without blocking when it is pinned.  Host labels are checked against
    [0, num_classes) and uploaded; labels that already live on the device are not read back (a label out of range matches
    no class: its share of the target row is dropped, nothing is written out of bounds)."""
    if not x.is_cuda:
        raise RuntimeError("mix_batch needs the batch on a HIP device (no CPU fallback)")
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
        raise ValueError(f"mix_batch: x must be f32 [N, 3, H, W], got {x.dtype} {tuple(x.shape)}")
    N, _, H, W = x.shape
    if x.is_contiguous():
        layout, flat = MIX_NCHW, x
    elif x.is_contiguous(memory_format=torch.channels_last):
        layout, flat = MIX_NHWC, x.permute(0, 2, 3, 1)
    else:
        raise ValueError(f"mix_batch: x must be dense NCHW or channels_last, got strides {x.stride()}")
    if num_classes < 1 or labels.dtype != torch.int64 or tuple(labels.shape) != (N,):
        raise ValueError(f"mix_batch: labels must be int64 [{N}] and num_classes >= 1, got {labels.dtype} {tuple(labels.shape)}")
    check_mix_jobs(jobs, N, H, W)
    if not labels.is_cuda:
        if bool(((labels < 0) | (labels >= num_classes)).any()):
            raise ValueError(f"mix_batch: a label lies outside [0, {num_classes})")
        labels = labels.to(x.device, non_blocking=True)
    table = jobs.to(x.device, non_blocking=True)
    y = torch.empty((N, num_classes), dtype=torch.float32, device=x.device)
    check(_L().dfd_mix_batch(_p(flat), _p(labels), _p(table), _p(y), N, H, W, num_classes, layout, _stream()), "dfd_mix_batch",
          f"{tuple(x.shape)}")
    return y


# ------------------------------------------------------------------ token-mixer set (ABI 110)
def _rows_c(t: torch.Tensor) -> tuple[int, int]:
    C = t.shape[-1]
    return t.numel() // C, C


def affine2_apply(dz: torch.Tensor, y: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    rows, C = _rows_c(y)
    out = torch.empty_like(y)
    check(_L().dfd_affine2_apply(_dt(y), _p(dz), _p(y), _p(coef), _p(out), rows, C, _stream()), "dfd_affine2_apply")
    return out


def bn_add_act(y: torch.Tensor, state: torch.Tensor | None, other: torch.Tensor | None, act: int) -> torch.Tensor:
    rows, C = _rows_c(y)
    out = torch.empty_like(y)
    check(_L().dfd_bn_add_act(_dt(y), _p(y), _p(state), _p(other), act, _p(out), rows, C, _stream()), "dfd_bn_add_act")
    return out


def bn_add_act_bwd(g: torch.Tensor, y: torch.Tensor, state: torch.Tensor | None, other: torch.Tensor | None, act: int,
                   stats: bool = True):
    rows, C = _rows_c(y)
    d = torch.empty_like(y)
    parts = partials_buf(y.device, C) if (stats and state is not None) else None
    n = ctypes.c_int(0)
    check(_L().dfd_bn_add_act_bwd(_dt(y), _p(g), _p(y), _p(state), _p(other), act, _p(d), rows, C, _p(parts), MAX_PARTIALS,
                                  ctypes.byref(n), _stream()), "dfd_bn_add_act_bwd")
    return d, parts, n.value


def channel_stats(x: torch.Tensor):
    rows, C = _rows_c(x)
    parts = partials_buf(x.device, C)
    n = ctypes.c_int(0)
    check(_L().dfd_channel_stats(_dt(x), _p(x), rows, C, _p(parts), MAX_PARTIALS, ctypes.byref(n), _stream()), "dfd_channel_stats")
    return parts, n.value


def sum_rows(partials: torch.Tensor, P: int, L: int, out: torch.Tensor, accumulate: bool = False, deferred: bool = False) -> torch.Tensor:
    """out[i] = sum_p partials[p][i] in a fixed order; `partials` (flat f32) must hold P + ceil(P/32) rows of L floats
    (the second reduction stage is written behind the slab).  More than 1024 rows are summed in groups of 1024, last
    group first, so that a group's second stage only overwrites rows that have already been consumed.
    deferred: `out` is a gradient-arena slot nobody reads before the end of the enclosing block and `partials` comes from
    scratch(): inside sum_batch() the sum joins the block's batched sums (same order, same bits) instead of two launches here."""
    if partials.numel() < (P + (min(P, 1024) + 31) // 32) * L:
        raise ValueError("sum_rows: partial slab too small for the two-stage reduction")
    if deferred and P <= 1024 and _sum_batch.open:
        check(_L().dfd_sum_rows_deferred(_p(partials), P, L, _p(out), int(accumulate), _stream()), "dfd_sum_rows_deferred")
        return out
    if P <= 1024:
        check(_L().dfd_sum_rows(_p(partials), P, L, _p(out), int(accumulate), _stream()), "dfd_sum_rows")
        return out
    G = (P + 1023) // 1024
    tmp = torch.empty((G + (G + 31) // 32 + 1) * L, dtype=torch.float32, device=partials.device)
    for gi in reversed(range(G)):
        rows = min(1024, P - gi * 1024)
        at = gi * 1024 * L
        check(_L().dfd_sum_rows(_p(partials[at:at + rows * L]), rows, L, _p(tmp[gi * L:(gi + 1) * L]), 0, _stream()), "dfd_sum_rows")
    return sum_rows(tmp, G, L, out, accumulate)


def up2_act_fwd(s: torch.Tensor, act: int) -> torch.Tensor:
    _chk_nhwc(s)
    N, h, w, C = s.shape
    out = torch.empty((N, 2 * h, 2 * w, C), dtype=s.dtype, device=s.device)
    check(_L().dfd_up2_act_fwd(_dt(s), _p(s), act, _p(out), N, h, w, C, _stream()), "dfd_up2_act_fwd")
    return out


def up2_act_bwd(g: torch.Tensor, s: torch.Tensor, act: int) -> torch.Tensor:
    N, h, w, C = s.shape
    ds = torch.empty_like(s)
    ws = torch.empty_like(g) if act != ACT_NONE else None
    check(_L().dfd_up2_act_bwd(_dt(s), _p(g), _p(s), act, _p(ds), N, h, w, C, _p(ws), _stream()), "dfd_up2_act_bwd")
    return ds


def subsample_add(a: torch.Tensor, bias: torch.Tensor | None, x: torch.Tensor, stride: int) -> torch.Tensor:
    N, H, W, C = x.shape
    out = torch.empty_like(a)
    check(_L().dfd_subsample_add(_dt(x), _p(a), _p(bias), _p(x), _p(out), N, H, W, stride, C, _stream()), "dfd_subsample_add")
    return out


def subsample_add_bwd(g: torch.Tensor, dx: torch.Tensor, stride: int) -> torch.Tensor:
    """dx[:, ::stride, ::stride] += g, in place."""
    N, H, W, C = dx.shape
    check(_L().dfd_subsample_add_bwd(_dt(dx), _p(g), _p(dx), N, H, W, stride, C, _stream()), "dfd_subsample_add_bwd")
    return dx


def bgemm(A: torch.Tensor, sa: tuple, B: torch.Tensor, sb: tuple, C: torch.Tensor, sc: tuple, nb: int, nh: int, M: int, N: int,
          Kd: int, alpha: float = 1.0, bias: torch.Tensor | None = None, round_a: bool = False, round_b: bool = False) -> None:
    """C[b,h,m,n] = alpha * sum_k A[b,h,m,k] B[b,h,k,n] (+ bias[h,m,n]); s* = (sb, sh, sr, sc) element strides."""
    ma, mb, mc = _lib.Mat(*sa), _lib.Mat(*sb), _lib.Mat(*sc)
    check(_L().dfd_bgemm(_dt(A), _p(A, strided=True), ctypes.byref(ma), _dt(B), _p(B, strided=True), ctypes.byref(mb),
                         _dt(C), _p(C, strided=True), ctypes.byref(mc), _p(bias), alpha, nb, nh, M, N, Kd, int(round_a),
                         int(round_b), _stream()), "dfd_bgemm", f"nb={nb} nh={nh} M={M} N={N} K={Kd}")


def attn_mfma_supported(dtype: torch.dtype, Nq: int, Nk: int, dk: int, dv: int) -> bool:
    """The one-wave-per-(image, head, 64-token block) attention products (csrc/dfd_attn.hip, dfd_attn_scores / dfd_attn_apply): bf16
    activations, at most 256 tokens on either side, head dimensions that are multiples of 8 up to 128."""
    return dtype == torch.bfloat16 and 1 <= Nq <= 256 and 1 <= Nk <= 256 and all(d % 8 == 0 and 8 <= d <= 128 for d in (dk, dv))


def attn_scores(x: torch.Tensor, y: torch.Tensor, H: int, alpha: float = 1.0, bias: torch.Tensor | None = None) -> torch.Tensor:
    """x [B, .., H*D] (Tx tokens per image), y [B, .., H*D] (Ty tokens) bf16 -> f32 [B, H, Tx, Ty] = alpha * x_h y_h^T (+ bias[H, Tx*Ty])."""
    B = x.shape[0]
    D = x.shape[-1] // H
    Tx, Ty = x.numel() // (B * H * D), y.numel() // (B * H * D)
    out = torch.empty((B, H, Tx, Ty), dtype=torch.float32, device=x.device)
    check(_L().dfd_attn_scores(_p(x), _p(y), _p(out), _p(bias), float(alpha), B, H, Tx, Ty, D, _stream()), "dfd_attn_scores",
          f"B={B} H={H} Tx={Tx} Ty={Ty} D={D}")
    return out


def attn_apply(f: torch.Tensor, x: torch.Tensor, out_shape, H: int, alpha: float = 1.0, transpose: bool = False) -> torch.Tensor:
    """f f32 [B, H, To, Tc] (transpose: [B, H, Tc, To]), x [B, .., H*D] with Tc tokens per image -> bf16 tensor of `out_shape`
    ([B, .., H*D], To tokens): out_h = alpha * f_h x_h (or f_h^T x_h)."""
    B = x.shape[0]
    D = x.shape[-1] // H
    Tc = x.numel() // (B * H * D)
    To = f.shape[3] if transpose else f.shape[2]
    out = torch.empty(tuple(out_shape), dtype=x.dtype, device=x.device)
    check(_L().dfd_attn_apply(_p(f), int(transpose), _p(x), _p(out), float(alpha), B, H, To, Tc, D, _stream()), "dfd_attn_apply",
          f"B={B} H={H} To={To} Tc={Tc} D={D}")
    return out


def wattn_supported(dtype: torch.dtype, T: int, hd: int) -> bool:
    """The fused MFMA window attention (csrc/dfd_attn.hip) covers bf16, head_dim 32, at most 64 tokens per window: FasterViT-0
    under bf16 autocast.  f32, and the head dims 40 / 48 / 64 of FasterViT-1 / -2 / -3, take the batched-GEMM + softmax-rows
    path of fastervit_functions.window_attention_fwd / _bwd."""
    return dtype == torch.bfloat16 and hd == 32 and 1 <= T <= 64


def wattn_fwd(qkv: torch.Tensor, bias: torch.Tensor | None, H: int, scale: float, want_lse: bool = True):
    """qkv [n, T, 1, 3*H*32] bf16 (q | k | v per token), bias f32 [H, T, T] or None ->
    (o [n, T, 1, H*32] bf16, L [n, H, T] f32 = row max + log(row sum) of scale*q k^T + bias)."""
    n, T = qkv.shape[0], qkv.shape[1]
    C = qkv.shape[-1] // 3
    out = torch.empty((n, T, 1, C), dtype=qkv.dtype, device=qkv.device)
    L = torch.empty((n, H, T), dtype=torch.float32, device=qkv.device) if want_lse else None
    check(_L().dfd_wattn_fwd(_p(qkv), _p(bias), _p(out), _p(L), n, T, H, C // H, float(scale), _stream()), "dfd_wattn_fwd",
          f"n={n} T={T} H={H}")
    return out, L


def wattn_bwd(qkv: torch.Tensor, dout: torch.Tensor, L: torch.Tensor, bias: torch.Tensor | None, H: int, scale: float,
              need_bias: bool):
    """-> (dqkv like qkv, dbias f32 [H, T, T] | None): gradients of wattn_fwd's inputs for the gradient `dout` of o."""
    n, T = qkv.shape[0], qkv.shape[1]
    C = qkv.shape[-1] // 3
    dqkv = torch.empty_like(qkv)
    parts = None
    rows = int(_L().dfd_wattn_parts(n))
    if need_bias:
        parts = torch.empty((rows + (min(rows, 1024) + 31) // 32 + 1) * H * T * T, dtype=torch.float32, device=qkv.device)
    check(_L().dfd_wattn_bwd(_p(qkv), _p(dout), _p(L), _p(bias), _p(dqkv), _p(parts), n, T, H, C // H, float(scale), _stream()),
          "dfd_wattn_bwd", f"n={n} T={T} H={H}")
    dbias = None
    if need_bias:
        dbias = torch.empty((H, T, T), dtype=torch.float32, device=qkv.device)
        sum_rows(parts, rows, H * T * T, dbias.view(-1))
    return dqkv, dbias


def attn_softmax_fwd(S: torch.Tensor, th: tuple | None):
    """S [B,H,Nq,Nk] f32 -> (P, T2); th = (w1 [H,H], b1 [H], w2 [H,H], b2 [H]) or None (then T2 is P)."""
    B, H, Nq, Nk = S.shape
    P = torch.empty_like(S)
    T2 = torch.empty_like(S) if th is not None else None
    w1, b1, w2, b2 = th if th is not None else (None,) * 4
    check(_L().dfd_attn_softmax_fwd(_p(S), _p(w1), _p(b1), _p(w2), _p(b2), _p(P), _p(T2), B, H, Nq, Nk, _stream()),
          "dfd_attn_softmax_fwd")
    return P, (T2 if th is not None else P)


def attn_softmax_bwd(dT2: torch.Tensor, P: torch.Tensor, th: tuple | None, out: torch.Tensor | None = None):
    """-> (dT1 | None, dS).  out: a contiguous destination for dS of P's shape (e.g. the leading rows of a padded buffer)."""
    B, H, Nq, Nk = P.shape
    if out is not None and (out.shape != P.shape or out.dtype != P.dtype):
        raise ValueError(f"attn_softmax_bwd: bad destination {tuple(out.shape)} {out.dtype} for {tuple(P.shape)} {P.dtype}")
    dS = torch.empty_like(P) if out is None else out
    dT1 = torch.empty_like(P) if th is not None else None
    w1, _, w2, _ = th if th is not None else (None,) * 4
    check(_L().dfd_attn_softmax_bwd(_p(dT2), _p(P), _p(w1), _p(w2), _p(dT1), _p(dS), B, H, Nq, Nk, _stream()), "dfd_attn_softmax_bwd")
    return dT1, dS


def bias_gather(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    H, T = table.shape
    L = idx.numel()
    full = torch.empty((H, L), dtype=torch.float32, device=table.device)
    check(_L().dfd_bias_gather(_p(table), _p(idx), _p(full), H, T, L, _stream()), "dfd_bias_gather")
    return full


def bias_scatter(dfull: torch.Tensor, idx: torch.Tensor, T: int, out: torch.Tensor | None = None) -> torch.Tensor:
    H = dfull.shape[0]
    L = idx.numel()
    dtable = _dst(out, (H, T), dfull.device)
    check(_L().dfd_bias_scatter(_p(dfull), _p(idx), _p(dtable), H, T, L, 0, _stream()), "dfd_bias_scatter")
    return dtable


def im2col(x: torch.Tensor, in_state: torch.Tensor | None, in_act: int, k: int, stride: int, pad: int, Ho: int, Wo: int) -> torch.Tensor:
    _chk_nhwc(x)
    N, H, W, C = x.shape
    col = torch.empty((N, Ho, Wo, k * k * C), dtype=x.dtype, device=x.device)
    shp = _dw_shape(x.shape, Ho, Wo, k, stride, pad, pad)
    check(_L().dfd_im2col(_dt(x), _p(x), _p(in_state), in_act, _p(col), ctypes.byref(shp), _stream()), "dfd_im2col")
    return col


def conv_fwd(x: torch.Tensor, in_state: torch.Tensor | None, in_act: int, w_nk: torch.Tensor, k: int, stride: int, pad: int,
             Ho: int, Wo: int, stats: bool = False):
    """Dense k x k convolution of act(bn(x)) (or x) with w_nk [Cout, k*k*C] as an implicit GEMM: (y, partials, nparts)."""
    _chk_nhwc(x)
    N, H, W, C = x.shape
    Cout = w_nk.shape[0]
    y = torch.empty((N, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
    parts = partials_buf(x.device, Cout) if stats else None
    n = ctypes.c_int(0)
    shp = _dw_shape(x.shape, Ho, Wo, k, stride, pad, pad)
    check(_L().dfd_conv_fwd(_dt(x), _p(x), ctypes.byref(shp), _p(in_state), in_act, _p(w_nk), Cout, _p(y), _p(parts),
                            MAX_PARTIALS, ctypes.byref(n), _stream()), "dfd_conv_fwd", f"{tuple(x.shape)} k{k}s{stride} -> {Cout}")
    return y, parts, n.value


def conv_wgrad(p: torch.Tensor, pro_p: Prologue | None, x: torch.Tensor, in_state: torch.Tensor | None, in_act: int, k: int,
               stride: int, pad: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """dw[Cout, k*k*C] (GEMM column order) = sum_m P(p)[m, co] * im2col(act(bn(x)))[m, :], the im2col operand gathered."""
    _chk_nhwc(x)
    Cout = p.shape[-1]
    _, Ho, Wo, _ = p.shape
    C = x.shape[-1]
    shp = _dw_shape(x.shape, Ho, Wo, k, stride, pad, pad)
    nbytes = int(_L().dfd_conv_wgrad_ws(ctypes.byref(shp), Cout))
    ws = scratch(p.device, "wgrad_ws", nbytes)
    dw = _dst(out, (Cout, k * k * C), p.device)
    check(_L().dfd_conv_wgrad(_dt(p), _p(p), ctypes.byref(pro_p) if pro_p is not None else None, Cout, _p(x), ctypes.byref(shp),
                              _p(in_state), in_act, _p(dw), 0, _p(ws), ws.numel() * 4, _stream()), "dfd_conv_wgrad",
          f"{tuple(x.shape)} k{k}s{stride} Cout={Cout}")
    return dw


def col2im(dcol: torch.Tensor, in_shape, k: int, stride: int, pad: int) -> torch.Tensor:
    N, H, W, C = in_shape
    Ho, Wo = dcol.shape[1], dcol.shape[2]
    dx = torch.empty((N, H, W, C), dtype=dcol.dtype, device=dcol.device)
    shp = _dw_shape(in_shape, Ho, Wo, k, stride, pad, pad)
    check(_L().dfd_col2im(_dt(dcol), _p(dcol), _p(dx), ctypes.byref(shp), _stream()), "dfd_col2im")
    return dx


def conv_weight_to_gemm(w: torch.Tensor) -> torch.Tensor:
    """torch [O, I, k, k] f32 -> [O, k*k*I] f32 with column (kh*k + kw)*I + i."""
    O, I, k, _ = w.shape
    out = torch.empty((O, k * k * I), dtype=torch.float32, device=w.device)
    check(_L().dfd_conv_weight_perm(_p(w), _p(out), O, I, k, 1, 0, _stream()), "dfd_conv_weight_perm")
    return out


def conv_weight_to_dgrad_gemm(w: torch.Tensor) -> torch.Tensor:
    """torch [O, I, k, k] f32 -> [I, k*k*O] f32, taps flipped: the forward-convolution weight that carries the output
    gradient of a stride-1 convolution back to its input (dfd_conv_fwd on the gradient tensor)."""
    O, I, k, _ = w.shape
    out = torch.empty((I, k * k * O), dtype=torch.float32, device=w.device)
    check(_L().dfd_conv_weight_perm(_p(w), _p(out), O, I, k, 2, 0, _stream()), "dfd_conv_weight_perm")
    return out


def conv_wgrad_from_gemm(dw_gemm: torch.Tensor, shape, out: torch.Tensor | None = None) -> torch.Tensor:
    O, I, k, _ = shape
    dw = _dst(out, (O, I, k, k), dw_gemm.device)
    check(_L().dfd_conv_weight_perm(_p(dw_gemm), _p(dw), O, I, k, 0, 0, _stream()), "dfd_conv_weight_perm")
    return dw


def layernorm_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, want_stats: bool = True):
    rows, C = _rows_c(x)
    y = torch.empty_like(x)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device) if want_stats else None
    check(_L().dfd_layernorm_fwd(_dt(x), _p(x), _p(gamma), _p(beta), eps, _p(y), _p(stats), rows, C, _stream()), "dfd_layernorm_fwd")
    return y, stats


def layernorm_bwd(g: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, stats: torch.Tensor, residual: torch.Tensor | None = None,
                  out2: torch.Tensor | None = None):
    """-> (dx [+ residual], dgamma, dbeta).  out2: an f32 [2, C] destination for (dgamma, dbeta) that nobody reads before the
    end of the enclosing block (two adjacent gradient-arena slots): the final sum of the partial rows then goes straight
    there and may be left to the block's batched sums (dfd_sum_rows_deferred) — no temporary, no copy kernels."""
    rows, C = _rows_c(x)
    dx = torch.empty_like(x)
    parts = partials_buf(x.device, C)
    n = ctypes.c_int(0)
    check(_L().dfd_layernorm_bwd(_dt(x), _p(g), _p(x), _p(gamma), _p(stats), _p(residual), _p(dx), _p(parts), MAX_PARTIALS,
                                 ctypes.byref(n), rows, C, _stream()), "dfd_layernorm_bwd")
    if out2 is not None:
        if tuple(out2.shape) != (2, C) or out2.dtype != torch.float32 or not out2.is_contiguous():
            raise ValueError("layernorm_bwd: out2 must be a contiguous f32 [2, C] tensor")
        check(_L().dfd_sum_rows_deferred(_p(parts), n.value, 2 * C, _p(out2), 0, _stream()), "dfd_sum_rows_deferred")
        return dx, out2[0], out2[1]
    both = torch.empty((2, C), dtype=torch.float32, device=x.device)
    sum_rows(parts, n.value, 2 * C, both)
    return dx, both[0], both[1]


def copy_rows(src: torch.Tensor, sidx: torch.Tensor | None, dst: torch.Tensor, didx: torch.Tensor | None, n: int) -> torch.Tensor:
    """dst[didx[r]] = src[sidx[r]] for r < n over [rows, C] matrices (int32 index tensors; None = identity)."""
    C = src.shape[-1]
    if dst.shape[-1] != C or src.dtype != dst.dtype:
        raise ValueError("copy_rows: source and destination rows differ")
    check(_L().dfd_copy_rows(_dt(src), _p(src), _p(sidx), _p(dst), _p(didx), n, C, _stream()), "dfd_copy_rows")
    return dst


def add_rowtable(x: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """x [.., T, C] + table [T, C] (f32), broadcast over the leading dimensions."""
    T, C = table.shape
    out = torch.empty_like(x)
    check(_L().dfd_add_rowtable(_dt(x), _p(x), _p(table), _p(out), x.numel() // C, T, C, _stream()), "dfd_add_rowtable")
    return out


def rowtable_grad(g: torch.Tensor, T: int) -> torch.Tensor:
    C = g.shape[-1]
    dtable = torch.empty((T, C), dtype=torch.float32, device=g.device)
    nbytes = int(_L().dfd_rowtable_grad_ws(T, C))
    ws = scratch(g.device, "rowtable_ws", nbytes)
    check(_L().dfd_rowtable_grad(_dt(g), _p(g), _p(dtable), g.numel() // C, T, C, 0, _p(ws), nbytes, _stream()),
          "dfd_rowtable_grad")
    return dtable


def rowtable_grad_plan(dtype: torch.dtype, rows: int, T: int, C: int) -> tuple[int, int, int]:
    """(splits, windows per split, row lanes) of rowtable_grad's launch for `rows` rows of C elements (host code, no launch)."""
    splits, w_per, rpb = ctypes.c_int(-1), ctypes.c_long(-1), ctypes.c_int(-1)
    check(_L().dfd_rowtable_grad_plan(_dt(dtype), rows, T, C, ctypes.byref(splits), ctypes.byref(w_per), ctypes.byref(rpb)),
          "dfd_rowtable_grad_plan", f"rows={rows} T={T} C={C}")
    return splits.value, w_per.value, rpb.value


def avgpool_fwd(x: torch.Tensor, k: int, stride: int) -> torch.Tensor:
    _chk_nhwc(x)
    N, H, W, C = x.shape
    out = torch.empty((N, (H - k) // stride + 1, (W - k) // stride + 1, C), dtype=x.dtype, device=x.device)
    check(_L().dfd_avgpool_fwd(_dt(x), _p(x), _p(out), N, H, W, k, stride, C, _stream()), "dfd_avgpool_fwd")
    return out


def avgpool_bwd(g: torch.Tensor, in_shape, k: int, stride: int) -> torch.Tensor:
    N, H, W, C = in_shape
    dx = torch.empty((N, H, W, C), dtype=g.dtype, device=g.device)
    check(_L().dfd_avgpool_bwd(_dt(g), _p(g), _p(dx), N, H, W, k, stride, C, _stream()), "dfd_avgpool_bwd")
    return dx


def relpos_bias_fwd(table: torch.Tensor, idx: torch.Tensor, n_local: int, n_global: int) -> torch.Tensor:
    """table [T, H] f32 -> [H, S, S] with S = n_local + n_global."""
    H = table.shape[1]
    S = n_local + n_global
    full = torch.empty((H, S, S), dtype=torch.float32, device=table.device)
    check(_L().dfd_relpos_bias_fwd(_p(table), _p(idx), _p(full), H, n_local, n_global, _stream()), "dfd_relpos_bias_fwd")
    return full


def relpos_bias_bwd(dfull: torch.Tensor, table: torch.Tensor, idx: torch.Tensor, n_local: int, n_global: int) -> torch.Tensor:
    T, H = table.shape
    dtable = torch.empty_like(table)
    check(_L().dfd_relpos_bias_bwd(_p(dfull), _p(table), _p(idx), _p(dtable), H, T, n_local, n_global, _stream()), "dfd_relpos_bias_bwd")
    return dtable


def _launch_jobs(name: str, Job, rows: list) -> None:
    """One launch of the batched entry point `name` over a ctypes array of `Job`, one per row of constructor arguments;
    a tensor in a row goes through the gate.  No rows: no launch."""
    if rows:
        arr = (Job * len(rows))(*(Job(*(_p(v) if isinstance(v, torch.Tensor) else v for v in row)) for row in rows))
        check(getattr(_L(), name)(arr, len(rows), _stream()), name)


def coord_tables_fwd(cmlp: list, relpos: list) -> None:
    """Every coordinate MLP of a level in one launch, then every relative-position bias built from their tables in one.
    cmlp: (coords [T, 2], w0 [Hd, 2], b0 [Hd], w2 [D, Hd], table [T, D]) f32, table = relu(coords w0^T + b0) w2^T;
    relpos: (table [T, H], idx int32, full [H, S, S], n_local, n_global) as relpos_bias_fwd."""
    _launch_jobs("dfd_coord_mlp_fwd_multi", _lib.CmlpJob,
                 [(c, w0, b0, w2, tab, None, None, None, None, c.shape[0], w2.shape[0], w0.shape[0], 0) for c, w0, b0, w2, tab in cmlp])
    _launch_jobs("dfd_relpos_bias_fwd_multi", _lib.RelposJob,
                 [(tab, idx, full, None, None, tab.shape[1], tab.shape[0], nl, ng) for tab, idx, full, nl, ng in relpos])


def coord_tables_bwd(relpos: list, cmlp: list) -> None:
    """The backward of coord_tables_fwd, bias first.  relpos: (table, idx, dfull, dtable [T, H], n_local, n_global);
    cmlp: (coords, w0, b0, w2, dtable [T, D], dw0 | None, db0 | None, dw2 | None)."""
    _launch_jobs("dfd_relpos_bias_bwd_multi", _lib.RelposJob,
                 [(tab, idx, None, g, dtab, tab.shape[1], tab.shape[0], nl, ng) for tab, idx, g, dtab, nl, ng in relpos])
    _launch_jobs("dfd_coord_mlp_bwd_multi", _lib.CmlpJob,
                 [(c, w0, b0, w2, None, g, dw0, db0, dw2, c.shape[0], w2.shape[0], w0.shape[0], 0) for c, w0, b0, w2, g, dw0, db0, dw2 in cmlp])


def axpby(x: torch.Tensor, y: torch.Tensor | None, a: float = 1.0, b: float = 1.0, a_dev: torch.Tensor | None = None,
          out: torch.Tensor | None = None) -> torch.Tensor:
    """(a * a_dev[0]) * x + b * y on f32 tensors (into `out`, e.g. a gradient-arena slot, when given)."""
    out = torch.empty_like(x) if out is None else out
    check(_L().dfd_axpby(_p(x), _p(y), a, b, _p(a_dev), _p(out), x.numel(), _stream()), "dfd_axpby")
    return out


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(a)
    check(_L().dfd_add(_dt(a), _p(a), _p(b), _p(out), a.numel(), _stream()), "dfd_add")
    return out


class DeviceRng:
    """Philox state {seed, offset} in device memory: every random tensor of a forward pass is a pure function of
    (seed, offset, stream id, index), and `tick()` advances the offset with a kernel — so a captured hipGraph
    draws fresh numbers on every replay (a host-side offset would be frozen into the graph)."""

    def __init__(self, device: torch.device, seed: int | None = None) -> None:
        with torch.inference_mode(False):
            self.state = torch.zeros(2, dtype=torch.int64, device=device)
        self.reseed(seed)
        self._counters = AddressTable([])

    @staticmethod
    def mix_seed(seed: int, rank: int) -> int:
        """The Philox key of data-parallel rank `rank`: ranks see different samples and must not share dropout /
        drop-connect / DropPath masks (a shared SEED would otherwise give every rank the same stream)."""
        return (seed ^ (rank * 0x9E3779B97F4A7C15)) & 0x7FFFFFFFFFFFFFFF

    def reseed(self, seed: int | None = None, rank: int | None = None) -> None:
        """(seed, offset) <- (mix(seed, rank), 0), in place (a captured hipGraph keeps reading the same two words).
        Defaults: torch.initial_seed() and $RANK.  Call after torch.manual_seed() to re-key an existing network."""
        seed = torch.initial_seed() if seed is None else seed
        rank = int(os.environ.get("RANK", "0")) if rank is None else rank
        host = torch.tensor([self.mix_seed(seed, rank), 0], dtype=torch.int64)
        with torch.inference_mode(False):
            self.state.copy_(host)

    def uniform(self, n: int, stream_id: int) -> torch.Tensor:
        out = torch.empty(n, dtype=torch.float32, device=self.state.device)
        check(_L().dfd_rand(_p(self.state), stream_id, 0.0, _p(out), n, _stream()), "dfd_rand")
        return out

    def drop_path_scale(self, n: int, keep: float, stream_id: int) -> torch.Tensor:
        out = torch.empty(n, dtype=torch.float32, device=self.state.device)
        check(_L().dfd_rand(_p(self.state), stream_id, keep, _p(out), n, _stream()), "dfd_rand")
        return out

    def tick(self, counters: list[torch.Tensor]) -> None:
        """One launch: every int64 counter += 1 (BatchNorm.num_batches_tracked) and the Philox offset += 1."""
        if not self._counters.valid_for(counters):
            table = self._counters = AddressTable(counters)
            with torch.inference_mode(False):
                table.dev = torch.tensor(table.ptrs, dtype=torch.int64).to(self.state.device) if counters else None
        self._counters.note()
        check(_L().dfd_step_tick(_p(self._counters.dev), len(counters), _p(self.state), _stream()), "dfd_step_tick")


# ------------------------------------------------------------------ measurement hook
# bench.py installs a list here; each front-end call then appends
# (name, algorithmic_bytes, flops, start_event, end_event).  Algorithmic bytes = every
# tensor the call must read or write once (activations, weights, coefficients), i.e.
# the DESIGN.md per-kernel figure, not counter traffic.
_profile_sink: list | None = None
_TIMED = ("bn_act_apply", "bn_bwd_reduce", "act_bn_bwd", "pool_act", "pool_bwd_reduce", "scale_rows", "dwconv_fwd",
          "dwconv_bwd_data", "dwconv_bwd_weight", "pwconv", "pwconv_wgrad", "pwconv_bwd_fused", "stem_conv_fwd", "stem_conv_wgrad",
          "stem_bwd_fused", "se_fc_fwd", "se_fc_bwd", "linear_fwd", "linear_bwd", "ce_loss", "adamw_step", "prep_weights", "bn_finalize",
          "bn_bwd_finalize", "dropout", "bgemm", "attn_scores", "attn_apply", "attn_softmax_fwd", "attn_softmax_bwd", "im2col", "col2im",
          "wattn_fwd", "wattn_bwd", "mx_quant_rows", "mx_gemm",
          "bn_add_act", "bn_add_act_bwd", "affine2_apply", "up2_act_fwd", "up2_act_bwd", "layernorm_fwd", "layernorm_bwd",
          "channel_stats", "subsample_add")


def set_profile_sink(sink: list | None) -> None:
    global _profile_sink
    _profile_sink = sink


def _tensor_bytes(obj) -> int:
    if isinstance(obj, torch.Tensor):
        if obj.dim() <= 1 and obj.numel() >= MAX_PARTIALS:      # scratch / partial slabs
            return 0
        return obj.numel() * obj.element_size()
    if isinstance(obj, Prologue):
        return getattr(obj, "_nbytes", 0)
    if isinstance(obj, (tuple, list)):
        return sum(_tensor_bytes(o) for o in obj)
    return 0


def _flops(name: str, args) -> float:
    if name == "pwconv":
        a, w = args[0], args[2]
        return 2.0 * (a.numel() // a.shape[-1]) * a.shape[-1] * w.shape[0]
    if name == "pwconv_wgrad":
        p, q = args[0], args[2]
        return 2.0 * (p.numel() // p.shape[-1]) * p.shape[-1] * q.shape[-1]
    if name == "pwconv_bwd_fused":                           # data gradient + weight gradient
        dz, x = args[0], args[3]
        return 4.0 * (dz.numel() // dz.shape[-1]) * dz.shape[-1] * x.shape[-1]
    return 0.0


def _bytes_8d(name: str, args, fallback: int) -> int:
    """Algorithmic bytes of SURVEY.md section 8(d) — every activation tensor the UNFUSED op must move once, without
    the operands the engine's own fusions add (the second tensor of an affine2 prologue, residuals, statistics):
      1x1 conv / dgrad   M*(K + Nout)*es + K*Nout*es          1x1 wgrad   M*(Ni + Nj)*es + Ni*Nj*4
      depthwise fwd      N*C*(Hin*Win + Hout*Wout)*es + k*k*C*4
      depthwise dgrad    N*C*(Hout*Wout + Hin*Win [+ Hin*Win when the activation derivative is fused])*es
      depthwise wgrad    N*C*(Hout*Wout + Hin*Win)*es
    Everything else: the tensors of the call (as `bytes incl. fusion operands`)."""
    try:
        if name == "pwconv":
            a, w = args[0], args[2]
            K_, es = a.shape[-1], a.element_size()
            M = a.numel() // K_
            return (M * K_ + M * w.shape[0]) * es + w.numel() * es
        if name == "pwconv_wgrad":
            p, q = args[0], args[2]
            M = p.numel() // p.shape[-1]
            return M * (p.shape[-1] + q.shape[-1]) * p.element_size() + p.shape[-1] * q.shape[-1] * 4
        if name == "pwconv_bwd_fused":
            # the TWO ops it replaces, each with its own 8(d) bytes (the kernel moves the shared operands once: that is the point)
            dz, x = args[0], args[3]
            Cm, Cin, es = dz.shape[-1], x.shape[-1], dz.element_size()
            M = dz.numel() // Cm
            return 2 * M * (Cm + Cin) * es + Cm * Cin * (es + 4)
        if name == "dwconv_fwd":
            x, k, Ho, Wo = args[0], args[4], args[8], args[9]
            N, H, W, C = x.shape
            return N * C * (H * W + Ho * Wo) * x.element_size() + k * k * C * 4
        if name == "dwconv_bwd_data":
            dz, xin, in_shape = args[0], args[4], args[7]
            N, H, W, C = in_shape
            return N * C * (dz.shape[1] * dz.shape[2] + H * W * (2 if xin is not None else 1)) * dz.element_size()
        if name == "dwconv_bwd_weight":
            dz, xin = args[0], args[3]
            N, H, W, C = xin.shape
            return N * C * (dz.shape[1] * dz.shape[2] + H * W) * dz.element_size()
    except (IndexError, AttributeError, TypeError):
        pass
    return fallback


def _timed(name: str, fn):
    def inner(*args, **kwargs):
        sink = _profile_sink
        if sink is None:
            return fn(*args, **kwargs)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*args, **kwargs)
        e1.record()
        nbytes = _tensor_bytes(args) + _tensor_bytes(list(kwargs.values())) + _tensor_bytes(out)
        sink.append((name, nbytes, _flops(name, args), e0, e1, _bytes_8d(name, args, nbytes)))
        return out

    inner.__name__ = name
    inner.__doc__ = fn.__doc__
    return inner


for _name in _TIMED:
    globals()[_name] = _timed(_name, globals()[_name])

__all__ = [name for name in dir() if not name.startswith("_")]
