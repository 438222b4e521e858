"""Deferred weight-gradient sums (kernels.sum_batch) against float64, inside a real autograd backward.

On the training path a block's slab sums are not launched at the block's exit: dfd_sum_batch_end_deferred parks the batch, the next two
dfd_act_bn_bwd launches run its two stages as passenger workgroups, and kernels.flush_passengers (an end-of-backward callback) launches
whatever is still parked.  Here a chain of small autograd Functions stands for the blocks of a network: each one's backward opens
K.sum_batch(), runs 0..3 carrier launches (act_bn_bwd on random tensors, some with a squeeze-excite job riding along) and adds seeded
partial slabs with K.sum_rows(deferred=True) into preallocated f32 destinations.  Every destination must then hold exactly the bits of the
same sum launched at once outside any batch, and lie within the float64 error bound of recursive f32 summation.
"""

from __future__ import annotations

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# |got - sum_p rows[p]| <= C_BOUND * terms * 2^-24 * sum_p |rows[p]| per element (terms: P, + 1 for an accumulated prior value).
# Recursive f32 summation of n terms is within (n - 1) * 2^-24 * sum |x| (the two-stage grouping only shortens the chains); a dropped or
# doubled row moves the result by about sum |x| / P, far outside this for every P used here.
C_BOUND = 2.0
SENTINEL = 3.0e30            # fills every slab behind its rows and every non-accumulated destination: a stage that reads rows nobody
                             # wrote, or a destination nobody wrote, shows up as a huge or NaN value


def _K():
    from deepfakedetection_amd import kernels as K

    return K


class Job:
    def __init__(self, P: int, L: int, acc: bool = False):
        self.P, self.L, self.acc = P, L, acc
        self.rows = self.out = self.prior = None


class Carrier:
    """One act_bn_bwd launch: dtype, channels, mode (0: D, 1: D * gate + dpool / HW, 2: dpool / HW), squeeze-excite job or not.
    invalid: a pointer combination no mode has (D and gate without dpool), sent through the raw ABI."""

    def __init__(self, dtype, C: int, mode: int = 0, se: bool = False, invalid: bool = False):
        self.dtype, self.C, self.mode, self.se, self.invalid = dtype, C, mode, se, invalid


def _launch_carrier(c: Carrier, gen: torch.Generator, dev) -> None:
    K = _K()
    from deepfakedetection_amd._lib import ACT_SILU, MAX_PARTIALS

    N, H, W = 2, 3, 5
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    y = rnd(N, H, W, c.C).to(c.dtype)
    D = rnd(N, H, W, c.C).to(c.dtype) if c.mode != 2 else None
    gate = torch.rand(N, c.C, generator=gen).to(dev) if c.mode == 1 else None
    dpool = rnd(N, c.C) if c.mode != 0 else None
    state = torch.cat([rnd(2, c.C), rnd(1, c.C), torch.rand(1, c.C, generator=gen).to(dev) + 0.5])
    if c.invalid:
        dz = torch.empty_like(y)
        parts = K.partials_buf(y.device, c.C)
        n = ctypes.c_int(0)
        rc = K._L().dfd_act_bn_bwd(K._dt(y), D.data_ptr(), y.data_ptr(), torch.rand(N, c.C, device=dev).data_ptr(), None,
                                   state.data_ptr(), ACT_SILU, dz.data_ptr(), N, H * W, c.C, parts.data_ptr(), MAX_PARTIALS,
                                   ctypes.byref(n), K._stream())
        assert rc != 0, "dfd_act_bn_bwd accepted D and gate without dpool"
        return
    se_job = None
    if c.se:
        R = 5
        se_job = (rnd(N, c.C), rnd(N * c.C + 2 * N * R), R, torch.empty(R, c.C, device=dev), torch.empty(R, device=dev),
                  torch.empty(c.C, R, device=dev), torch.empty(c.C, device=dev))
    K.act_bn_bwd(D, y, gate, dpool, state, ACT_SILU, se_job=se_job)


def _make_block(carriers, jobs, gen: torch.Generator):
    """An identity Function whose backward is one network block's worth of carriers and deferred slab sums."""
    K = _K()

    class Block(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            dev = g.device
            with K.sum_batch():
                for c in carriers:
                    _launch_carrier(c, gen, dev)
                for j in jobs:
                    need = (j.P + (min(j.P, 1024) + 31) // 32) * j.L
                    slab = K.scratch(dev, "test_slab", need * 4)
                    slab.fill_(SENTINEL)
                    slab[:j.P * j.L].copy_(j.rows.view(-1))
                    K.sum_rows(slab, j.P, j.L, out=j.out, accumulate=j.acc, deferred=True)
            return g

    return Block


def _run(blocks):
    """blocks: (carriers, jobs) in BACKWARD order (the first entry's backward runs first).  Returns every job."""
    K = _K()
    assert K.PASSENGER_SUMS and K.passenger_sums_enabled and K._DEFER_SUMS
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(1234)
    jobs = []
    for carriers, js in blocks:
        for j in js:
            j.rows = torch.randn(j.P, j.L, generator=gen)
            if j.acc:
                j.prior = torch.randn(j.L, generator=gen)
                j.out = j.prior.to(dev)
            else:
                j.out = torch.full((j.L,), SENTINEL, device=dev)
            jobs.append(j)
    fns = [_make_block(c, js, gen) for c, js in blocks]
    x = torch.zeros(4, device=dev, requires_grad=True)
    h = x
    for fn in reversed(fns):                          # forward order: the last block of the list is the first layer
        h = fn.apply(h)
    ends = K.deferred_ends[0]
    h.sum().backward()
    torch.cuda.synchronize()
    assert K._passenger_keep == [], "slab workspaces still held after the backward"
    return jobs, K.deferred_ends[0] - ends


def _check(jobs):
    K = _K()
    bad = []
    for k, j in enumerate(jobs):
        got = j.out.cpu()
        # the same slab summed at once, outside any batch: same grouping, same order, same bits
        need = (j.P + (min(j.P, 1024) + 31) // 32) * j.L
        slab = torch.full((need,), SENTINEL, device="cuda")
        slab[:j.P * j.L].copy_(j.rows.view(-1))
        once = j.prior.cuda() if j.acc else torch.full((j.L,), SENTINEL, device="cuda")
        K.sum_rows(slab, j.P, j.L, out=once, accumulate=j.acc, deferred=False)
        once = once.cpu()
        rows = j.rows.double()
        want = rows.sum(0)
        mag = rows.abs().sum(0)
        terms = j.P
        if j.acc:
            want, mag, terms = want + j.prior.double(), mag + j.prior.double().abs(), terms + 1
        err = (got.double() - want).abs()
        bound = C_BOUND * terms * 2.0 ** -24 * mag
        if not torch.isfinite(got).all() or bool((err > bound).any()):
            bad.append((k, j.P, j.L, j.acc, "float64", float((err / bound).nan_to_num(float("inf")).max())))
        elif not torch.equal(got, once):
            bad.append((k, j.P, j.L, j.acc, "bits", int((got != once).sum())))
    assert not bad, bad


f32, bf16 = torch.float32, torch.bfloat16


def test_deferred_sums_match_float64_and_immediate_bits():
    blocks = [
        # stage 1 and stage 2 jobs (P = 1, 31, 32 take stage 2 only), no carrier: parked at the stage-1 slot
        ([], [Job(1, 257), Job(31, 300), Job(32, 256), Job(33, 999), Job(1024, 260)]),
        # one carrier with nvc = 6 (f32, C = 1152): the passenger count is no multiple of it
        ([Carrier(f32, 1152, 1)], [Job(33, 513, acc=True), Job(64, 77)]),
        # a stage-2-only batch, behind two carriers, one carrying a squeeze-excite job as well
        ([Carrier(bf16, 672, 1, se=True), Carrier(f32, 40, 2)], [Job(1, 100), Job(31, 77, acc=True), Job(32, 1000)]),
        # three carriers; P > 1024 inside the open batch is summed at once (grouped, last group first) between parked jobs
        ([Carrier(bf16, 1152, 0), Carrier(f32, 64, 2, se=True), Carrier(bf16, 16, 1)],
         [Job(40, 300), Job(1025, 130), Job(1, 50, acc=True), Job(2100, 257, acc=True), Job(96, 33)]),
        # more than SUM_MAX_JOBS (8) jobs: the batch launches its first eight early
        ([], [Job(p, 70 + 13 * i, acc=(i % 3 == 0)) for i, p in enumerate([1, 2, 31, 32, 33, 65, 200, 257, 500, 1, 40])]),
        # a second deferred batch with no carrier in between: the stage-1 slot is still taken
        ([], [Job(100, 260), Job(3, 259, acc=True)]),
        ([Carrier(f32, 1152, 0)], [Job(1024, 129, acc=True)]),
        # the last batches of the pass are left for the end-of-backward flush
        ([], [Job(33, 31), Job(5, 511)]),
    ]
    jobs, deferred = _run(blocks)
    assert deferred == len(blocks), f"{deferred} of {len(blocks)} batches were deferred"
    _check(jobs)


def test_invalid_carrier_keeps_the_parked_sums():
    """A carrier launch that fails validation returns an error and carries nothing: the batches it would have taken stay parked and
    are summed by a later carrier or by the flush."""
    blocks = [
        ([], [Job(33, 300), Job(100, 129), Job(1, 77)]),                    # stage 1 parked
        ([Carrier(f32, 64, invalid=True)], [Job(31, 260), Job(2, 33)]),      # stage-2-only batch; the carrier would have moved stage 1 on
        ([Carrier(bf16, 672, 0)], [Job(65, 100, acc=True)]),                 # takes stage 1 of block 0: its stage 2 waits
        ([Carrier(f32, 1152, 0, invalid=True)], [Job(1, 50)]),               # would have dropped that stage 2
        ([Carrier(f32, 64, 1)], [Job(40, 257)]),
    ]
    jobs, deferred = _run(blocks)
    assert deferred == len(blocks)
    _check(jobs)
