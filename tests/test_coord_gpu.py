"""The batched coordinate-MLP kernels (csrc/dfd_coord.hip), called by name: tolerance 0, the batching itself, the edges.

dfd_coord_mlp_fwd_multi / _bwd_multi and dfd_relpos_bias_fwd_multi / _bwd_multi produce every position table and every
relative-position attention bias of FasterViT's levels 2 and 3 and the gradients of all cpb_mlp parameters.  The model tests reach
them through one HAT block (4 or 2 jobs in one launch) at 2e-3; a dropped tail column or a row counted twice in one job of 24 moves a
network-level gradient by far less.  Here they are called through `_L()` with CmlpJob / RelposJob arrays as CoordTablesFunction
does, and through CoordTablesFunction itself:

  * on the integer data of tests/_exact.py (coord_mlp, coord_cpb; the conditions and the f32 evaluation of the same data run on any
    machine, tests/test_exact_cpu.py) every output has to equal the float64 reference bit for bit - at the smallest shapes where each
    branch turns (T 64 | 65, T 88 | 89, D and Hd no multiple of a chunk), with pre-activations of exactly 0, with every subset of
    gradient destinations, and for the whole chain MLP -> table -> bias -> dbias -> dtable -> MLP backward at table = 0;
  * every output is an interior slice of a larger buffer prefilled with a NaN of a fixed payload: after the launch the slice equals the
    reference (so it was filled) and the guard elements still hold the payload; a destination that was not requested is not passed and
    its buffer stays untouched.  The inputs the backward pre-fetches in chunks (dtable, w2) lie in such buffers too, so a fetch past
    the tail of a row - harmless while what it reads is finite and gets multiplied by 0 - poisons the result here;
  * 1, 24, 25, 48 and 49 jobs in one call (1, 1, 2, 2, 3 launches of CM_JOBS = 24), shapes mixed in the shipped order with the largest
    job first or last, hidden widths 36 / 512 / 1024 in one backward launch, three attention geometries in one relpos launch; and on
    Gaussian data a job's bits are the same alone, at slot 0 and at slot 24 (the fixed summation order the kernels' header promises);
  * the six shipped geometries on real numbers against the oracle in float64 at the tolerances of test_rowtable_avgpool_relpos
    (1e-5 forward, 1e-4 gradients), after the CPU has checked that no ReLU unit sits within f32 rounding of 0;
  * argument checks: DFD_EINVAL and nothing written.
All tensors are at most 176 x 1024 floats (1024 x 512 for a weight).
"""

from __future__ import annotations

import functools
import math
from types import SimpleNamespace as NS

import pytest
import torch

from tests import _exact as E
from tests._exact import same

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD = 64                                   # floats in front of and behind every guarded tensor: the slice keeps a 256-byte alignment
NAN_BITS = 0x7FC5A5A5                        # a quiet NaN with a payload no kernel produces
ALL = ("dw0", "db0", "dw2")
POS49, POS16, BIG_D, T65, T89, HD36, HD1024 = 2, 1, 3, 7, 9, 10, 6          # indices into E.COORD_SHAPES
assert [E.COORD_SHAPES[i] for i in (POS49, POS16, BIG_D, T65, T89, HD36, HD1024)] == \
    [(49, 256, 512), (16, 320, 512), (49, 1024, 512), (65, 17, 512), (89, 40, 512), (176, 70, 36), (64, 33, 1024)]
CPB53, CPB49, CPB16 = 0, 1, 2                                                # indices into E.CPB_GEOMS


def _k():
    from deepfakedetection_amd import kernels

    return kernels


def _structs():
    from deepfakedetection_amd._lib import CmlpJob, RelposJob

    return CmlpJob, RelposJob


def close(got, want, rel, what=""):
    """max |err| over max |ref|, as the tolerance tests of the single-job kernels measure it (tests/test_vit_ops_gpu.py)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    scale = max(float(want.abs().max()), 1e-6)
    err = float((got - want).abs().max()) / scale
    assert err <= rel, f"{what}: max err {err:.3e} of max |ref| {scale:.3e} > {rel:.1e}"


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int32).cpu()


class Guarded:
    """A tensor that is an interior slice of a larger buffer prefilled with NAN_BITS."""

    def __init__(self, shape, back: int = GUARD) -> None:
        self.n, self.front = math.prod(shape), GUARD
        self.buf = torch.full((self.front + self.n + back,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
        self.t = self.buf[self.front:self.front + self.n].view(tuple(shape))

    @classmethod
    def of(cls, src: torch.Tensor, back: int = GUARD) -> "Guarded":
        g = cls(src.shape, back)
        g.t.copy_(src)
        return g

    def guards_intact(self, what: str) -> None:
        b = self.buf.view(torch.int32)
        edge = torch.cat([b[:self.front], b[self.front + self.n:]])
        assert bool((edge == NAN_BITS).all()), f"{what}: elements outside the output were written"

    def untouched(self, what: str) -> None:
        assert bool((self.buf.view(torch.int32) == NAN_BITS).all()), f"{what}: written although it was not passed"

    def equals(self, want: torch.Tensor, what: str) -> None:
        same(self.t, want, what)
        self.guards_intact(what)


@functools.lru_cache(maxsize=None)
def _inputs(kind: str, i: int):
    """The read-only operands of one case on the device, shared by every job made from it.  w2 and the MLP's dtable sit in guarded
    buffers: the backward fetches both in chunks of up to 32 columns (32 rows of w2), and what lies behind them is NaN."""
    c = E.coord_mlp(i) if kind == "mlp" else E.coord_cpb(i)
    Hd = c.shape[2]
    d = NS(c=c, coords=c.coords.cuda(), w0=c.w0.cuda(), b0=c.b0.cuda(), w2=Guarded.of(c.w2.cuda(), back=32 * Hd))
    if kind == "mlp":
        d.dtable = Guarded.of(c.dtable.cuda())
    else:
        d.idx, d.dbias, d.sat_table = c.idx.cuda(), c.dbias.cuda(), c.sat_table.cuda()
        d.zero_table = torch.zeros(c.shape[:2], device="cuda")
    return d


class Job:
    """One coordinate-MLP job with guarded outputs of its own; `cpb` jobs own the relpos tensors (full, dtable) as well."""

    def __init__(self, kind: str, i: int, want=ALL, data=None) -> None:
        self.kind, self.want = kind, tuple(want)
        self.d = d = data if data is not None else _inputs(kind, i)
        self.c = c = d.c
        T, D, Hd = c.shape
        self.table = Guarded((T, D))
        self.dw0, self.db0, self.dw2 = Guarded((Hd, 2)), Guarded((Hd,)), Guarded((D, Hd))
        if kind == "cpb":
            nl, ng, _, H = c.geom
            self.full = Guarded((H, nl + ng, nl + ng))
            self.dtable = Guarded((T, D))              # written by the relpos backward, read by the MLP backward
        else:
            self.dtable = d.dtable

    def _dest(self, name: str):
        return _k()._p(getattr(self, name).t) if name in self.want else None

    def mlp_fwd(self):
        p, d, (T, D, Hd) = _k()._p, self.d, self.c.shape
        return _structs()[0](p(d.coords), p(d.w0), p(d.b0), p(d.w2.t), p(self.table.t), None, None, None, None, T, D, Hd, 0)

    def mlp_bwd(self):
        p, d, (T, D, Hd) = _k()._p, self.d, self.c.shape
        return _structs()[0](p(d.coords), p(d.w0), p(d.b0), p(d.w2.t), None, p(self.dtable.t), self._dest("dw0"), self._dest("db0"),
                             self._dest("dw2"), T, D, Hd, 0)

    def rp_fwd(self, table=None, full=None):
        p, (nl, ng, T, H) = _k()._p, self.c.geom
        return _structs()[1](p(self.table.t if table is None else table), p(self.d.idx), p((self.full if full is None else full).t), None, None,
                             H, T, nl, ng)

    def rp_bwd(self, table=None):
        p, (nl, ng, T, H) = _k()._p, self.c.geom
        return _structs()[1](p(self.table.t if table is None else table), p(self.d.idx), None, p(self.d.dbias), p(self.dtable.t), H, T, nl, ng)

    def check_fwd(self, what: str) -> None:
        self.table.equals(self.c.table, f"{what} {self.c.what}: table")
        if self.kind == "cpb":
            self.full.equals(self.c.bias, f"{what} {self.c.what}: bias")

    def check_bwd(self, what: str) -> None:
        if self.kind == "cpb":
            self.dtable.equals(self.c.dtable, f"{what} {self.c.what}: dtable")
            rows = self.dtable.t[~self.c.used.cuda()]
            assert rows.numel() == 0 or float(rows.abs().max()) == 0.0, f"{what} {self.c.what}: a table row nobody names has a gradient"
        for name in ALL:
            out = getattr(self, name)
            if name in self.want:
                out.equals(getattr(self.c, name), f"{what} {self.c.what} wanting {self.want}: {name}")
            else:
                out.untouched(f"{what} {self.c.what} wanting {self.want}: {name}")


def launch(name: str, structs) -> int:
    arr = (type(structs[0]) * len(structs))(*structs)
    return getattr(_k()._L(), name)(arr, len(structs), _k()._stream())


def ok(code: int, name: str) -> None:
    assert code == 0, f"{name} returned {code}"


def run_all(jobs, what: str) -> None:
    """Forward and backward of a list of jobs through the four entry points, one call each, and every output compared."""
    cpb = [j for j in jobs if j.kind == "cpb"]
    ok(launch("dfd_coord_mlp_fwd_multi", [j.mlp_fwd() for j in jobs]), "dfd_coord_mlp_fwd_multi")
    if cpb:
        ok(launch("dfd_relpos_bias_fwd_multi", [j.rp_fwd() for j in cpb]), "dfd_relpos_bias_fwd_multi")
        ok(launch("dfd_relpos_bias_bwd_multi", [j.rp_bwd() for j in cpb]), "dfd_relpos_bias_bwd_multi")
    ok(launch("dfd_coord_mlp_bwd_multi", [j.mlp_bwd() for j in jobs]), "dfd_coord_mlp_bwd_multi")
    for n, j in enumerate(jobs):
        j.check_fwd(f"{what}, slot {n}")
        j.check_bwd(f"{what}, slot {n}")


# ------------------------------------------------------------------------------------------------------ a. exact, one job
@pytest.mark.parametrize("ci", E.COORD_CASES)
def test_mlp_exact(ci):
    run_all([Job("mlp", ci)], "one job")


@pytest.mark.parametrize("gi", range(len(E.CPB_GEOMS)))
def test_cpb_chain_exact(gi):
    j = Job("cpb", gi)
    run_all([j], "one job")
    sat = Guarded(j.full.t.shape)                                             # the gather itself: rows of 0 and of 16 by the index
    ok(launch("dfd_relpos_bias_fwd_multi", [j.rp_fwd(j.d.sat_table, sat)]), "dfd_relpos_bias_fwd_multi")
    sat.equals(j.c.sat_bias, f"{j.c.what}: bias of the saturated table")


# ------------------------------------------------------------------------------------------------------ b. batching
SHIPPED_ORDER = [("mlp", POS49), ("cpb", CPB53), ("mlp", POS16), ("cpb", CPB16)]       # pos 49 x dim, cpb 169 x heads, pos 16 x dim, cpb 49 x heads


def shipped_mix(n: int, largest: str):
    specs = [SHIPPED_ORDER[i % 4] for i in range(n)]
    specs[0 if largest == "first" else -1] = ("mlp", BIG_D)                   # 49 x 1024: it sizes the forward grid of its launch
    return specs


@pytest.mark.parametrize("largest", ["first", "last"])
@pytest.mark.parametrize("n", [1, 24, 25, 48, 49])
def test_batches_of_mixed_jobs(n, largest):
    run_all([Job(kind, i) for kind, i in shipped_mix(n, largest)], f"{n} jobs, largest {largest}")


@pytest.mark.parametrize("order", [(HD1024, POS49, HD36, T89), (HD36, T65, POS49, HD1024)])
def test_backward_launch_of_mixed_hidden_widths(order):
    """Hd 36, 512 and 1024 in one launch: the grid has 16 hidden chunks, the jobs 1, 8 and 16."""
    run_all([Job("mlp", ci) for ci in order], f"hidden widths {[E.COORD_SHAPES[ci][2] for ci in order]}")


@pytest.mark.parametrize("order", [(CPB49, CPB53, CPB16), (CPB16, CPB53, CPB49)])
@pytest.mark.parametrize("n", [1, 24, 25, 48, 49])
def test_relpos_batches_of_mixed_geometries(n, order):
    """The relpos kernels alone on tables of their own: even slots gather a saturated table (bias 0 / 16 by the row named), odd slots
    the zero table (bias 8); every backward runs at the zero table (dtable = 4 scatter(dbias))."""
    jobs = [Job("cpb", order[s % 3]) for s in range(n)]
    fwd = [j.rp_fwd(j.d.sat_table if s % 2 == 0 else j.d.zero_table) for s, j in enumerate(jobs)]
    ok(launch("dfd_relpos_bias_fwd_multi", fwd), "dfd_relpos_bias_fwd_multi")
    ok(launch("dfd_relpos_bias_bwd_multi", [j.rp_bwd(j.d.zero_table) for j in jobs]), "dfd_relpos_bias_bwd_multi")
    for s, j in enumerate(jobs):
        j.full.equals(j.c.sat_bias if s % 2 == 0 else j.c.bias, f"{n} relpos jobs, slot {s} {j.c.what}: bias")
        j.dtable.equals(j.c.dtable, f"{n} relpos jobs, slot {s} {j.c.what}: dtable")
        j.table.untouched(f"{n} relpos jobs, slot {s}: the MLP's table")


def _gaussian(kind: str, i: int, seed: int):
    """A job of the case's shape on Gaussian numbers (weights as the model tests draw them): no reference, only bits to compare."""
    c = E.coord_mlp(i) if kind == "mlp" else E.coord_cpb(i)
    T, D, Hd = c.shape
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape, scale=1.0: (torch.randn(shape, generator=g) * scale).cuda()
    d = NS(c=c, coords=r(T, 2), w0=r(Hd, 2, scale=0.5), b0=r(Hd, scale=0.1), w2=Guarded.of(r(D, Hd, scale=0.05), back=32 * Hd))
    if kind == "mlp":
        d.dtable = Guarded.of(r(T, D))
    else:
        nl, ng, _, H = c.geom
        d.idx, d.dbias = c.idx.cuda(), r(H, nl + ng, nl + ng)
    return d


@pytest.mark.parametrize("kind,i", [("mlp", T89), ("mlp", T65), ("cpb", CPB53)])
def test_a_jobs_bits_do_not_depend_on_its_slot(kind, i):
    """Alone, at slot 0 and at slot 24 (the first job of the second launch) among jobs of other shapes: the same bits in every output,
    on data where a changed summation order would show."""
    data = _gaussian(kind, i, 77 + i)
    alone, first, second = (Job(kind, i, data=data) for _ in range(3))
    fill = [Job(k, ci) for k, ci in shipped_mix(24, "last")[1:]]               # 23 exact jobs in between, the largest at slot 23
    batch = [first] + fill + [second]

    def run(jobs):
        cpb = [j for j in jobs if j.kind == "cpb"]
        ok(launch("dfd_coord_mlp_fwd_multi", [j.mlp_fwd() for j in jobs]), "dfd_coord_mlp_fwd_multi")
        if cpb:
            ok(launch("dfd_relpos_bias_fwd_multi", [j.rp_fwd() for j in cpb]), "dfd_relpos_bias_fwd_multi")
            ok(launch("dfd_relpos_bias_bwd_multi", [j.rp_bwd() for j in cpb]), "dfd_relpos_bias_bwd_multi")
        ok(launch("dfd_coord_mlp_bwd_multi", [j.mlp_bwd() for j in jobs]), "dfd_coord_mlp_bwd_multi")

    run([alone])
    run(batch)
    names = ("table", "dw0", "db0", "dw2") + (("full", "dtable") if kind == "cpb" else ())
    for name in names:
        a = getattr(alone, name)
        assert bool(torch.isfinite(a.t).all()) and float(a.t.abs().max()) > 0.0, f"{name}: not filled"
        for where, other in (("slot 0", first), ("slot 24", second)):
            o = getattr(other, name)
            assert torch.equal(bits(a.t), bits(o.t)), f"{name}: alone and at {where} differ in their bits"
            o.guards_intact(f"{name} at {where}")
    for n, j in enumerate(fill):
        j.check_fwd(f"fill job {n + 1}")
        j.check_bwd(f"fill job {n + 1}")


# ------------------------------------------------------------------------------------------------------ c. partial gradients
@pytest.mark.parametrize("ci", E.COORD_CASES)
def test_mlp_partial_gradients(ci):
    """dw2 alone is the path without dh; dw0 / db0 alone and together leave dw2 out.  What is not requested is not passed."""
    for want in (("dw2",), ("dw0",), ("db0",), ("dw0", "db0")):
        j = Job("mlp", ci, want)
        ok(launch("dfd_coord_mlp_bwd_multi", [j.mlp_bwd()]), "dfd_coord_mlp_bwd_multi")
        j.check_bwd("partial gradients")
        j.table.untouched("partial gradients: the forward's table")


def test_partial_gradients_mixed_in_one_launch():
    """Jobs with and without dh side by side (the early exit behind the dw2 loop is per workgroup), the cpb chain's among them."""
    wants = [("dw2",), ALL, ("db0",), ("dw0", "db0"), ("dw2",), ("dw0",)]
    specs = [("mlp", T89), ("mlp", HD1024), ("cpb", CPB53), ("mlp", T65), ("cpb", CPB16), ("mlp", HD36)]
    run_all([Job(k, i, w) for (k, i), w in zip(specs, wants)], "mixed destinations")


# ------------------------------------------------------------------------------------------------------ d. through autograd
def _autograd_run(specs, frozen=None, left_out=()):
    """coord_tables on leaf parameters; `frozen`: {job: names without a gradient}; `left_out`: jobs whose output is not differentiated.
    -> (outputs, parameter triples)."""
    from deepfakedetection_amd.fastervit_functions import CoordJob, coord_tables

    frozen = frozen or {}
    jobs, params, gouts = [], [], []
    for n, (kind, i) in enumerate(specs):
        d = _inputs(kind, i)
        c = d.c
        for name in ("w0", "b0", "w2"):
            params.append(getattr(c, name).cuda().requires_grad_(name not in frozen.get(n, ())))
        if kind == "cpb":
            nl, ng, _, _ = c.geom
            jobs.append(CoordJob("cpb", d.coords, d.idx, nl, ng))
            gouts.append(d.dbias)
        else:
            jobs.append(CoordJob("pos", d.coords))
            gouts.append(d.dtable.t)
    outs = coord_tables(jobs, params)
    keep = [n for n in range(len(specs)) if n not in left_out]
    torch.autograd.backward([outs[n] for n in keep], [gouts[n] for n in keep])
    return outs, [params[3 * n:3 * n + 3] for n in range(len(specs))]


AUTOGRAD_SPECS = shipped_mix(25, "last")[:-2] + [("mlp", T89), ("mlp", BIG_D)]


def _check_autograd(specs, outs, triples, frozen=None, left_out=(), what=""):
    frozen = frozen or {}
    for n, (kind, i) in enumerate(specs):
        c = _inputs(kind, i).c
        same(outs[n], c.bias if kind == "cpb" else c.table, f"{what} job {n} {c.what}: output")
        for name, p in zip(("w0", "b0", "w2"), triples[n]):
            if name in frozen.get(n, ()):
                assert p.grad is None, f"{what} job {n}: frozen {name} got a gradient"
            elif n in left_out:
                # an output that is left out of the loss reaches backward as a zero gradient: the kernels run and write exact zeros
                assert p.grad is not None and float(p.grad.abs().max()) == 0.0, f"{what} job {n}: {name} of an unused output"
            else:
                same(p.grad, getattr(c, "d" + name), f"{what} job {n} {c.what}: {name}.grad")


def test_coord_tables_through_autograd():
    """25 mixed jobs (two launches of each kernel) outside any gradient arena: outputs and every .grad exact, and two runs bit for bit."""
    outs, triples = _autograd_run(AUTOGRAD_SPECS)
    _check_autograd(AUTOGRAD_SPECS, outs, triples, what="all trainable")
    outs2, triples2 = _autograd_run(AUTOGRAD_SPECS)
    for a, b in zip(outs, outs2):
        assert torch.equal(bits(a), bits(b))
    for ta, tb in zip(triples, triples2):
        for a, b in zip(ta, tb):
            assert torch.equal(bits(a.grad), bits(b.grad))


def test_coord_tables_with_frozen_parameters():
    """Job 0 fully frozen (it drops out of the backward), job 1 (a cpb job) with only w2 trainable, job 2 with only b0 frozen."""
    frozen = {0: ("w0", "b0", "w2"), 1: ("w0", "b0"), 2: ("b0",)}
    outs, triples = _autograd_run(AUTOGRAD_SPECS, frozen)
    _check_autograd(AUTOGRAD_SPECS, outs, triples, frozen, what="some frozen")


def test_coord_tables_with_an_output_left_out_of_the_loss():
    left_out = (2, 5)                                          # a position table and an attention bias
    assert [AUTOGRAD_SPECS[n][0] for n in left_out] == ["mlp", "cpb"]
    outs, triples = _autograd_run(AUTOGRAD_SPECS, None, left_out)
    _check_autograd(AUTOGRAD_SPECS, outs, triples, None, left_out, what="two outputs unused")


# ------------------------------------------------------------------------------------------------------ e. shipped geometry
def test_shipped_geometries_against_the_oracle_in_float64():
    """All six modules of a block as one batch on real numbers, fed by the project's own coordinate and index buffers.  Seed
    E.SHIPPED_SEED is one at which every pre-activation clears 4 * 2**-24 * (|cx w0x| + |cy w0y| + |b0|) (E.relu_margin, checked on the
    CPU before the first launch; a violation raises): the ReLU masks of f32 and float64 agree, so what is left is rounding - the f32
    oracle stays within 5.4e-7 of float64 on these modules - against 1e-5 forward and 1e-4 for every gradient."""
    from deepfakedetection_amd.fastervit_functions import CoordJob, coord_tables

    ref = E.coord_shipped()                                    # builds the references and checks the condition: no launch before this
    jobs, params = [], []
    for r in ref:
        coords = r.coords.cuda()
        jobs.append(CoordJob("pos", coords) if r.kind == "pos" else CoordJob("cpb", coords, r.idx.cuda(), r.n_local, r.n_global))
        params += [t.cuda().requires_grad_(True) for t in (r.w0, r.b0, r.w2)]
    outs = coord_tables(jobs, params)
    torch.autograd.backward(outs, [r.g.cuda() for r in ref])
    for n, r in enumerate(ref):
        what = f"shipped {r.kind} {r.spec}"
        close(outs[n], r.out, 1e-5, f"{what}: output")
        if r.kind == "cpb" and r.n_global:
            o = outs[n].detach()
            assert float(o[:, :r.n_global].abs().max()) == 0.0 and float(o[:, :, :r.n_global].abs().max()) == 0.0
        for name, p in zip(("dw0", "db0", "dw2"), params[3 * n:3 * n + 3]):
            close(p.grad, getattr(r, name), 1e-4, f"{what}: {name}")


# ------------------------------------------------------------------------------------------------------ f. argument checks
def _with(struct, **fields):
    new = type(struct)()
    for name, _ in struct._fields_:
        setattr(new, name, getattr(struct, name))
    for name, v in fields.items():
        setattr(new, name, v)
    return new


def test_argument_checks_return_einval_and_write_nothing():
    lib, stream = _k()._L(), _k()._stream()
    m, r = Job("mlp", 0), Job("cpb", CPB16)
    good = Job("mlp", POS16)
    fwd, bwd, rfwd, rbwd = m.mlp_fwd(), m.mlp_bwd(), r.rp_fwd(), r.rp_bwd()
    for name, one in (("dfd_coord_mlp_fwd_multi", fwd), ("dfd_coord_mlp_bwd_multi", bwd), ("dfd_relpos_bias_fwd_multi", rfwd),
                      ("dfd_relpos_bias_bwd_multi", rbwd)):
        arr = (type(one) * 1)(one)
        assert getattr(lib, name)(arr, 0, stream) == EINVAL, f"{name}: njobs = 0"
        assert getattr(lib, name)(arr, -1, stream) == EINVAL, f"{name}: njobs = -1"
        assert getattr(lib, name)(None, 1, stream) == EINVAL, f"{name}: null jobs"
    bad_mlp = {"T = 0": dict(T=0), "T = 177": dict(T=177), "Hd = 6": dict(Hd=6), "Hd = 1028": dict(Hd=1028), "Hd = 0": dict(Hd=0),
               "D = 0": dict(D=0), "no coords": dict(coords=None), "no w2": dict(w2=None)}
    for what, fields in bad_mlp.items():
        assert launch("dfd_coord_mlp_fwd_multi", [_with(fwd, **fields)]) == EINVAL, f"forward, {what}"
        assert launch("dfd_coord_mlp_bwd_multi", [_with(bwd, **fields)]) == EINVAL, f"backward, {what}"
    assert launch("dfd_coord_mlp_fwd_multi", [_with(fwd, table=None)]) == EINVAL, "a forward job without table"
    assert launch("dfd_coord_mlp_bwd_multi", [_with(bwd, dw0=None, db0=None, dw2=None)]) == EINVAL, "dtable but no destination"
    assert launch("dfd_coord_mlp_bwd_multi", [_with(bwd, dtable=None)]) == EINVAL, "a backward job without dtable"
    for what, fields in {"n_local = 0": dict(n_local=0), "n_global = -1": dict(n_global=-1), "H = 0": dict(H=0), "T = 0": dict(T=0),
                         "no idx": dict(idx=None), "no table": dict(table=None)}.items():
        assert launch("dfd_relpos_bias_fwd_multi", [_with(rfwd, **fields)]) == EINVAL, f"relpos forward, {what}"
        assert launch("dfd_relpos_bias_bwd_multi", [_with(rbwd, **fields)]) == EINVAL, f"relpos backward, {what}"
    assert launch("dfd_relpos_bias_fwd_multi", [_with(rfwd, full=None)]) == EINVAL, "relpos forward without full"
    assert launch("dfd_relpos_bias_bwd_multi", [_with(rbwd, dfull=None)]) == EINVAL, "relpos backward without dfull"
    assert launch("dfd_relpos_bias_bwd_multi", [_with(rbwd, dtable=None)]) == EINVAL, "relpos backward without dtable"
    # every job is checked before the first launch: a valid job in front of an invalid one is not run either
    assert launch("dfd_coord_mlp_fwd_multi", [good.mlp_fwd()] * 24 + [_with(fwd, T=177)]) == EINVAL
    assert launch("dfd_coord_mlp_bwd_multi", [good.mlp_bwd()] * 24 + [_with(bwd, Hd=6)]) == EINVAL
    assert launch("dfd_relpos_bias_fwd_multi", [rfwd] * 24 + [_with(rfwd, n_local=0)]) == EINVAL
    assert launch("dfd_relpos_bias_bwd_multi", [rbwd] * 24 + [_with(rbwd, dfull=None)]) == EINVAL
    torch.cuda.synchronize()
    for j in (m, r, good):
        for name in ("table", "dw0", "db0", "dw2") + (("full", "dtable") if j.kind == "cpb" else ()):
            getattr(j, name).untouched(f"argument checks: {name} of {j.c.what}")
