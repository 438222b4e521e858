"""The reference side of tests/test_fastervit_bf16_gpu.py on its own, without a GPU (tests/_fastervit_bwd_ref.py): for every case
the float64 dictionary has the expected keys (qkv cut into its q, k and v thirds), the structurally zero gradients are exactly the
names the arithmetic predicts (the k third of every qkv.bias; conv1.bias and conv2.bias of a training-mode ConvBlock), a scaled
case's row scales hold both 0 and 1.25 with indices 1 and n - 1 dropped and differ between the two streams, and no yardstick
exceeds the cap.

The cap is a condition of the GPU test: its bound is 2 * yardstick + 2e-3, and a yardstick near 0.5 would let anything pass.
CAP is 0.10 against a measured maximum of 0.0764 (conv_down.1.bias of the FasterViT-0 patch embed, 0.0710 for FasterViT-1: the first
BatchNorm's bias gradient behind a ReLU at 4 x 112^2 rows); the hat blocks' largest are the coordinate MLPs' gradients (cpb_mlp.0.bias
0.039 .. 0.060), every other tensor is below 0.03.  A seed that pushes a yardstick over the cap is changed; the cap is not.

CPU seconds for the float64 and the autocast pass together, measured on 8 threads: 0.0 .. 1.0 per ConvBlock, Downsample,
TokenInitializer, stem and tail case (6.3 for all 28); 0.1 .. 3.2 per hat case (17.5 for all 13; the largest blocks: fv0 at B 97 1.6 ..
1.9, fv3 at B 48 2.3, and the first case of a variant pays for building its network); this module as a whole 24.  No case is
impractically slow, so none is shrunk; the references are kept by lru_cache for the tests of the GPU module to share.
"""

from __future__ import annotations

import pytest
import torch

from tests import _fastervit_bwd_ref as E

CAP = 0.10


@pytest.mark.parametrize("case", E.CASES, ids=[c.id for c in E.CASES])
def test_reference_of_the_case(case):
    inp = E.inputs(case)
    ref, yard, zeros = E.reference(case)
    params = [n for n in E.cut_qkv(dict(inp.mod.named_parameters()))]
    outs = {"out.x", "out.ct", "x.grad", "ct.grad"} if inp.carrier else {"out"} | ({"x.grad"} if case.kind != "stem" else set())
    assert set(ref) == outs | set(params), set(ref) ^ (outs | set(params))
    assert set(yard) == set(ref)
    assert all(bool(torch.isfinite(t).all()) and t.dtype == torch.float64 for t in ref.values())
    for name, g in inp.g.items():
        assert tuple(ref[name].shape) == tuple(g.shape), name
    assert set(zeros) == E.expected_zeros(case, params), set(zeros) ^ E.expected_zeros(case, params)
    assert E.exact_zeros(case, params) <= set(zeros)
    if case.kind == "hat":                                               # the slice rule: the k third of qkv.bias, on the k third of the weight
        want = {"attn.qkv.bias[k]"} | ({"hat_attn.qkv.bias[k]"} if inp.carrier else set())
        assert set(zeros) == want and all(E.sibling(n) == n.replace("bias", "weight") and E.sibling(n) in ref for n in zeros)
        assert not any(n.endswith(("qkv.weight", "qkv.bias")) for n in ref)
        if case.variant == "3":
            assert {n for n in params if n.startswith("gamma")} == ({"gamma1", "gamma2", "gamma3", "gamma4"} if inp.carrier else {"gamma3", "gamma4"})
    for n in set(ref) - set(zeros):                                      # everything else carries signal: nothing is judged against noise
        assert float(ref[n].abs().max()) > 0.0, n
        if E._is_bias(n) and E.sibling(n) in ref:
            assert float(ref[n].abs().max()) > 1e-4 * float(ref[E.sibling(n)].abs().max()), n
    assert (inp.masks is not None) == case.scaled
    for m in (inp.masks or ()):
        if m is not None:
            assert set(m.tolist()) == {0.0, 1.25} and m[1] == 0.0 and m[-1] == 0.0
    if case.scaled and case.kind == "hat":
        m_ct, m_win = inp.masks
        assert m_win.shape == (case.windows,) and (m_ct is None) == (not inp.carrier)
        if m_ct is not None:                                             # the streams do not share a pattern, image by image
            assert m_ct.shape == (case.n,)
            per_image = m_win.view(case.n, 4)
            assert bool(((per_image != 0) & (m_ct[:, None] == 0)).any()) and bool(((per_image == 0) & (m_ct[:, None] != 0)).any())
    elif case.scaled:
        assert inp.masks[0].shape == (case.n,)
    worst = max(yard, key=yard.get)
    print(f"{case.id}: largest yardstick {yard[worst]:.4f} ({worst}); structural zeros: {sorted(zeros)}")
    assert yard[worst] <= CAP, (worst, yard[worst])


def test_ids_are_readable_and_unique():
    ids = [c.id for c in E.CASES]
    assert len(set(ids)) == len(ids)
    assert {"fv0-hat2-b97-scaled", "fv3-hat2-b48-scaled", "fv0-conv1-b3-eval", "fv0-downsample2-b5", "fv1-stem-b4", "fv0-tail-b37"} <= set(ids)


def test_the_past_the_grid_batches_come_from_the_tile_width():
    """28 tiles per 56 px image against 512 workgroups, 8 per 28 px image against 256: the first batch with more work than grid."""
    assert E.conv3_tile_width() == 16
    assert E.B_PAST_GRID == {0: 19, 1: 33}
    for level, c in ((0, 64), (1, 128)):
        n = E.B_PAST_GRID[level]
        work, grid = E.conv3_direct_grid(n, E.RES[level], c)
        assert grid < work < 2 * grid and E.conv3_direct_grid(n - 1, E.RES[level], c)[0] <= grid
    assert E.conv3_direct_grid(3, 56, 96) is None and E.conv3_direct_grid(3, 56, 80) is None      # Cout % 64: the implicit GEMM
