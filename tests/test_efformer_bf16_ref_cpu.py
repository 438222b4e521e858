"""The reference side of tests/test_efformer_bf16_gpu.py on its own, without a GPU (tests/_efformer_bwd_ref.py): for every case
the float64 dictionary has the expected keys, the structurally zero gradients are exactly the names the arithmetic predicts, a
scaled case's row scales hold both 0 and 1.25 (with images 1 and N - 1 dropped), and no yardstick exceeds 0.15.

The cap is a condition of the GPU test: its bound is 2 * yardstick + 2e-3, and a yardstick near 0.5 would let anything pass.  The
largest yardsticks are those of mlp.fc1.bn of the ConvMlp blocks at 197,568 rows (gradients that nearly cancel over that many
rows); everything else is 0.1 .. 3 %.  A seed that pushes a yardstick over the cap is changed; the cap is not.
"""

from __future__ import annotations

import pytest
import torch

from tests import _efformer_bwd_ref as E

CAP = 0.15


@pytest.mark.parametrize("case", E.CASES, ids=[c.id for c in E.CASES])
def test_reference_of_the_case(case):
    inp = E.inputs(case)
    ref, yard, zeros = E.reference(case)
    params = [n for n, _ in inp.mod.named_parameters()]
    assert set(ref) == {"out", *params} | ({"x.grad"} if case.kind != "stem" else set())
    assert set(yard) == set(ref)
    assert all(bool(torch.isfinite(t).all()) and t.dtype == torch.float64 for t in ref.values())
    assert tuple(ref["out"].shape) == tuple(E.nchw(inp.g).shape)
    assert set(zeros) == E.expected_zeros(case, params), set(zeros) ^ E.expected_zeros(case, params)
    assert E.exact_zeros(case, params) <= set(zeros)
    for n in set(ref) - set(zeros):                                      # everything else carries signal: nothing is judged against noise
        assert float(ref[n].abs().max()) > 0.0, n
        if n.endswith("bias") and E.sibling(n) in ref:
            assert float(ref[n].abs().max()) > 1e-4 * float(ref[E.sibling(n)].abs().max()), n
    if case.kind == "block":
        assert (inp.masks is not None) == case.scaled
        assert (inp.mod.token_mixer is not None) == inp.attention
    for m in (inp.masks or ()):
        if m is not None:
            assert m.shape == (case.n,) and set(m.tolist()) == {0.0, 1.25} and m[1] == 0.0 and m[case.n - 1] == 0.0
    if inp.masks is not None and inp.masks[0] is not None:
        a, b = inp.masks
        assert bool(((a == 0) & (b != 0)).any()) and bool(((a != 0) & (b == 0)).any())     # the two branches do not share a scale
    if inp.u is not None:
        assert 0.1 < float((inp.u < E.P_DROP).float().mean()) < 0.3
    worst = max(yard, key=yard.get)
    print(f"{case.id}: largest yardstick {yard[worst]:.4f} ({worst}); structural zeros: {sorted(zeros)}")
    assert yard[worst] <= CAP, (worst, yard[worst])


def test_ids_are_readable_and_unique():
    ids = [c.id for c in E.CASES]
    assert len(set(ids)) == len(ids)
    assert "s1-block2.7-n37-scaled" in ids and "s1-block2.7-n37-eval" in ids and "s1-tail-n37-dropout" in ids
