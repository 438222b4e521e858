"""No-GPU checks of the layer-geometry list (tests/_layer_shapes.py) that tests/test_layer_shapes_gpu.py runs the depthwise, stem
and squeeze-excite kernels at: its size per configuration, the hard cases it must hold, and the host-side planners' answers."""

from __future__ import annotations

import ctypes

import pytest

from deepfakedetection_amd import _lib
from tests import _layer_shapes as S


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        from deepfakedetection_amd.build import build

        build()
    return _lib.load()


# distinct (stem, depthwise, squeeze-excite) geometries; B3 has 14 depthwise geometries in 26 blocks, EfficientFormerV2 10
COUNTS = {
    "b0_timm_224": (1, 12, 10), "b0_timm_160": (1, 12, 10),
    "b3_lukemelas_224": (1, 14, 12), "b3_lukemelas_160": (1, 14, 12), "b3_lukemelas_300": (1, 14, 12),
    "efficientformerv2_s0_224": (1, 10, 0), "efficientformerv2_s0_160": (1, 10, 0),
    "efficientformerv2_s1_224": (1, 10, 0), "efficientformerv2_s1_160": (1, 10, 0),
    "efficientformerv2_s2_224": (1, 10, 0), "efficientformerv2_s2_160": (1, 10, 0),
}


def test_counts_per_configuration():
    assert set(COUNTS) == set(S.CONFIGS)
    for name, want in COUNTS.items():
        stems, dws, ses = S.config_geometries(name)
        assert (len(stems), len(dws), len(ses)) == want, name
    stems, dws, ses = S.config_layers("b3_lukemelas_224")
    assert (len(stems), len(dws), len(ses)) == (1, 26, 26)
    stems, dws, ses = S.config_layers("efficientformerv2_s2_224")
    # mid layers, attention of stage 2 (stride_conv + v_local) and of stage 3 (v_local), the downsampling's local_q + v_local
    assert len(dws) == (4 + 4 + 12 + 8) + 4 * 2 + 4 + 2
    stems, dws, ses = S.all_geometries()
    assert (len(stems), len(dws), len(ses)) == (7, 112, 53)


def test_geometries_are_consistent():
    for name in S.CONFIGS:
        stems, dws, ses = S.config_layers(name)
        for g in stems:
            assert (g.k, g.stride, g.pt, g.pl) in ((3, 2, 0, 0), (3, 2, 1, 1)) and (g.H, g.Ho) == (g.W, g.Wo) and g.Cout % 8 == 0
            assert g.Ho == -(-g.H // 2)
        for g in dws:
            assert g.k in (3, 5) and g.stride in (1, 2) and g.C % 8 == 0 and g.pt == g.pl and (g.H, g.Ho) == (g.W, g.Wo)
            # the input rows the last output row reads exist, and the padding the oracle adds below stays under one kernel
            assert 0 <= (g.Ho - 1) * g.stride - g.pt <= g.H - 1
            assert 0 <= (g.Ho - 1) * g.stride + g.k - g.pt - g.H < g.k
            assert g.pro in (None, "silu") and g.epi in (None, "silu", "gelu") and (g.stats or g.epi is None)
        assert all(g.C % 8 == 0 and g.R >= 1 for g in ses)


def test_known_hard_cases_are_in_the_list():
    b3_224 = S.config_geometries("b3_lukemelas_224")
    # TF-SAME padding frozen at 300 px on 224 px maps: stride-2 3x3 layers with pads (0, 1), i.e. no top / left padding
    assert [g.geom for g in b3_224[1] if g.stride == 2 and g.pt == 0] == [(112, 112, 144, 3, 2, 0, 0, 56, 56), (28, 28, 288, 3, 2, 0, 0, 14, 14)]
    assert b3_224[0] == [S.Stem(224, 224, 40, 3, 2, 0, 0, 112, 112)]
    # 5x5 kernels on 5x5 maps at 160 px (the whole map inside one tap window), and the stride-2 5x5 layer that makes them
    for name, C in (("b0_timm_160", 1152), ("b3_lukemelas_160", 1392)):
        geoms = [g.geom for g in S.config_geometries(name)[1]]
        assert (5, 5, C, 5, 1, 2, 2, 5, 5) in geoms, name
        assert any(g[:2] == (10, 10) and g[3:5] == (5, 2) and g[7] == 5 for g in geoms), name
    # odd maps: 75 / 19 at 300 px, 7 at 224, 5 at 160
    for name, odd in (("b3_lukemelas_300", {75, 19}), ("b0_timm_224", {7}), ("efficientformerv2_s1_160", {5})):
        assert odd <= {g.H for g in S.config_geometries(name)[1] if g.H % 2}, name
    # B3 at 300 px: stride-2 5x5 on a 19 px map (pads (2, 2) from the nominal size: 10 output rows)
    assert (19, 19, 816, 5, 2, 2, 2, 10, 10) in [g.geom for g in S.config_geometries("b3_lukemelas_300")[1]]
    # the three call patterns of EfficientFormerV2: ConvMlp mid (GELU epilogue), BN'd local convolutions, the plain local_q
    s1 = S.config_geometries("efficientformerv2_s1_224")[1]
    assert (7, 7, 896, 3, 1, 1, 1, 7, 7, None, "gelu", True, False) in s1
    assert (14, 14, 120, 3, 2, 1, 1, 7, 7, None, None, True, False) in s1
    assert (14, 14, 120, 3, 2, 1, 1, 7, 7, None, None, False, False) in s1


def test_matrix_core_planner_takes_every_geometry_without_a_gpu(lib):
    """dfd_dw_mm_plan (host side only) accepts every bf16 geometry with C % 16 == 0, with and without the prologue the model
    uses, at the batch of the tests and of the benchmark."""
    plan = (ctypes.c_int * 12)()
    stems, dws, ses = S.all_geometries()
    mm = [g for g in dws if g.C % 16 == 0]
    assert len(mm) == 100
    for g in mm:
        for n in (2, 256):
            shp = _lib.DwShape(n, g.H, g.W, g.C, g.Ho, g.Wo, g.k, g.stride, g.pt, g.pl)
            assert lib.dfd_dw_mm_plan(ctypes.byref(shp), 1 if g.pro else 0, plan) == 0, (n, g)
            assert plan[8] >= 1, (n, g)                     # work items


def test_eval_form_planner_takes_every_geometry_without_a_gpu(lib):
    """dfd_dwconv_fwd_eval_tiles (the vector-unit tile planner dfd_dwq_geom behind the inference form) accepts every EfficientNet
    geometry in f32 and bf16: a declined one would raise in kernels.dwconv_eval.  Its tiles cover the output map."""
    stems, dws, ses = S.all_geometries()
    for g in [g for g in dws if g.eval]:
        shp = _lib.DwShape(2, g.H, g.W, g.C, g.Ho, g.Wo, g.k, g.stride, g.pt, g.pl)
        for dt in (_lib.F32, _lib.BF16):
            tiles = lib.dfd_dwconv_fwd_eval_tiles(dt, ctypes.byref(shp))
            assert 1 <= tiles <= g.Ho * -(-g.Wo // 4), (dt, g)
