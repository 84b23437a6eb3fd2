"""Normal integration without a GPU: the float64 yardstick (tests/normal_integration_ref.py) against analytic surfaces, the
properties of the definition, and the host side of the new entry points (header / ctypes table / library, module aliasing,
host tensors refused)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import normal_integration_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sp_normal_integration_plan_words", "sp_normal_integration_segment_floats", "sp_normal_integration_plan",
               "sp_normal_integration")


def test_plane_direct_solution_is_the_ground_truth_logdepth():
    """The synth plane on SAM-shaped masks: the direct solution is the ground-truth log-depth up to one constant per segment, and so is
    the field synth fakes (``logdepth_perseg``).  Bound: for a plane the two halves of an edge's energy err by +-a eps^2 / 2 with
    eps = nx / (fx d) ~ 1e-3 and cancel, leaving O(eps^3) ~ 1e-9 per edge, i.e. < 1e-6 over a 300-pixel path; the float32 ``depth`` field
    adds 1.2e-7.  A wrong stencil, axis or sign shows as >= 1e-2."""
    from super_primitive_amd import synth
    pair = synth.make_pair(120, 160, 24, seed=11, shape="sam")
    normals = synth.plane_normals(pair)
    assert np.allclose(normals[0, 0], ref.plane_normal_of_pair(pair), atol=1e-7)
    logz = np.log(pair.depth.astype(np.float64))
    worst = worst_fake = 0.0
    for k in range(pair.N):
        m = pair.keypoint_regions[k]
        L, b, index = ref.build_system(normals, pair.K, m)
        lab = ref.component_labels(m)
        u = ref.direct_solution(L, b, lab)
        worst = max(worst, float(np.abs(u - ref.remove_component_means(logz[m], lab)).max()))
        fake = pair.logdepth_perseg[k][m].astype(np.float64)
        worst_fake = max(worst_fake, float(np.abs(u - ref.remove_component_means(fake, lab)).max()))
    print(f"plane: direct solution vs ground truth {worst:.3g}, vs synth's logdepth_perseg {worst_fake:.3g}")
    assert worst <= 2e-6 and worst_fake <= 2e-6


def test_curved_surface_converges_at_second_order():
    """log z = -log(n0 . ray) + g on an ellipse with an elliptic hole: the error of the direct solution falls by >= 3 x per doubling of
    the resolution (a second-order scheme gives 4 x)."""
    errs = []
    for H, W in ((120, 160), (240, 320), (480, 640)):
        n, K, logz, mask = ref.curved_scene(H, W)
        L, b, index = ref.build_system(n, K, mask)
        lab = ref.component_labels(mask)
        assert lab.max() == 1
        u = ref.direct_solution(L, b, lab)
        errs.append(float(np.abs(u - ref.remove_component_means(logz[mask], lab)).max()))
    print("curved surface, max error at 120x160 / 240x320 / 480x640:", " / ".join(f"{e:.3g}" for e in errs),
          "ratios", f"{errs[0] / errs[1]:.2f} {errs[1] / errs[2]:.2f}")
    assert errs[0] / errs[1] >= 3.0 and errs[1] / errs[2] >= 3.0
    assert errs[1] < 1e-2            # (and it is the right surface, not merely a convergent one)


def test_cg_restatement_reaches_the_direct_solution():
    n, K, logz, mask = ref.curved_scene(60, 80)
    L, b, index = ref.build_system(n, K, mask)
    lab = ref.component_labels(mask)
    want = ref.direct_solution(L, b, lab)
    u, k, res = ref.cg(L, b, 1e-10, 5000, dtype=np.float64)
    assert 0 < k < 5000 and res <= 1e-10
    assert np.abs(ref.remove_component_means(u, lab) - want).max() < 1e-8
    assert abs(u.mean()) < 1e-10                      # CG from zero stays orthogonal to the null space
    u32, k32, res32 = ref.cg(L, b, 1e-3, 5000, dtype=np.float32)
    assert 0 < k32 < k and res32 <= 1e-3


def test_sign_flipped_normals_give_the_identical_system():
    n, K, logz, mask = ref.curved_scene(48, 64)
    flip = np.random.default_rng(0).uniform(size=mask.shape) < 0.5
    n2 = np.where(flip[..., None], -n, n)
    L1, b1, _ = ref.build_system(n, K, mask)
    L2, b2, _ = ref.build_system(n2, K, mask)
    assert (L1 != L2).nnz == 0 and np.array_equal(b1, b2)


def test_degenerate_segments_have_zero_right_hand_side():
    n, K, logz, _ = ref.curved_scene(24, 32)
    lone = np.zeros((24, 32), dtype=bool)
    lone[5, 7] = lone[9, 20] = lone[10, 21] = True               # three pixels, no two 4-adjacent
    L, b, index = ref.build_system(n, K, lone)
    assert b.shape == (3,) and not b.any() and L.nnz == 0
    assert ref.cg(L, b, 1e-3, 100)[1] == 0
    L, b, index = ref.build_system(n, K, np.zeros((24, 32), dtype=bool))
    assert b.shape == (0,) and ref.cg(L, b, 1e-3, 100)[1] == 0
    block = np.zeros((24, 32), dtype=bool)
    block[4:12, 6:20] = True
    L, b, index = ref.build_system(np.zeros_like(n), K, block)
    assert not b.any() and not L.data.any()
    u, k, _ = ref.cg(L, b, 1e-3, 100)
    assert k == 0 and not u.any()


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp_hip.h")).read()
    assert "frontend/normals/normals_integration.py:7-28" in header and "frontend/process_frame.py:78-92" in header
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
    # the N2 block comes first, the new section after it
    assert header.index("int sp_kth_mask_pixel(") < header.index("int sp_normal_integration_plan_words(")


def test_size_queries_and_argument_checks():
    """Everything the entry points refuse is refused before any device work, so this runs without a GPU."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    assert lib.sp_normal_integration_plan_words(0) == -1 and lib.sp_normal_integration_plan_words(70000) == -2
    w = lib.sp_normal_integration_plan_words(300)
    assert w >= 4 + 9 * 300 and w % 16 == 0
    f = lib.sp_normal_integration_segment_floats(240, 320)
    assert f % 16 == 0 and 6 * (240 + 2) * 320 <= f <= 6 * (240 + 2) * 320 + 6 * 16      # six vectors of the frame plus two guard rows
    assert lib.sp_normal_integration_segment_floats(0, 5) == -1 and lib.sp_normal_integration_segment_floats(40000, 8) == -2
    one = ctypes.c_void_p(16)                                                               # any non-null address: never dereferenced
    assert lib.sp_normal_integration(None, one, one, None, 1, 8, 8, 10, 1e-3, 0, one, 1 << 20, one, one, None) == -1
    assert lib.sp_normal_integration(one, one, one, None, 1, 8, 8, 10, 1e-3, 1, one, 1 << 20, one, one, None) == -1     # reserved flags
    assert lib.sp_normal_integration(one, one, one, None, 1, 8, 8, 10, 1e-3, 0, one, 8, one, one, None) == -1           # scratch < plan
    assert lib.sp_normal_integration(one, one, one, None, 1, 8, 8, -1, 1e-3, 0, one, 1 << 20, one, one, None) == -1
    assert lib.sp_normal_integration(one, one, one, None, 70000, 8, 8, 10, 1e-3, 0, one, 1 << 30, one, one, None) == -2
    assert lib.sp_normal_integration_plan(None, None, 1, 8, 8, one, None) == -1


def test_host_tensors_are_refused():
    from super_primitive_amd.frontend.normals import normals_integration as ni
    from super_primitive_amd.frontend.keyframe_assembly import keyframe_from_normals
    normals = torch.zeros(8, 8, 3)
    normals[..., 2] = 1
    masks = torch.ones(1, 8, 8, dtype=torch.bool)
    K = np.array([[8.0, 0, 4], [0, 8, 4], [0, 0, 1]], dtype=np.float32)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ni.integrate_normals(normals, K, masks)
    with pytest.raises(RuntimeError, match="HIP-only"):
        ni.run_tiled_normal_integration(normals, K, masks, down_scale=2)
    with pytest.raises(RuntimeError, match="HIP-only"):
        keyframe_from_normals(torch.zeros(3, 8, 8), K, normals, masks, torch.zeros(1, 2), cg_max_iter=10, cg_tol=1e-3)


def test_reference_module_path_resolves_to_the_hip_integrator():
    import super_primitive_amd
    from super_primitive_amd.frontend.normals import normals_integration as ours
    saved = dict(sys.modules)
    try:
        super_primitive_amd.install_as_reference_modules()
        import frontend.normals.normals_integration as theirs
        assert theirs is ours
        import inspect
        assert list(inspect.signature(theirs.run_tiled_normal_integration).parameters) == \
            ["normals", "intrinsics", "mask", "down_scale", "cg_max_iter", "cg_tol"]
        sig = inspect.signature(theirs.run_tiled_normal_integration)
        assert (sig.parameters["down_scale"].default, sig.parameters["cg_max_iter"].default, sig.parameters["cg_tol"].default) == (1, 1000, 1e-3)
        import frontend.segment.post_processer as pp
        from super_primitive_amd.frontend.segment import post_processer
        assert pp is post_processer
    finally:
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)


def test_synth_plane_normals_reproduce_the_rendered_depth():
    """The helper's normal is the plane the pair was rendered from: depth = h / (n . ray) with h = 3."""
    from super_primitive_amd import synth
    pair = synth.make_pair(30, 40, 6, seed=5)
    n = synth.plane_normals(pair)
    assert n.shape == (30, 40, 3) and n.dtype == np.float32
    K = pair.K.astype(np.float64)
    c, r = np.meshgrid(np.arange(40.0), np.arange(30.0))
    ray = np.stack([(c - K[0, 2]) / K[0, 0], (r - K[1, 2]) / K[1, 1], np.ones_like(c)], -1)
    np.testing.assert_allclose(3.0 / (ray * n.astype(np.float64)).sum(-1), pair.depth, rtol=1e-6)
