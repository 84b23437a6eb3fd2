"""-m gpu: normal integration on the device (sp_normal_integration through frontend.normals.normals_integration) against the float64
restatement of its definition (tests/normal_integration_ref.py): solution parity with the direct solution measured against a float32 CG
of the same definition, the per-segment stopping rule, the output contract, and keyframes rebuilt from normals through the pair
optimiser.

Scenes: the masks of ``synth.make_pair(240, 320, 64, seed=11, shape='sam')`` with the plane's normals and with the curved analytic
surface of ``normal_integration_ref.curved_scene``; one full-frame mask (cg_tol 1e-3 only: float32 stalls on a whole frame below 1e-4).
"""
import functools

import numpy as np
import pytest
import torch

import normal_integration_ref as ref
from gpu_util import T, npy
from parity_util import pose_depth_errors

pytestmark = pytest.mark.gpu
H, W = 240, 320
DEPTH_BAR = 1e-3                 # the project's depth bar


def ni():
    from super_primitive_amd.frontend.normals import normals_integration
    return normals_integration


@functools.lru_cache(maxsize=None)
def sam_pair():
    from super_primitive_amd import synth
    return synth.make_pair(H, W, 64, seed=11, shape="sam")


@functools.lru_cache(maxsize=None)
def scene(name):
    """(normals (H,W,3) f32, K (3,3) f32, masks (N,H,W) bool) of a test scene."""
    from super_primitive_amd import synth
    pair = sam_pair()
    if name == "plane":
        return synth.plane_normals(pair), pair.K, pair.keypoint_regions
    n, K, _, _ = ref.curved_scene(H, W)
    assert np.allclose(K, pair.K)
    masks = pair.keypoint_regions if name == "curved" else np.ones((1, H, W), dtype=bool)
    assert name in ("curved", "frame")
    return n.astype(np.float32), K.astype(np.float32), masks


@functools.lru_cache(maxsize=None)
def systems(name):
    """Per segment (L, b, component labels, direct solution) of a scene, float64, from the float32 normals the device reads."""
    normals, K, masks = scene(name)
    out = []
    for m in masks:
        L, b, _ = ref.build_system(normals, K, m)
        lab = ref.component_labels(m)
        out.append((L, b, lab, ref.direct_solution(L, b, lab)))
    return out


@functools.lru_cache(maxsize=None)
def ref32(name, cg_tol, cg_max_iter):
    """The yardstick: the same CG in float32 on the host.  Per segment (error against the direct solution, iterations, |r| / |b|)."""
    out = []
    for L, b, lab, want in systems(name):
        u, k, res = ref.cg(L, b, cg_tol, cg_max_iter, dtype=np.float32)
        err = float(np.abs(ref.remove_component_means(u, lab) - want).max()) if b.size else 0.0
        out.append((err, k, res))
    return out


def device_run(name, cg_tol, cg_max_iter, **kw):
    normals, K, masks = scene(name)
    depth, info = ni().integrate_normals(T(normals), T(K), T(masks), cg_max_iter=cg_max_iter, cg_tol=cg_tol, return_info=True, **kw)
    torch.cuda.synchronize()
    return npy(depth), npy(info)


def device_errors(name, depth):
    """Per segment max |u_dev - u_direct| after removing the per-component means."""
    _, _, masks = scene(name)
    errs = []
    for m, d, (L, b, lab, want) in zip(masks, depth, systems(name)):
        u = np.log(d[m].astype(np.float64))
        errs.append(float(np.abs(ref.remove_component_means(u, lab) - want).max()))
    return np.array(errs)


def test_the_scene_is_the_one_the_bounds_were_reasoned_on():
    pair = sam_pair()
    sizes = pair.keypoint_regions.reshape(pair.N, -1).sum(1)
    assert pair.N == 70 and sizes.min() == 28 and sizes.max() == 9897
    assert abs(sizes.sum() / (H * W) - 1.1) < 0.05


@pytest.mark.parametrize("name,cg_tol", [("plane", 1e-3), ("plane", 1e-4), ("curved", 1e-3), ("curved", 1e-4), ("frame", 1e-3)])
def test_solution_parity_with_the_direct_solution(name, cg_tol):
    """max_k err_dev <= 3 x max_k err_ref32: the device against the float64 direct solution, measured by a float32 host CG of the same
    definition at the same settings.  Two host variants of the iteration (float32 / float64 dot products) end within 1.1 x of each
    other; a different reduction order deserves room beyond that; a wrong stencil, axis or sign shows as >= 1e-2 on the curved scene.
    At cg_tol 1e-3 every segment is also within the project's depth bar of the direct solution."""
    depth, info = device_run(name, cg_tol, 4000)
    err_dev = device_errors(name, depth)
    yard = np.array([e for e, _, _ in ref32(name, cg_tol, 4000)])
    big = np.argsort(-np.array([b.size for _, b, _, _ in systems(name)]))[:4]
    print(f"\n{name} cg_tol {cg_tol:g}: max err device {err_dev.max():.3g} (segment {err_dev.argmax()}), float32 host CG {yard.max():.3g} "
          f"(segment {yard.argmax()}); largest masks device {' '.join(f'{err_dev[k]:.2g}' for k in big)} | host {' '.join(f'{yard[k]:.2g}' for k in big)}; "
          f"iterations device max {int(info[:, 0].max())} host max {max(k for _, k, _ in ref32(name, cg_tol, 4000))}")
    assert (info[:, 0] >= 0).all() and (info[:, 0] < 4000).all()
    assert err_dev.max() <= 3.0 * yard.max(), (err_dev.max(), yard.max())
    if cg_tol == 1e-3:
        assert err_dev.max() <= DEPTH_BAR


@pytest.mark.parametrize("name,cg_tol", [("plane", 1e-3), ("curved", 1e-3), ("curved", 1e-4), ("frame", 1e-3)])
def test_iteration_counts_follow_the_float32_host_cg(name, cg_tol):
    """Per segment within +-5 % (at least +-3) of the host's float32 count, and the reported residual is at or below the tolerance."""
    _, info = device_run(name, cg_tol, 4000)
    want = np.array([k for _, k, _ in ref32(name, cg_tol, 4000)])
    got = info[:, 0].astype(np.int64)
    slack = np.maximum(3, np.ceil(0.05 * want))
    worst = np.abs(got - want) / np.maximum(want, 1)
    print(f"\n{name} cg_tol {cg_tol:g}: iterations device {got.min()}..{got.max()} host {want.min()}..{want.max()}, "
          f"largest difference {np.abs(got - want).max()} ({100 * worst.max():.1f} %)")
    assert (np.abs(got - want) <= slack).all(), list(zip(got[np.abs(got - want) > slack], want[np.abs(got - want) > slack]))
    assert (info[:, 1] <= cg_tol * (1 + 1e-6)).all() and (info[got > 0, 1] > 0).all()


def test_iteration_cap_and_degenerate_segments():
    """cap 10: the large masks use exactly 10 iterations and report a residual above the tolerance; an empty mask, a single pixel, pixels
    without a neighbour and all-zero normals take 0 iterations (|b| = 0), depth 1 on their pixels."""
    normals, K, masks = scene("curved")
    sizes = masks.reshape(len(masks), -1).sum(1)
    _, info = device_run("curved", 1e-3, 10)
    big = sizes > 1000
    assert big.sum() >= 5 and (info[big, 0] == 10).all() and (info[big, 1] > 1e-3).all()
    assert (info[:, 0] <= 10).all()
    want = np.array([k for _, k, _ in ref32("curved", 1e-3, 10)])
    assert (np.abs(info[:, 0] - want) <= 3).all()

    deg = np.zeros((4, H, W), dtype=bool)
    deg[1, 17, 23] = True
    deg[2, 5, 7] = deg[2, 6, 8] = deg[2, 100, 300] = True
    deg[3] = masks[int(sizes.argmax())]
    depth, info = ni().integrate_normals(T(normals), T(K), T(deg), cg_max_iter=100, cg_tol=1e-3, return_info=True)
    depth, info = npy(depth), npy(info)
    assert (info[:3] == 0).all() and info[3, 0] == 100
    assert not depth[0].any() and (depth[1][deg[1]] == 1).all() and (depth[2][deg[2]] == 1).all()
    assert not depth[1][~deg[1]].any() and not depth[2][~deg[2]].any()
    depth, info = ni().integrate_normals(T(np.zeros_like(normals)), T(K), T(deg), cg_max_iter=100, cg_tol=1e-3, return_info=True)
    assert (npy(info) == 0).all() and (npy(depth)[deg] == 1).all()


def test_output_contract_with_back_facing_grazing_and_border_normals():
    """0 outside the masks, finite and > 1e-7 inside -- also where normals face away from the camera or graze the ray, and for masks on the
    image border; sign-flipped normals give bitwise the same depth."""
    normals, K, masks = scene("curved")
    rng = np.random.default_rng(3)
    bad = normals.copy()
    flip = rng.uniform(size=(H, W)) < 0.3
    bad[flip] = -bad[flip]
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([(c - K[0, 2]) / K[0, 0], (r - K[1, 2]) / K[1, 1], np.ones_like(c)], -1)
    graze = np.cross(ray, [0.3, 1.0, 0.1])                       # orthogonal to the ray: n . ray = 0
    graze /= np.linalg.norm(graze, axis=-1, keepdims=True)
    patch = np.zeros((H, W), dtype=bool)
    patch[60:140, 90:200] = rng.uniform(size=(80, 110)) < 0.2
    mixed = np.where(patch[..., None], graze.astype(np.float32), normals)
    border = np.zeros((3, H, W), dtype=bool)
    border[0, :40, :] = True
    border[1, :, W - 25:] = True
    border[2, H - 1, :] = True
    border[2, :, 0] = True
    all_masks = np.concatenate([masks, border])
    base = ni().integrate_normals(T(normals), T(K), T(all_masks), cg_max_iter=300, cg_tol=1e-3)
    flipped = ni().integrate_normals(T(bad), T(K), T(all_masks), cg_max_iter=300, cg_tol=1e-3)
    assert torch.equal(base, flipped)
    for nrm in (normals, mixed):
        d = npy(ni().integrate_normals(T(nrm), T(K), T(all_masks), cg_max_iter=300, cg_tol=1e-3))
        assert np.isfinite(d).all() and (d[all_masks] > 1e-7).all() and not d[~all_masks].any()


def test_results_are_deterministic_and_independent_of_batch_box_hint_and_subsampling():
    from super_primitive_amd.optim.batch_prepare import segment_boxes_of
    normals, K, masks = scene("curved")
    n_t, K_t, m_t = T(normals), T(K), T(masks)
    a, ia = ni().integrate_normals(n_t, K_t, m_t, cg_max_iter=400, cg_tol=1e-4, return_info=True)
    b, ib = ni().integrate_normals(n_t, K_t, m_t, cg_max_iter=400, cg_tol=1e-4, return_info=True)
    assert torch.equal(a, b) and torch.equal(ia, ib)
    # a segment alone == the same segment inside the batch
    sizes = masks.reshape(len(masks), -1).sum(1)
    for k in (int(sizes.argmax()), int(sizes.argmin()), 17, len(masks) - 1):
        alone, ik = ni().integrate_normals(n_t, K_t, m_t[k:k + 1], cg_max_iter=400, cg_tol=1e-4, return_info=True)
        assert torch.equal(alone[0], a[k]) and torch.equal(ik[0], ia[k]), k
    # ... and in another order
    perm = torch.randperm(len(masks), generator=torch.Generator().manual_seed(0)).to(m_t.device)
    c, ic = ni().integrate_normals(n_t, K_t, m_t[perm], cg_max_iter=400, cg_tol=1e-4, return_info=True)
    assert torch.equal(c, a[perm]) and torch.equal(ic, ia[perm])
    # with the box hint (tight, and loose)
    boxes = segment_boxes_of(m_t)
    d, idd = ni().integrate_normals(n_t, K_t, m_t, boxes=boxes, cg_max_iter=400, cg_tol=1e-4, return_info=True)
    assert torch.equal(d, a) and torch.equal(idd, ia)
    loose = boxes + torch.tensor([-3, -5, 7, 2], dtype=torch.int32, device=boxes.device)
    e = ni().integrate_normals(n_t, K_t, m_t, boxes=loose, cg_max_iter=400, cg_tol=1e-4)
    assert torch.equal(e, a)
    # down_scale = 2 == the call on the subsampled inputs with the scaled K; float masks (what process_frame.py hands over) are fine
    half = ni().run_tiled_normal_integration(n_t, K, m_t.float(), down_scale=2, cg_max_iter=400, cg_tol=1e-4)
    K2 = K.copy()
    K2[:2] /= 2
    want = ni().integrate_normals(n_t[::2, ::2], T(K2), m_t[:, ::2, ::2], cg_max_iter=400, cg_tol=1e-4)
    assert half.shape == (len(masks), H // 2, W // 2) and torch.equal(half, want)
    full = ni().run_tiled_normal_integration(n_t, K_t, m_t, cg_max_iter=400, cg_tol=1e-4)
    assert torch.equal(full, a)


def test_two_lobes_have_zero_mean_each_and_are_split_into_two_segments():
    """CG from zero stays orthogonal to the null space: u has zero mean on every connected component (to float32 rounding: the mean of n
    values of size <= 0.5 accumulated over ~100 iterations, bound 1e-4 -- an offset between lobes that was not removed would be the
    lobes' log-depth difference, ~0.1).  kf_fix_disconnected_regions then makes two segments of the keyframe."""
    from super_primitive_amd import synth
    from super_primitive_amd.frontend.keyframe_assembly import keyframe_from_normals
    pair = sam_pair()
    normals = synth.plane_normals(pair)
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    lobe_a = ((c - 70) / 45.0) ** 2 + ((r - 80) / 30.0) ** 2 <= 1
    lobe_b = ((c - 240) / 50.0) ** 2 + ((r - 170) / 40.0) ** 2 <= 1
    mask = (lobe_a | lobe_b)[None]
    depth = npy(ni().integrate_normals(T(normals), T(pair.K), T(mask), cg_max_iter=2000, cg_tol=1e-4))[0]
    u = np.log(depth[mask[0]].astype(np.float64))
    for lobe in (lobe_a, lobe_b):
        assert abs(np.log(depth[lobe].astype(np.float64)).mean()) < 1e-4
    logz = np.log(pair.depth.astype(np.float64))
    for lobe in (lobe_a, lobe_b):
        d = np.log(depth[lobe].astype(np.float64)) - logz[lobe]
        assert np.abs(d - d.mean()).max() < DEPTH_BAR
    kp = np.array([[2.0 * 80 / (H - 1) - 1, 2.0 * 70 / (W - 1) - 1]], dtype=np.float32)
    kf = keyframe_from_normals(T(pair.src_image), T(pair.K), T(normals), T(mask), T(kp), cg_max_iter=2000, cg_tol=1e-4)
    assert kf.num_segments() == 2
    regions = npy(kf.keypoint_regions)
    assert sorted(int(x) for x in regions.reshape(2, -1).sum(1)) == sorted([int(lobe_a.sum()), int(lobe_b.sum())])
    assert kf.segment_boxes is not None and tuple(kf.segment_boxes.shape) == (2, 4)
    whole = keyframe_from_normals(T(pair.src_image), T(pair.K), T(normals), T(mask), T(kp), cg_max_iter=2000, cg_tol=1e-4,
                                  split_disconnected=False)
    assert whole.num_segments() == 1 and torch.equal(whole.keypoint_regions[0], T(mask[0]))


def test_keyframe_from_normals_resizes_to_the_keyframe_size():
    """Integration at 240 x 320, keyframe at 120 x 160 (process_frame.py:231-236): intrinsics scaled for the integration, the depth brought
    down by nearest resize; every segment's log-depth is the ground truth of the small frame up to a constant."""
    from super_primitive_amd import synth
    from super_primitive_amd.frontend.keyframe_assembly import keyframe_from_normals
    big = sam_pair()
    small = synth.make_pair(H // 2, W // 2, 6, seed=11)                  # the same plane and camera at half size
    sizes = big.keypoint_regions.reshape(big.N, -1).sum(1)
    pick = np.argsort(-sizes)[:12]
    masks = big.keypoint_regions[pick]
    kf = keyframe_from_normals(T(small.src_image), T(small.K), T(synth.plane_normals(big)), T(masks), T(big.keypoints[pick]),
                               cg_max_iter=2000, cg_tol=1e-4, split_disconnected=False)
    assert tuple(kf.logdepth_perseg.shape) == (12, H // 2, W // 2) and kf.num_segments() == 12
    L, regions = npy(kf.logdepth_perseg).astype(np.float64), npy(kf.keypoint_regions)
    assert not L[~regions].any()
    # nearest resize picks source pixel (2 r, 2 c), whose ray ((2 c - 160) / 256, (2 r - 120) / 256) IS the small frame's ray of (r, c)
    logz = np.log(small.depth.astype(np.float64))
    for k in range(12):
        d = L[k][regions[k]] - logz[regions[k]]
        assert np.abs(d - d.mean()).max() < DEPTH_BAR, k


def test_pairs_with_the_source_keyframe_rebuilt_from_normals_end_where_the_stock_pairs_end():
    """Stock synth pairs (grid and blobs) against the same pairs whose source keyframe comes from keyframe_from_normals (plane normals,
    cg_tol 1e-4): the log-depth field is the stock one up to a constant per segment, and the scheduled pair optimiser gives the same verdict
    and an end state within the project's bar (1e-4 rad / 1e-4 t / 1e-3 depth, gauge removed) of the stock pairs'."""
    from super_primitive_amd import synth
    from super_primitive_amd.frontend.keyframe_assembly import keyframe_from_normals
    from super_primitive_amd.optim.pair_batch import FRAME_PAIR_SCHEDULE, PairBatch
    # (the pairs of test_gpu_pairs.py's slot-queue tests: 96 x 128, grid with overlapping tiles and ragged blobs)
    pairs = [synth.make_pair(96, 128, 6, seed=120, init_sigma=0.002, overlap=2), synth.make_pair(96, 128, 6, seed=122, init_sigma=0.004, overlap=2),
             synth.make_pair(96, 128, 5, seed=150, init_sigma=0.002, shape="blobs", blob_coverage=0.9),
             synth.make_pair(96, 128, 11, seed=152, init_sigma=0.004, shape="blobs", blob_coverage=1.2)]
    srcs = []
    for p in pairs:
        normals = synth.plane_normals(p)
        kf = keyframe_from_normals(T(p.src_image), T(p.K), T(normals), T(p.keypoint_regions), T(p.keypoints), cg_max_iter=4000, cg_tol=1e-4,
                                   split_disconnected=False)
        assert kf.num_segments() == p.N and torch.equal(kf.keypoint_regions, T(p.keypoint_regions))
        np.testing.assert_allclose(npy(kf.keypoints), p.keypoints, atol=1e-6)
        # the field: stock up to a constant per segment, within the solution-parity error (3 x the float32 host CG's, plus the 2e-6 that
        # the stock field itself is from the direct solution: test_normal_integration_host.py)
        L_new, yard, worst = npy(kf.logdepth_perseg).astype(np.float64), 0.0, 0.0
        for k in range(p.N):
            m = p.keypoint_regions[k]
            Lk, bk, _ = ref.build_system(normals, p.K, m)
            lab = ref.component_labels(m)
            assert lab.max() == 1
            u32, _, _ = ref.cg(Lk, bk, 1e-4, 4000, dtype=np.float32)
            yard = max(yard, float(np.abs(ref.remove_component_means(u32, lab) - ref.direct_solution(Lk, bk, lab)).max()))
            d = L_new[k][m] - p.logdepth_perseg[k][m].astype(np.float64)
            worst = max(worst, float(np.abs(d - d.mean()).max()))
        print(f"\n{p.H}x{p.W}x{p.N} {p.meta['shape']}: rebuilt field vs stock, constant removed {worst:.3g}; float32 host CG vs direct {yard:.3g}")
        assert worst <= 3.0 * yard + 2e-6
        srcs.append(kf)
    kw = {k: v for k, v in FRAME_PAIR_SCHEDULE.items() if k != "check_every"}
    stock = PairBatch.from_synth(pairs, levels=(0, 3), device="cuda:0")
    rebuilt = PairBatch(srcs, [T(p.trg_image) for p in pairs], [T(p.K) for p in pairs], torch.stack([T(p.pose_init) for p in pairs]),
                        [T(p.kld_init) for p in pairs], levels=(0, 3))
    for b in (stock, rebuilt):
        b.run_scheduled(**kw)
    torch.cuda.synchronize()
    assert torch.equal(stock.failed(), rebuilt.failed())
    for m, p in enumerate(pairs):
        e = pose_depth_errors(npy(rebuilt.poses()[m]), npy(rebuilt.klds()[m]), npy(stock.poses()[m]), npy(stock.klds()[m]))
        print(f"pair {m}: rebuilt vs stock end state rot {e[0]:.2g} t {e[1]:.2g} depth {e[2]:.2g}; failed {bool(stock.failed()[m])}")
        assert e[0] <= 1e-4 and e[1] <= 1e-4 and e[2] <= DEPTH_BAR, (m, e)
