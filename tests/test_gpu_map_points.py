"""-m gpu: ``sp_map_points`` (csrc/sp_results.hip) through ``odometery.results.keyframe_points`` -- the coloured world points of several
keyframes of different sizes in ONE launch: row <-> pixel correspondence against ``torch.nonzero`` of the masks, colours and (identity
pose, no alignment) points bitwise, aligned points against the float64 formula at a bound derived per point."""
import numpy as np
import pytest
import torch

import traj_align_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

STRIDES = [1, 3, 4, 1000]          # (3, 4 and 1000 exceed B's single point; 1000 exceeds every keyframe's: one row each)


def _keyframe(H, W, masks, seed):
    """A KeyFrame whose image value identifies its pixel: image[ch, r, c] = (ch H W + r W + c + 1) / 4096, exact in float32."""
    from super_primitive_amd.image.keyframe import KeyFrame
    rng = np.random.default_rng(seed)
    N = masks.shape[0]
    image = ((np.arange(3 * H * W, dtype=np.float32) + 1.0) / 4096.0).reshape(3, H, W)
    K = np.array([[0.9 * W, 0, 0.5 * W - 0.25], [0, 0.95 * W, 0.5 * H + 0.5], [0, 0, 1]], dtype=np.float32)
    L = (0.3 * rng.standard_normal((N, H, W)) + 0.8).astype(np.float32) * masks
    keypoints = np.zeros((N, 2), dtype=np.float32)
    for n in range(N):
        rc = np.argwhere(masks[n])
        r, c = rc[len(rc) // 2] if len(rc) else (0, 0)
        keypoints[n] = (2.0 * r / (H - 1) - 1.0, 2.0 * c / (W - 1) - 1.0)
    kld = (0.2 * rng.standard_normal(N) + 0.5).astype(np.float32)
    return KeyFrame(T(image), T(K), T(L), T(keypoints), T(masks)), T(kld)


def _scene():
    """A: 12x20, 3 segments, one empty, two overlapping.  B: 9x7, one single-pixel segment.  C: 24x40, 2 segments of 500 + 270 = 770
    points: ceil(770 / 3) = 257 rows, so at stride 3 its last workgroup holds ONE row."""
    A = np.zeros((3, 12, 20), dtype=bool)
    A[0, 2:9, 3:12] = True
    A[2, 5:11, 8:17] = True                                   # overlaps segment 0 on rows 5-8, columns 8-11; segment 1 is empty
    B = np.zeros((1, 9, 7), dtype=bool)
    B[0, 4, 5] = True
    C = np.zeros((2, 24, 40), dtype=bool)
    C.reshape(2, -1)[0, 100:600] = True
    C.reshape(2, -1)[1, 37:37 + 540:2] = True
    assert A[1].sum() == 0 and (A[0] & A[2]).sum() == 16 and C.sum() == 770
    kfs, klds = zip(*[_keyframe(m.shape[1], m.shape[2], m, 50 + k) for k, m in enumerate((A, B, C))])
    return list(kfs), list(klds), [A, B, C]


def _pose(rng):
    from scipy.spatial.transform import Rotation
    Tm = np.eye(4)
    Tm[:3, :3] = Rotation.from_rotvec(rng.uniform(-1.2, 1.2, 3)).as_matrix()
    Tm[:3, 3] = rng.uniform(-2.0, 2.0, 3)
    return Tm.astype(np.float32)


@pytest.fixture(scope="module")
def scene():
    return _scene()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("stride", STRIDES)
def test_rows_pixels_colours_and_camera_points(scene, stride):
    from super_primitive_amd.core.dense_optim import unproject_kf
    from super_primitive_amd.odometery.results import keyframe_points
    kfs, klds, masks = scene
    eye = torch.eye(4, device="cuda").repeat(3, 1, 1)
    out = keyframe_points(kfs, klds, eye, stride=stride)
    torch.cuda.synchronize()
    P = [int(m.sum()) for m in masks]
    Q = [-(-p // stride) for p in P]
    assert out['offsets'].tolist() == np.concatenate(([0], np.cumsum(Q))).tolist()
    assert out['points'].shape == (sum(Q), 3) and out['colours'].shape == (sum(Q), 3)
    assert out['kf_index'].dtype == torch.int32 and out['seg_ids'].dtype == torch.int32
    if stride == 3:
        assert Q[2] == 257
    for k, (kf, kld) in enumerate(zip(kfs, klds)):
        a, b = int(out['offsets'][k]), int(out['offsets'][k + 1])
        nz = torch.nonzero(kf.keypoint_regions)[::stride]                    # (segment, row, column) of every reported table point
        assert b - a == nz.shape[0]
        assert bool((out['kf_index'][a:b] == k).all())
        assert torch.equal(out['seg_ids'][a:b].long(), nz[:, 0])
        want_rgb = kf.image[:, nz[:, 1], nz[:, 2]].t()
        assert torch.equal(_bits(out['colours'][a:b]), _bits(want_rgb)), f"keyframe {k}: colours"
        src = unproject_kf(kf, kld)
        assert torch.equal(_bits(out['points'][a:b]), _bits(src['src_pts'][::stride])), f"keyframe {k}: points under the identity pose"
        assert torch.equal(out['seg_ids'][a:b].long(), src['segm_ids'][::stride])


@pytest.mark.parametrize("stride", [1, 3])
def test_world_points_with_poses_and_alignment(scene, stride):
    from super_primitive_amd.core.dense_optim import unproject_kf
    from super_primitive_amd.odometery.results import keyframe_points
    from super_primitive_amd.tool.pose_utils import record_views
    kfs, klds, _ = scene
    rng = np.random.default_rng(7)
    poses = np.stack([_pose(rng) for _ in kfs])
    # two alignment records written by hand: s != 1, rot_reanchor != I
    record = np.zeros((2, 32))
    recs = []
    for r in range(2):
        rec = dict(rot=_pose(rng)[:3, :3].astype(np.float64), trans_scaled=rng.uniform(-3, 3, 3), s=(0.37, 2.6)[r],
                   rot_reanchor=_pose(rng)[:3, :3].astype(np.float64))
        record[r, 0:9], record[r, 9:12], record[r, 15], record[r, 16:25] = rec['rot'].reshape(-1), rec['trans_scaled'], rec['s'], rec['rot_reanchor'].reshape(-1)
        recs.append(rec)
    record_d = T(record)
    views = record_views(record_d)
    np.testing.assert_array_equal(npy(views['rot_reanchor'][1]), recs[1]['rot_reanchor'])
    np.testing.assert_array_equal(npy(views['s']), [0.37, 2.6])
    index = [1, -1, 0]                                                       # A by record 1, B not aligned, C by record 0
    out = keyframe_points(kfs, klds, T(poses), stride=stride, align=record_d, align_index=index)
    torch.cuda.synchronize()
    worst = 0.0
    for k, (kf, kld) in enumerate(zip(kfs, klds)):
        a, b = int(out['offsets'][k]), int(out['offsets'][k + 1])
        p = npy(unproject_kf(kf, kld)['src_pts'][::stride])                  # (bitwise the kernel's camera points: the test above)
        want, bound = ref.world_points(p, poses[k], recs[index[k]] if index[k] >= 0 else None)
        err = np.abs(npy(out['points'][a:b]).astype(np.float64) - want).max(1)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (k, float((err / bound).max()))
    print(f"\nstride {stride}: largest error of an aligned world point, in units of its bound 8 * 2^-24 (s |p|_1 + |t'|_inf): {worst:.3f}")
    # every keyframe by one record: the default of ``align`` without ``align_index``
    out0 = keyframe_points(kfs, klds, T(poses), stride=stride, align=dict(record=record_d[:1].contiguous()))
    a, b = int(out['offsets'][2]), int(out['offsets'][3])
    assert torch.equal(out0['points'][a:b], out['points'][a:b])


def test_keyframe_without_pixels_and_bad_arguments(scene):
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.odometery.results import keyframe_points
    kfs, klds, _ = scene
    empty, kld = _keyframe(6, 8, np.zeros((2, 6, 8), dtype=bool), 3)
    eye = torch.eye(4, device="cuda")
    with pytest.raises(ValueError, match="no segment pixels"):
        keyframe_points([kfs[0], empty], [klds[0], kld], eye.repeat(2, 1, 1))
    with pytest.raises(ValueError):
        keyframe_points(kfs[:1], klds[:1], eye[None], stride=0)
    with pytest.raises(ValueError):
        keyframe_points(kfs[:1], klds[:1], eye[None], align_index=[0])             # no record to index
    with pytest.raises(ValueError):
        keyframe_points(kfs[:1], klds[:2], eye[None])
    half = KeyFrame(kfs[0].image[:, ::2, ::2].contiguous(), kfs[0].K, kfs[0].logdepth_perseg, kfs[0].keypoints, kfs[0].keypoint_regions)
    with pytest.raises(ValueError, match="image"):
        keyframe_points([half], klds[:1], eye[None])
    with pytest.raises(RuntimeError, match="HIP-only"):
        keyframe_points(kfs[:1], klds[:1], torch.eye(4)[None])
