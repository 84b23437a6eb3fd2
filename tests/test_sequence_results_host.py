"""CPU-only: the float64 restatement of the trajectory alignment (tests/traj_align_ref.py) against what the real reference returned
(golden g26, tools/gen_golden_traj_align.py); the ABI of the two result entry points (include/sp_hip.h: sp_traj_align, sp_map_points);
the trajectory files of ``write_tum_format``."""
import ctypes

import numpy as np
import pytest
import torch

import traj_align_ref as ref
from conftest import load_golden

CASE_IDS = [c[0] for c in ref.CASES]


@pytest.fixture(scope="module")
def golden():
    return load_golden("g26_traj_align")


@pytest.mark.parametrize("case", ref.CASES, ids=CASE_IDS)
def test_restatement_equals_the_reference(case, golden):
    """Same LAPACK calls in float64 on the same inputs: 1e-12 (3e-15 seen between two summation orders)."""
    name, kind, n, seed = case
    pred, gt = ref.make_case(kind, n, seed)
    np.testing.assert_array_equal(pred, golden[f"{name}_pred"])
    np.testing.assert_array_equal(gt, golden[f"{name}_gt"])
    a = ref.align(pred[:, :3, 3].T, gt[:, :3, 3].T)
    for key in ('rot', 'trans_scaled', 'trans_scaled_error', 'trans', 'trans_error', 's', 'model_aligned_scaled', 'model_aligned'):
        want = golden[f"{name}_align_{key}"]
        assert np.shape(a[key]) == want.shape, key
        np.testing.assert_allclose(a[key], want, rtol=0, atol=1e-12, err_msg=key)
    for anchor in (False, True):
        tag = f"{name}_anchor{int(anchor)}"
        est, pa = ref.transfer_scale(gt, pred, anchor_rotation=anchor)
        assert ('rot_reanchor' in pa) == bool(golden[f"{tag}_has_reanchor"]) == anchor
        if anchor:
            np.testing.assert_allclose(pa['rot_reanchor'], golden[f"{tag}_rot_reanchor"], rtol=0, atol=1e-12)
        if f"{tag}_poses" in golden:
            np.testing.assert_allclose(np.stack(est), golden[f"{tag}_poses"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(ref.apply_scale(pred[1], pa), golden[f"{tag}_applied"], rtol=0, atol=1e-12)
        # the record's view of the same numbers
        r = ref.align_poses(pred, gt, anchor)
        np.testing.assert_allclose(r['rot'], a['rot'], rtol=0, atol=1e-14)
        np.testing.assert_array_equal(r['rot_reanchor'], pa['rot_reanchor'] if anchor else np.eye(3))
        np.testing.assert_allclose([r['ate_scaled'], r['s']], [np.sqrt(np.mean(a['trans_scaled_error'] ** 2)), a['s']], rtol=0, atol=1e-14)


@pytest.mark.parametrize("case", ref.CASES, ids=CASE_IDS)
def test_cases_have_a_unique_answer(case):
    """A property of the INPUTS: the gap (sigma_2 - sigma_3) / sigma_1 that makes the rotation unique; what each case is there for."""
    name, kind, n, seed = case
    pred, gt = ref.make_case(kind, n, seed)
    assert pred.dtype == np.float32 and gt.dtype == np.float32 and pred.shape == (n, 4, 4)
    a = ref.align(pred[:, :3, 3].T, gt[:, :3, 3].T)
    assert ref.condition(pred, gt) >= 0.1, (name, a['sigma'])
    if kind == "planar":
        assert np.all(pred[:, 2, 3] == 0.0) and a['sigma'][2] == 0.0
    if kind == "mirrored":
        assert a['reflected'] and a['sigma'][2] > 0.01 * a['sigma'][0]
    if kind == "generic" and n > 3:
        assert not a['reflected']
    # the tolerance rule of the device test gives finite, small bounds
    base, spread = ref.permutation_spread(pred, gt, anchor_rotation=True)
    tol = ref.tolerance(spread)
    assert set(tol) == set(ref.FIELDS) and all(1e-13 <= v < 1e-9 for v in tol.values()), tol


def test_result_records_and_symbols_match_the_header():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    import abi_header
    from super_primitive_amd import _lib
    assert "sp_traj_align" in _lib.SIGNATURES and "sp_map_points" in _lib.SIGNATURES
    # the wrapper reads the record as float64 words: its own table of them is the header's field order
    fields = abi_header.parse()[2]["SpTrajAlign"]["fields"]
    from super_primitive_amd.tool import pose_utils
    assert {k: v[0] for k, v in pose_utils._FIELDS.items()} == {name: offset / 8 for name, offset, _ in fields}


def test_result_entry_points_refuse_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)                                    # (never dereferenced: the checks fail first)
    assert lib.sp_traj_align(None, p, p, 1, 3, 0, p, p, p, None) == -1
    assert lib.sp_traj_align(p, p, p, 0, 3, 0, p, p, p, None) == -1 and lib.sp_traj_align(p, p, p, 1, 2, 0, p, p, p, None) == -1
    assert lib.sp_traj_align(p, p, p, 1, 3, 0, None, p, p, None) == -1 and lib.sp_traj_align(p, p, p, 70000, 3, 0, p, p, p, None) == -1
    assert lib.sp_traj_align(p, p, p, 65535, 1 << 20, 0, p, p, p, None) == -2
    assert lib.sp_map_points(None, 1, 1, 1, None, 0, p, p, p, p, 1, None) == -1
    assert lib.sp_map_points(p, 0, 1, 1, None, 0, p, p, p, p, 1, None) == -1 and lib.sp_map_points(p, 1, 0, 1, None, 0, p, p, p, p, 1, None) == -1
    assert lib.sp_map_points(p, 1, 1, 0, None, 0, p, p, p, p, 1, None) == -1 and lib.sp_map_points(p, 1, 1, 1, None, 0, p, p, p, p, 0, None) == -1
    assert lib.sp_map_points(p, 1, 1, 1, None, 0, p, p, p, p, 257, None) == -1                 # more rows than the workgroups hold
    assert lib.sp_map_points(p, 1, 1, 1, None, 1, p, p, p, p, 1, None) == -1 and lib.sp_map_points(p, 1, 1, 1, p, 0, p, p, p, p, 1, None) == -1
    assert lib.sp_map_points(p, 1, 1, 1, None, 0, p, None, p, p, 1, None) == -1


def test_python_surface_refuses_host_tensors_and_short_trajectories():
    from super_primitive_amd.tool import pose_utils
    from super_primitive_amd.odometery import results
    T = torch.eye(4).repeat(1, 5, 1, 1)
    with pytest.raises(RuntimeError, match="HIP-only"):
        pose_utils.align_trajectories(T, T)
    with pytest.raises(RuntimeError, match="HIP-only"):
        pose_utils.align(torch.zeros(3, 5), torch.zeros(3, 5))
    with pytest.raises(RuntimeError, match="HIP-only"):
        pose_utils.apply_scale(torch.eye(4), {})
    assert pose_utils.get_sorted_by_timestamp({"10": "b", 9: "a", 11: "c"}, return_ids=True) == (["a", "b", "c"], [9, "10", 11])
    assert pose_utils.get_sorted_by_timestamp({2: "b", 1: "a"}) == ["a", "b"]
    with pytest.raises(ValueError):
        results.keyframe_points([], [], [])
    with pytest.raises(ValueError, match="keep_keyframes"):
        results.sequence_map(dict(kf_archive={0: dict(pose=None, kld=None, aff=None, kf=None)}, kf_trajectory={}), 4)


def test_write_tum_format_round_trip(tmp_path):
    from scipy.spatial.transform import Rotation
    from super_primitive_amd.lie.lie_algebra import tq_to_pose
    from super_primitive_amd.odometery.results import write_tum_format
    rng = np.random.default_rng(5)
    n = 7
    def poses():
        T = np.tile(np.eye(4), (n, 1, 1))
        T[:, :3, :3] = Rotation.from_rotvec(rng.uniform(-1.5, 1.5, (n, 3))).as_matrix()
        T[:, :3, 3] = rng.uniform(-2, 2, (n, 3))
        return T
    pred, gt = poses(), poses()
    stamps = [1305031452.791720 + 0.03 * i for i in range(n)]
    files = write_tum_format(stamps, torch.from_numpy(pred), list(gt), tmp_path / "out")
    assert [f.name for f in files] == ["converted_tum_traj.txt", "converted_gt_tum_traj.txt"]
    for file, want in zip(files, (pred, gt)):
        lines = open(file).read().splitlines()
        assert len(lines) == n
        rows = np.array([[float(v) for v in line.split(" ")] for line in lines])
        assert rows.shape == (n, 8)
        np.testing.assert_array_equal(rows[:, 0], stamps)
        np.testing.assert_allclose(rows[:, 1:4], want[:, :3, 3], rtol=0, atol=1e-15)
        q = rows[:, 4:]
        np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-12)
        # xyzw: the scalar part is LAST -- cos(angle / 2) of the rotation
        angle = np.linalg.norm(Rotation.from_matrix(want[:, :3, :3]).as_rotvec(), axis=1)
        np.testing.assert_allclose(np.abs(q[:, 3]), np.abs(np.cos(angle / 2)), atol=1e-12)
        np.testing.assert_allclose(tq_to_pose(rows[:, 1:]), want, atol=1e-12)
    with pytest.raises(ValueError):
        write_tum_format(stamps[:-1], pred, gt, tmp_path / "out")
