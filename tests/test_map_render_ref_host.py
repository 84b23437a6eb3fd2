"""CPU-only: the float64 statements of tests/map_render_ref.py against what the REAL reference's ``tool/viz.py`` ``render_pcd`` returned
(golden g_render_pcd, tools/gen_golden_render_pcd.py), the inputs of every device case of tests/test_gpu_map_render.py against the
conditions the comparison there relies on (how many pixels the two ambiguity masks exclude; how far another float64 summation order
moves a position), and the lift statement against a literal per-pixel loop."""
import numpy as np
import pytest

import map_render_ref as ref
from conftest import load_golden
from map_splat_ref import case_splat_views17

TAINT_CAP = 0.02          # the project's cap on excluded pixels (tests/test_gpu_segment_depth.py)


@pytest.mark.parametrize("name", list(ref.GOLDEN_CASES))
def test_mode0_statement_reproduces_the_reference_image(name):
    g = load_golden("g_render_pcd")
    case = ref.GOLDEN_CASES[name]()
    assert ref.digest(case) == str(g[name + "_sha256"]), "the seeded inputs are not the ones the golden was made from"
    if name + "_points" in g:
        np.testing.assert_array_equal(case['points'], g[name + "_points"])
        np.testing.assert_array_equal(case['colours'], g[name + "_colours"])
        np.testing.assert_array_equal(case['K'], g[name + "_K"])
    image, depth, index = ref.render(case['points'], case['colours'], case['K'], None, case['H'], case['W'], 0)
    np.testing.assert_array_equal(image, g[name + "_image"])
    hit = index >= 0
    if name == "golden0":
        z = case['points'][index[hit], 2]
        assert (z < 0).sum() >= 2 and (np.abs(case['points'][:, 2]) < 1e-3).any()       # behind the camera, and near z = 0
        assert len(case['points']) % 256 != 0 and len(case['points']) > 256
    else:
        assert index.max() > 65535 and len(case['points']) / index.size > 80
    # the highest index of every pixel, said once more without the loop
    u, v, _ = ref.project(case['points'], case['K'])
    keep = (u >= 0) & (u < case['W']) & (v >= 0) & (v < case['H'])
    top = np.full(index.shape, -1, np.int64)
    np.maximum.at(top, (v[keep].astype(np.int64), u[keep].astype(np.int64)), np.nonzero(keep)[0])
    np.testing.assert_array_equal(top, index)


def _views():
    """(name, case, view, pose) of every view of every device case."""
    dup, _ = ref.case_duplicates()
    cases = dict(golden0=ref.case_golden0(), collide=ref.case_collide(), duplicates=dup, posed=ref.case_posed(), edges=ref.case_edges(),
                 views17=case_splat_views17())                                # (its points and views as points: the radii are not read)
    for name, case in cases.items():
        poses = case.get('poses')
        for k in range(1 if poses is None else len(poses)):
            yield name, case, k, None if poses is None else poses[k]


@pytest.mark.parametrize("name,case,k,pose", list(_views()), ids=[f"{n}-{k}" for n, _, k, _ in _views()])
def test_ambiguity_masks_exclude_few_pixels(name, case, k, pose):
    """A condition on the INPUTS: continuous random coordinates put almost no point within 1e-6 px of a pixel edge."""
    H, W = case['H'], case['W']
    taint = ref.position_taint(case['points'], case['K'], pose, H, W) | ref.depth_tie_taint(case['points'], case['K'], pose, H, W)
    share = taint.mean()
    print(f"\n{name} view {k}: {int(taint.sum())} of {taint.size} pixels excluded ({100 * share:.3f} %)")
    assert share <= TAINT_CAP
    if name == "duplicates":
        _, (r, c) = ref.case_duplicates()
        assert not taint[r, c]                                               # one float32(z), two float64 z: the index decides


def test_duplicates_case_holds_what_it_is_there_for():
    case, (r, c) = ref.case_duplicates()
    pose = case['poses'][0]
    _, _, z = ref.project(case['points'], case['K'], pose)
    assert z[550] != z[551] and np.float32(z[550]) == np.float32(z[551]) == np.float32(9.0)
    _, depth, index = ref.render(case['points'], case['colours'], case['K'], pose, case['H'], case['W'], 1)
    assert index[r, c] == 551 and depth[r, c] == np.float32(9.0)
    assert (index >= 500).sum() >= 10 and ((index >= 0) & (index < 50)).sum() == 0          # a duplicate wins over its original
    win = index[(index >= 500) & (index < 550)]
    assert not np.array_equal(case['colours'][win], case['colours'][win - 500])


def test_posed_case_holds_what_it_is_there_for():
    case = ref.case_posed()
    H, W = case['H'], case['W']
    out = {(k, m): ref.render(case['points'], case['colours'], case['K'], case['poses'][k], H, W, m) for k in range(3) for m in (0, 1)}
    _, _, z1 = ref.project(case['points'], case['K'], case['poses'][1])
    assert 0.4 < (z1 < 0).mean() < 0.6                                      # half the cloud is behind the second view
    idx0, idx1 = out[1, 0][2], out[1, 1][2]
    assert (z1[idx0[idx0 >= 0]] < 0).sum() >= 20 and (z1[idx1[idx1 >= 0]] < 0).sum() == 0
    assert (out[0, 1][2] >= 0).mean() > 0.3                                 # the first view looks at the cloud
    for m in (0, 1):
        image, depth, index = out[2, m]
        assert not image.any() and not depth.any() and (index == -1).all()


@pytest.mark.parametrize("name,case,k,pose", [v for v in _views() if v[3] is not None], ids=[f"{n}-{k}" for n, _, k, p in _views() if p is not None])
def test_summation_order_moves_no_position_by_a_sixteenth_of_delta(name, case, k, pose):
    H, W = case['H'], case['W']
    u0, v0, _ = ref.project(case['points'], case['K'], pose, order=0)
    worst = 0.0
    for order in (1, 2):
        u, v, _ = ref.project(case['points'], case['K'], pose, order=order)
        with np.errstate(invalid='ignore'):
            near = (np.minimum(u0, u) > -1) & (np.maximum(u0, u) < W + 1) & (np.minimum(v0, v) > -1) & (np.maximum(v0, v) < H + 1)
        if near.any():
            worst = max(worst, float(np.abs(u - u0)[near].max()), float(np.abs(v - v0)[near].max()))
    print(f"\n{name} view {k}: another summation order moves a position by at most {worst:.2e} px (DELTA / 16 = {ref.DELTA / 16:.2e})")
    assert worst <= ref.DELTA / 16


@pytest.mark.parametrize("make", [ref.lift_case_small, ref.lift_case_single, ref.lift_case_blocks, ref.lift_case_blocks_odd],
                         ids=["3x19x23", "1x64x80", "3x150x150", "3x149x149"])
def test_lift_statement_against_a_literal_loop(make):
    depth, K, poses, image = make()
    B, H, W = depth.shape
    got = ref.lift(depth, K, poses, image)
    rows, cols, pix, counts = [], [], [], []
    for b in range(B):
        fx, fy, cx, cy = (float(K[b][0, 0]), float(K[b][1, 1]), float(K[b][0, 2]), float(K[b][1, 2]))
        T = poses[b].astype(np.float64)
        n = 0
        for r in range(H):
            for c in range(W):
                d = float(depth[b, r, c])
                if not (d > 0 and d <= 100.0):
                    continue
                x, y = (c - cx) * d / fx, (r - cy) * d / fy
                rows.append([((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * d) + T[k, 3] for k in range(3)])
                cols.append(image[b, :, r, c])
                pix.append(r * W + c)
                n += 1
        counts.append(n)
    np.testing.assert_array_equal(got['counts'], counts)
    np.testing.assert_array_equal(got['offsets'], np.concatenate(([0], np.cumsum(counts))))
    np.testing.assert_array_equal(got['pixel'], pix)
    np.testing.assert_array_equal(got['points'], np.array(rows).reshape(-1, 3))
    np.testing.assert_array_equal(got['colours'], np.array(cols).reshape(-1, 3))
    if H * W > 65536 // 3:                                                   # more blocks than the scan has threads: two per thread
        nblk = -(-H * W // 256)
        assert 256 < B * nblk <= 512 and min(counts) > 0
        assert (nblk % 2 == 1) == (make is ref.lift_case_blocks_odd)         # image 1 starts at an odd block: inside a scan thread's pair
    elif B == 3:
        assert counts[1] == 0 and counts[2] == H * W and 0 < counts[0] < H * W and pix[0] == 0       # 100.0 itself is valid
        for bad in (0.0, -1.5, 100.5):
            assert (depth[0] == bad).any()
        assert np.isnan(depth[0]).any() and np.isinf(depth[0]).any()
