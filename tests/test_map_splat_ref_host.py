"""CPU-only: the float64 statements of tests/map_splat_ref.py against the point render's statement (radius 0), the inputs of every
device case of tests/test_gpu_map_splat.py against the conditions the comparison there relies on (how many pixels the two ambiguity
masks exclude in every posed view; how far another float64 summation order moves an edge of a footprint), and what every constructed
case is there for."""
import functools

import numpy as np
import pytest

import map_render_ref as base
import map_splat_ref as ref

TAINT_CAP = 0.02          # the project's cap on excluded pixels (tests/test_gpu_segment_depth.py)


@functools.lru_cache(maxsize=None)
def _case(name):
    return ref.CASES[name]()


def _posed_views():
    for name in ref.CASES:
        case = _case(name)
        for k, pose in enumerate(case.get('poses', [None])):
            if not ref.is_identity(pose):
                yield name, k


POSED = list(_posed_views())


@functools.lru_cache(maxsize=None)
def _rendered(name, k):
    c = _case(name)
    pose = None if 'poses' not in c else c['poses'][k]
    return ref.render(c['points'], c['colours'], c['radii'], c['K'], pose, c['H'], c['W'], c['max_px'])


@pytest.mark.parametrize("make", [base.case_posed, lambda: base.case_duplicates()[0]], ids=["posed", "duplicates"])
def test_radius_zero_is_the_point_render_in_mode_1(make):
    c = make()
    zero = np.zeros(len(c['points']), np.float32)
    for pose in c['poses']:
        want = base.render(c['points'], c['colours'], c['K'], pose, c['H'], c['W'], 1)
        got = ref.render(c['points'], c['colours'], zero, c['K'], pose, c['H'], c['W'], max_px=3)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("name,k", POSED, ids=[f"{n}-{k}" for n, k in POSED])
def test_ambiguity_masks_exclude_few_pixels(name, k):
    """A condition on the INPUTS, asserted on every posed view of every case."""
    c = _case(name)
    args = (c['points'], c['radii'], c['K'], c['poses'][k], c['H'], c['W'], c['max_px'])
    taint = ref.position_taint(*args) | ref.depth_tie_taint(*args)
    print(f"\n{name} view {k}: {int(taint.sum())} of {taint.size} pixels excluded ({100 * taint.mean():.3f} %)")
    assert taint.mean() <= TAINT_CAP


@pytest.mark.parametrize("name,k", POSED, ids=[f"{n}-{k}" for n, k in POSED])
def test_summation_order_moves_no_edge_by_a_sixteenth_of_delta(name, k):
    c = _case(name)
    H, W = c['H'], c['W']
    u0, v0, z0, ru0, rv0 = ref.footprints(c['points'], c['radii'], c['K'], c['poses'][k], c['max_px'], order=0)
    worst = 0.0
    for order in (1, 2):
        u, v, z, ru, rv = ref.footprints(c['points'], c['radii'], c['K'], c['poses'][k], c['max_px'], order=order)
        with np.errstate(invalid='ignore'):
            near = ((np.minimum(z0, z) > 0) & (np.minimum(u0 + ru0, u + ru) > -1) & (np.maximum(u0 - ru0, u - ru) < W + 1)
                    & (np.minimum(v0 + rv0, v + rv) > -1) & (np.maximum(v0 - rv0, v - rv) < H + 1))
        for e0, e in ((u0 - ru0, u - ru), (u0 + ru0, u + ru), (v0 - rv0, v - rv), (v0 + rv0, v + rv)):
            if near.any():
                worst = max(worst, float(np.abs(e - e0)[near].max()))
    print(f"\n{name} view {k}: another summation order moves an edge by at most {worst:.2e} px (DELTA / 16 = {ref.DELTA / 16:.2e})")
    assert worst <= ref.DELTA / 16


def _coverage(index):
    return float((index >= 0).mean())


def test_splat_posed_holds_what_it_is_there_for():
    c = _case("splat_posed")
    assert len(c['points']) == 3001 and (c['radii'][::7] == 0).all() and (c['radii'] > 0).sum() > 2500
    cover, point_cover = [], []
    for k in range(3):
        cover.append(_coverage(_rendered("splat_posed", k)[2]))
        point_cover.append(_coverage(base.render(c['points'], c['colours'], c['K'], c['poses'][k], c['H'], c['W'], 1)[2]))
    capped = ref.triples(c['points'], c['radii'], c['K'], c['poses'][1], c['H'], c['W'], c['max_px'])[1]
    print(f"\nsplat_posed: coverage {np.round(cover, 3).tolist()} (point render {np.round(point_cover, 3).tolist()}); {capped} splats at the cap in view 1")
    assert cover[0] > point_cover[0] and cover[1] > point_cover[1]
    assert capped >= 20
    image, depth, index = _rendered("splat_posed", 2)
    assert not image.any() and not depth.any() and (index == -1).all() and point_cover[2] == 0


def test_splat_collide_holds_what_it_is_there_for():
    c = _case("splat_collide")
    assert len(c['points']) == 70001 and ref.is_identity(c['poses'][0]) and not ref.is_identity(c['poses'][1])
    cover = [_coverage(_rendered("splat_collide", k)[2]) for k in range(2)]
    top = int(_rendered("splat_collide", 0)[2].max())
    print(f"\nsplat_collide: coverage {np.round(cover, 3).tolist()}, highest winning index from the identity pose {top}")
    assert top > 65535 and min(cover) > 0.5
    # a footprint lets a near point take its neighbours' pixels: fewer distinct winners than pixels covered
    idx = _rendered("splat_collide", 0)[2]
    assert len(np.unique(idx[idx >= 0])) < (idx >= 0).sum()


def test_splat_views17_holds_what_it_is_there_for():
    c = _case("splat_views17")
    assert len(c['poses']) == 17 and len(c['points']) == 300 and not any(ref.is_identity(p) for p in c['poses'])
    cover = [_coverage(_rendered("splat_views17", k)[2]) for k in range(17)]
    print(f"\nsplat_views17: coverage {min(cover):.3f} .. {max(cover):.3f}")
    assert min(cover) > 0.2
    assert not np.array_equal(_rendered("splat_views17", 16)[2], _rendered("splat_views17", 0)[2])


def test_splat_edges_each_point_does_what_it_is_there_for():
    c = _case("splat_edges")
    R = ref.EDGE_ROWS
    image, depth, index = ref.render(c['points'], c['colours'], c['radii'], c['K'], None, c['H'], c['W'], c['max_px'])

    def pixels(name):
        return sorted(map(tuple, np.argwhere(index == R[name]).tolist()))

    def block(r0, r1, c0, c1):
        return [(r, col) for r in range(r0, r1 + 1) for col in range(c0, c1 + 1)]
    assert pixels("reaches") == block(7, 9, 0, 0)
    assert pixels("misses") == [] and pixels("below_z_min") == [] and pixels("nan_point") == []
    assert pixels("nan_radius") == [(12, 3)] and pixels("negative_radius") == [(12, 6)] and pixels("zero_radius") == [(12, 9)]
    assert pixels("inf_radius") == block(1, 7, 1, 7)
    assert pixels("z_inf") == [(7, 8)] and np.isinf(depth[7, 8])
    assert pixels("corner") == block(15, 19, 19, 23)
    assert pixels("near") == block(1, 7, 11, 17) and depth[4, 14] == np.float32(0.01)
    assert len(c['points']) == 11 == len(R)
    n, capped = ref.triples(c['points'], c['radii'], c['K'], None, c['H'], c['W'], c['max_px'])
    assert n == (index >= 0).sum() and capped == 3                            # no two of these footprints overlap


@pytest.mark.parametrize("footprint", [2.0, 3.0])
def test_plane_is_covered_within_its_bound(footprint):
    c = ref.case_plane(footprint)
    H, W = c['H'], c['W']
    _, point_depth, point_index = base.render(c['points'], c['colours'], c['K_mid'], None, H, W, 1)
    assert _coverage(point_index) == 0.25
    _, depth, index = ref.render(c['points'], c['colours'], c['radii'], c['K_mid'], None, H, W, c['max_px'])
    err = np.abs(depth.astype(np.float64) - c['gt'].astype(np.float64))
    print(f"\nplane, footprint {footprint}: coverage {_coverage(index)}, worst error {err.max():.7f} (bound {c['bound']:.6f})")
    assert _coverage(index) == 1.0 and err.max() <= c['bound']
    if footprint == 2.0:                                                        # (at 3 a nearer neighbour reaches over a sample's own pixel)
        hit = point_index >= 0
        np.testing.assert_array_equal(index[hit], point_index[hit])


def test_image_metrics_statement_against_a_literal_loop():
    rendered, target, index = ref.metrics_inputs(2, 5, 7, 203)
    index[1] = -1
    got = ref.image_metrics(rendered, target, index)
    want = np.zeros((2, 3), np.int64)
    for k in range(2):
        for r in range(5):
            for c in range(7):
                if index[k, r, c] < 0:
                    continue
                want[k, 0] += 1
                for ch in range(3):
                    t = float(target[k, ch, r, c]) * 255.0
                    b = 0 if not t > 0 else (255 if t >= 255 else int(t))
                    d = abs(int(rendered[k, r, c, ch]) - b)
                    want[k, 1] += d
                    want[k, 2] += d * d
    np.testing.assert_array_equal(got, want)
    assert want[0, 0] > 0 and not want[1].any() and np.isnan(target).any()
