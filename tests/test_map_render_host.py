"""CPU-only: the ABI of the map-view entry points (include/sp_hip.h: sp_render_views, sp_depth_lift), their argument checks -- made before
any device work, so they answer without a GPU -- and the argument checks of the Python surface (``tool/viz.py``, ``odometery/results.py``
``render_map`` / ``score_map``)."""
import ctypes

import pytest
import torch


def test_symbols_and_view_record_match_the_header():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    for name in ("sp_render_views", "sp_depth_lift", "sp_depth_lift_blocks"):
        assert name in _lib.SIGNATURES, name


def test_render_views_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)                                    # (never dereferenced: the checks fail first)
    ok = dict(points=p, colours=p, Q=10, views=p, V=1, H=4, W=4, mode=0, z_min=1e-6, keys=p, image=p, depth=p, index=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_render_views(a['points'], a['colours'], a['Q'], a['views'], a['V'], a['H'], a['W'], a['mode'], a['z_min'], a['keys'],
                                   a['image'], a['depth'], a['index'], None)
    for bad in (dict(points=None), dict(views=None), dict(keys=None), dict(colours=None), dict(Q=0), dict(Q=-1), dict(V=0), dict(H=0), dict(W=-3),
                dict(mode=2), dict(mode=-1), dict(z_min=-1.0), dict(z_min=float("nan"))):
        assert call(**bad) == -1, bad
    for big in (dict(Q=2 ** 31 - 1), dict(Q=2 ** 40), dict(V=65536), dict(H=1 << 16, W=1 << 15), dict(V=2, H=1 << 15, W=1 << 15),
                dict(V=65535, H=1 << 10, W=1 << 10)):
        assert call(**big) == -2, big
    # invalid beats too large: nothing is launched either way
    assert call(Q=2 ** 40, points=None) == -1


def test_depth_lift_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)
    ok = dict(depth=p, K=p, pose=None, image=None, B=1, H=4, W=4, trunc=100.0, bc=p, points=p, colours=None, pixel=p, counts=p, offsets=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_depth_lift(a['depth'], a['K'], a['pose'], a['image'], a['B'], a['H'], a['W'], a['trunc'], a['bc'], a['points'], a['colours'],
                                 a['pixel'], a['counts'], a['offsets'], None)
    for bad in (dict(depth=None), dict(K=None), dict(bc=None), dict(points=None), dict(pixel=None), dict(counts=None), dict(offsets=None),
                dict(image=p), dict(colours=p), dict(B=0), dict(H=0), dict(W=-1), dict(trunc=0.0), dict(trunc=float("nan"))):
        assert call(**bad) == -1, bad
    for big in (dict(B=65536), dict(H=1 << 16, W=1 << 15), dict(B=2, H=1 << 15, W=1 << 15)):
        assert call(**big) == -2, big
    assert lib.sp_depth_lift_blocks(3, 19, 23) == 3 * 2 and lib.sp_depth_lift_blocks(1, 64, 80) == 20
    assert lib.sp_depth_lift_blocks(0, 4, 4) == -1 and lib.sp_depth_lift_blocks(65536, 4, 4) == -2


def test_python_surface_raises_value_error_before_any_launch():
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    pts, cols, K, eye = torch.zeros(5, 3), torch.zeros(5, 3), torch.eye(3), torch.eye(4)
    with pytest.raises(ValueError, match="HIP-only"):                          # CPU tensors
        viz.render_pcd(pts, cols, K, 4, 4)
    with pytest.raises(ValueError, match="HIP-only"):
        viz.depth_image_lift(torch.ones(4, 4), K)
    with pytest.raises(ValueError, match="HIP-only"):
        viz.lift_depth_images(torch.ones(1, 4, 4), K)
    with pytest.raises(ValueError, match="HIP-only"):
        results.render_map(dict(points=pts, colours=cols), K, eye[None], (4, 4))
    with pytest.raises(ValueError, match="cuda tensors"):
        viz.render_pcd(pts.numpy(), cols, K, 4, 4)
    with pytest.raises(ValueError, match=r"\(V,4,4\)"):
        results.render_map(dict(points=pts, colours=cols), K, eye, (4, 4))
    with pytest.raises(ValueError, match=r"\(V,H,W\)"):
        results.score_map(dict(points=pts), torch.ones(4, 4), K, eye[None])
    with pytest.raises(ValueError, match="size"):
        results.score_map(dict(points=pts), torch.ones(1, 4, 4), K, eye[None], size=(4, 5))


def _meta(*shape, dtype=torch.float32):
    """A tensor without storage: the shape and dtype checks run where there is no GPU, and every case must raise before a pointer is taken."""
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_python_surface_checks_shapes_and_dtypes(monkeypatch):
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)              # shapes and dtypes only: nothing below reaches a launch
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error reached the library"))
    pts, cols, K, eye = _meta(5, 3), _meta(5, 3), _meta(3, 3), _meta(1, 4, 4)
    bad_render = [dict(points=_meta(0, 3), colours=_meta(0, 3)),               # Q = 0
                  dict(points=_meta(5, 4)), dict(points=_meta(15)), dict(colours=_meta(4, 3)), dict(colours=_meta(5, 3, 1)),
                  dict(points=_meta(5, 3, dtype=torch.float64)), dict(colours=_meta(5, 3, dtype=torch.float16)),
                  dict(Ks=_meta(2, 3, 3)), dict(Ks=_meta(9)), dict(Ks=_meta(3, 3, dtype=torch.int32)),
                  dict(poses=_meta(4, 4)), dict(poses=_meta(1, 3, 4)), dict(poses=_meta(0, 4, 4)), dict(H=0), dict(W=-2), dict(z_min=-1.0),
                  dict(colours=None)]
    for kw in bad_render:
        a = dict(dict(points=pts, colours=cols, Ks=K, poses=eye, H=4, W=6), **kw)
        with pytest.raises(ValueError):
            viz.render_views(**a)
    with pytest.raises(ValueError):
        viz.render_pcd(pts, cols, _meta(1, 3, 3), 4, 6)
    with pytest.raises(ValueError, match="limits"):
        viz.render_views(pts, cols, K, _meta(2, 4, 4), 1 << 15, 1 << 15)
    d = _meta(2, 4, 6)
    for kw in (dict(depths=_meta(4, 6)), dict(depths=_meta(2, 4, 6, dtype=torch.float64)), dict(depths=_meta(0, 4, 6)), dict(Ks=_meta(3, 3, 3)),
               dict(poses=_meta(3, 4, 4)), dict(images=_meta(2, 4, 6, 3)), dict(images=_meta(2, 3, 4, 5)), dict(depth_trunc=0.0)):
        a = dict(dict(depths=d, Ks=K, poses=None, images=None), **kw)
        with pytest.raises(ValueError):
            viz.lift_depth_images(**a)
    for kw in (dict(depth=d), dict(image=_meta(4, 6)), dict(T=_meta(1, 4, 4)), dict(mask=_meta(24))):
        a = dict(dict(depth=_meta(4, 6), K=K), **kw)
        with pytest.raises(ValueError):
            viz.depth_image_lift(**a)
    world = dict(points=pts, colours=cols)
    with pytest.raises(ValueError):
        results.render_map(world, K, _meta(4, 4), (4, 6))
    with pytest.raises(ValueError, match="size"):
        results.score_map(world, _meta(1, 4, 6), K, eye, size=(6, 4))
    with pytest.raises(ValueError):
        results.score_map(world, _meta(2, 4, 6), K, eye)                       # two depth images, one pose
    with pytest.raises(ValueError):
        results.score_map(world, _meta(1, 4, 6, dtype=torch.float64), K, eye)
