"""CPU-only: the ABI of the footprint render and the image score (include/sp_hip.h: sp_render_splats, sp_image_metrics), their argument
checks -- made before any device work, so they answer without a GPU -- and the argument checks of the Python surface (``tool/viz.py``
``render_views(radii=...)`` / ``image_metrics``, ``odometery/results.py`` ``render_map`` / ``score_map`` / ``score_map_images``)."""
import ctypes
import inspect
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_match_the_header_and_the_abi_version_stays():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp_hip.h")).read()
    for name in ("sp_render_splats", "sp_image_metrics"):
        assert name in _lib.SIGNATURES, name
    assert "NOT when its centre lies inside" in header                      # the cell rule is part of the contract


def test_render_splats_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)                                    # (never dereferenced: the checks fail first)
    ok = dict(points=p, colours=p, Q=10, views=p, V=1, H=4, W=4, z_min=1e-6, radii=p, max_px=3, keys=p, image=p, depth=p, index=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_render_splats(a['points'], a['colours'], a['Q'], a['views'], a['V'], a['H'], a['W'], a['z_min'], a['radii'], a['max_px'],
                                    a['keys'], a['image'], a['depth'], a['index'], None)
    for bad in (dict(points=None), dict(views=None), dict(keys=None), dict(radii=None), dict(colours=None), dict(Q=0), dict(Q=-1), dict(V=0),
                dict(H=0), dict(W=-3), dict(z_min=-1.0), dict(z_min=float("nan")), dict(max_px=-1), dict(max_px=17), dict(max_px=1 << 20)):
        assert call(**bad) == -1, bad
    for big in (dict(Q=2 ** 31 - 1), dict(Q=2 ** 40), dict(V=65536), dict(H=1 << 16, W=1 << 15), dict(V=2, H=1 << 15, W=1 << 15),
                dict(V=65535, H=1 << 10, W=1 << 10)):
        assert call(**big) == -2, big
    assert call(Q=2 ** 40, radii=None) == -1                        # invalid beats too large: nothing is launched either way


def test_image_metrics_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)
    ok = dict(rendered=p, target=p, index=p, V=1, H=4, W=4, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_image_metrics(a['rendered'], a['target'], a['index'], a['V'], a['H'], a['W'], a['out'], None)
    for bad in (dict(rendered=None), dict(target=None), dict(index=None), dict(out=None), dict(V=0), dict(H=0), dict(W=-1)):
        assert call(**bad) == -1, bad
    for big in (dict(V=65536), dict(H=1 << 16, W=1 << 15), dict(V=2, H=1 << 15, W=1 << 15)):
        assert call(**big) == -2, big
    assert call(V=65536, out=None) == -1


def test_the_new_keywords_default_to_the_existing_call():
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    for fn in (viz.render_views, results.render_map, results.score_map, results.score_map_images):
        sig = inspect.signature(fn).parameters
        assert sig['radii'].default is None and sig['max_px'].default == 8, fn.__name__
    assert inspect.signature(results.point_radii).parameters['footprint'].default == 1.0


def _meta(*shape, dtype=torch.float32):
    """A tensor without storage: every case must raise before a pointer is taken."""
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_python_surface_raises_value_error_before_any_launch(monkeypatch):
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    with pytest.raises(ValueError, match="HIP-only"):                          # CPU tensors
        viz.render_views(torch.zeros(5, 3), torch.zeros(5, 3), torch.eye(3), torch.eye(4)[None], 4, 4, depth_buffer=True, radii=torch.zeros(5))
    with pytest.raises(ValueError, match="HIP-only"):
        viz.image_metrics(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int32))
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)              # shapes and dtypes only: nothing below reaches a launch
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error reached the library"))
    pts, cols, K, eye, rad = _meta(5, 3), _meta(5, 3), _meta(3, 3), _meta(1, 4, 4), _meta(5)
    ok = dict(points=pts, colours=cols, Ks=K, poses=eye, H=4, W=6, depth_buffer=True, radii=rad, max_px=3)
    with pytest.raises(ValueError, match="depth_buffer"):
        viz.render_views(**dict(ok, depth_buffer=False))
    with pytest.raises(ValueError, match="depth_buffer"):
        viz.render_views(pts, cols, K, eye, 4, 6, radii=rad)                   # the default is the reference's mode: refused with radii
    for kw in (dict(radii=_meta(4)), dict(radii=_meta(5, 1)), dict(radii=_meta(5, dtype=torch.float64)), dict(radii=_meta(5, dtype=torch.int32)),
               dict(max_px=-1), dict(max_px=17), dict(max_px=2.5), dict(radii=[0.1] * 5)):
        with pytest.raises(ValueError):
            viz.render_views(**dict(ok, **kw))
    world = dict(points=pts, colours=cols)
    with pytest.raises(ValueError, match="depth_buffer"):
        results.render_map(world, K, eye, (4, 6), depth_buffer=False, radii=rad)
    with pytest.raises(ValueError):
        results.render_map(world, K, eye, (4, 6), radii=_meta(6))
    with pytest.raises(ValueError):
        results.score_map(world, _meta(1, 4, 6), K, eye, radii=rad, max_px=99)
    with pytest.raises(ValueError):
        results.score_map(world, _meta(1, 4, 6), K, eye, radii=_meta(5, dtype=torch.float16))
    for images in (_meta(1, 4, 6, 3), _meta(3, 4, 6), _meta(2, 3, 4, 6), _meta(1, 3, 4, 6, dtype=torch.float64)):
        with pytest.raises(ValueError, match="images"):
            results.score_map_images(world, images, K, eye)
    with pytest.raises(ValueError):
        results.score_map_images(world, _meta(1, 3, 4, 6), K, eye, radii=_meta(4))
    with pytest.raises(ValueError):
        results.score_map_images(world, _meta(1, 3, 4, 6), K, _meta(4, 4))
    good = dict(rendered=_meta(2, 4, 6, 3, dtype=torch.uint8), target=_meta(2, 3, 4, 6), index=_meta(2, 4, 6, dtype=torch.int32))
    for kw in (dict(rendered=_meta(2, 4, 6, 3)), dict(rendered=_meta(2, 4, 6, dtype=torch.uint8)), dict(rendered=_meta(2, 3, 4, 6, dtype=torch.uint8)),
               dict(rendered=_meta(0, 4, 6, 3, dtype=torch.uint8), target=_meta(0, 3, 4, 6), index=_meta(0, 4, 6, dtype=torch.int32)),
               dict(target=_meta(2, 4, 6, 3)), dict(target=_meta(2, 3, 4, 6, dtype=torch.float64)), dict(index=_meta(2, 4, 6, dtype=torch.int64)),
               dict(index=_meta(2, 6, 4, dtype=torch.int32))):
        with pytest.raises(ValueError):
            viz.image_metrics(**dict(good, **kw))
    with pytest.raises(ValueError, match="limits"):
        viz.image_metrics(_meta(2, 1 << 15, 1 << 15, 3, dtype=torch.uint8), _meta(2, 3, 1 << 15, 1 << 15), _meta(2, 1 << 15, 1 << 15, dtype=torch.int32))
