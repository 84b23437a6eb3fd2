"""Frame ingest without a GPU: the float64 restatement (tests/frame_ingest_ref.py) against torch's own float64 ops and against an
analytic pinhole image rendered through the distortion (the direction of the map), its exact cases, and the host side of the two
entry points (header / ctypes table / library, every refusal, host tensors refused)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frame_ingest_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sp_frame_ingest", "sp_depth_ingest")


def test_remap_is_grid_sample_with_a_zero_border():
    """Every case's map, float64 grid_sample(bilinear, zeros, align_corners=True) on the same coordinates: 1e-12 (a few roundings of
    2^-53 on values up to 255; the normalised grid costs grid_sample about 1e-14)."""
    worst = 0.0
    for name, c in list(ref.CASES.items()) + [("tum", ref.tum_case())]:
        H, W = c["size"]
        raw = ref.noise_frames(1, H, W, 11)[0]
        mx, my = ref.undistort_map(H, W, c["K"], c["dist"])
        got = ref.remap(raw, mx, my)
        grid = torch.from_numpy(np.stack([2 * mx / (W - 1) - 1, 2 * my / (H - 1) - 1], -1))[None]
        want = F.grid_sample(torch.from_numpy(raw.astype(np.float64)).permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="zeros",
                             align_corners=True)[0].permute(1, 2, 0).numpy()
        err = np.abs(got - want).max()
        worst = max(worst, err)
        assert err <= 1e-12 * 255, (name, err)
    print("remap vs grid_sample, worst", worst)


def test_the_rational_case_leaves_the_frame_and_the_tum_crop_does_not():
    c = ref.CASES["7x9_rational_p0"]
    H, W = c["size"]
    leaving = ref.taps_leaving(*ref.undistort_map(H, W, c["K"], c["dist"]), H, W)
    assert 0.25 < leaving.mean() < 0.9, leaving.mean()
    c = ref.tum_case()
    H, W = c["size"]
    mh, mw = c["margins"]
    leaving = ref.taps_leaving(*ref.undistort_map(H, W, c["K"], c["dist"]), H, W)
    assert leaving.any() and not leaving[mh:H - mh, mw:W - mw].any()


@pytest.mark.parametrize("shape,out", [((448, 576), (224, 288)), ((447, 575), (223, 287)), ((84, 120), (21, 30)), ((13, 17), (6, 8)),
                                       ((9, 11), (9, 11))], ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_is_interpolate_bilinear(shape, out):
    image = np.random.default_rng(3).random(shape + (3,))
    got = ref.resize_bilinear(image, *out)
    want = F.interpolate(torch.from_numpy(image).permute(2, 0, 1)[None], size=out, mode="bilinear", align_corners=False)[0]
    assert np.abs(got - want.permute(1, 2, 0).numpy()).max() <= 1e-12
    if shape == out:
        assert np.array_equal(got, image)                                           # the identity, exactly
    elif shape[0] == 2 * out[0]:
        assert np.abs(got - ref.two_by_two_mean(image)).max() <= 1e-15             # even sizes: the mean of the central pixels
    elif out[0] == shape[0] // 2:
        assert np.abs(got - ref.two_by_two_mean(image)).max() > 0.1                # odd sizes: NOT that mean (the shortcut's guard)


def test_the_map_undoes_the_distortion():
    """A pinhole image P rendered through the distortion (every raw pixel inverted by 50 fixed-point iterations), quantised to uint8
    and undistorted by the restatement, is P again where the map stays in the frame: within 6e-3 = half a grey level (2e-3) plus
    twice the bilinear error bound h^2/8 |P''| <= 1.2e-3 per axis for these periods.  With the coefficients negated -- the map
    applied in the wrong direction -- it is far off."""
    H, W = 120, 160
    K = ref.camera_matrix(129.0, 129.3, 79.6, 60.4)
    dist = ref.tum_camera()["dist"]
    vd, ud = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, v = ref.undistort_points(ud, vd, K, dist)
    xd, yd = ref.distort((u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], dist)
    assert np.abs(K[0, 0] * xd + K[0, 2] - ud).max() < 1e-9 and np.abs(K[1, 1] * yd + K[1, 2] - vd).max() < 1e-9     # the inversion converged
    raw = np.rint(ref.pinhole_pattern(u, v) * 255).astype(np.uint8)
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    want = np.moveaxis(ref.pinhole_pattern(uu, vv), -1, 0)
    inside = ~ref.taps_leaving(*ref.undistort_map(H, W, K, dist), H, W)
    assert inside.mean() > 0.9
    err = np.abs(ref.ingest(raw, K, dist, bgr=False) - want)[:, inside].max()
    wrong = np.abs(ref.ingest(raw, K, tuple(-d for d in dist), bgr=False) - want)[:, inside].max()
    print(f"pinhole image recovered to {err:.2e} on {inside.mean():.1%} of the pixels; wrong direction {wrong:.2f}")
    assert err <= 6e-3
    assert wrong > 0.3


def test_zero_distortion_is_the_identity_and_image_tt():
    from super_primitive_amd.tool.etc import image_tt
    raw = ref.noise_frames(1, 9, 14, 5)[0]
    for dist in (None, (0.0,) * 5, (0.0,) * 8):
        got = ref.ingest(raw, ref.small_camera(9, 14), dist, bgr=False)
        assert np.array_equal(got, np.moveaxis(raw, -1, 0) / 255.0)
    assert np.array_equal(ref.ingest(raw, ref.small_camera(9, 14), None, bgr=True), np.moveaxis(raw[..., ::-1], -1, 0) / 255.0)
    # the float32 anchor of the device kernel: float32(v) / 255.0f is what image_tt computes
    assert np.array_equal(image_tt(raw, "cpu").numpy(), np.moveaxis(raw, -1, 0).astype(np.float32) / np.float32(255.0))


def test_intrinsics_are_exact():
    from super_primitive_amd.frontend.frame_ingest import FrameIngest
    c = ref.tum_camera()
    fi = FrameIngest(c["K"], c["dist"], size=c["size"], crop=c["margins"], downsample_pow=1)
    K = c["K"]
    assert fi.out_size == (224, 288) and fi.crop_size == (448, 576)
    want_crop = np.array([[K[0, 0], 0, K[0, 2] - 32], [0, K[1, 1], K[1, 2] - 16], [0, 0, 1]])
    assert fi.K_crop.dtype == torch.float32 and np.array_equal(fi.K_crop.numpy(), want_crop.astype(np.float32))
    want_kf = want_crop.copy()
    want_kf[0] *= 288 / 576
    want_kf[1] *= 224 / 448
    assert fi.K_kf.dtype == torch.float32 and np.array_equal(fi.K_kf.numpy(), want_kf.astype(np.float32))
    assert np.array_equal(fi.K_kf.numpy(), ref.intrinsics(K, c["size"], c["margins"], 1))
    # an odd size scales the two axes differently (tool/camera.py:13-22)
    odd = FrameIngest(ref.small_camera(13, 17), None, size=(13, 17), downsample_pow=1)
    K = ref.small_camera(13, 17)
    assert odd.out_size == (6, 8)
    want = np.array([[K[0, 0] * (8 / 17), 0, K[0, 2] * (8 / 17)], [0, K[1, 1] * (6 / 13), K[1, 2] * (6 / 13)], [0, 0, 1]])
    assert np.array_equal(odd.K_kf.numpy(), want.astype(np.float32))
    assert np.array_equal(odd.intrinsics(0).numpy(), K.astype(np.float32)) and odd.output_size(0) == (13, 17)
    for bad in (dict(dist=(0.1, 0.2, 0.3)), dict(crop=(7, 0)), dict(downsample_pow=5), dict(size=None)):
        with pytest.raises(ValueError):
            FrameIngest(K, **dict(dict(dist=None, size=(13, 17)), **bad))


@pytest.mark.parametrize("shape,margins,size", [((12, 16), (0, 0), None), ((12, 16), (1, 2), (5, 6)), ((13, 17), (0, 0), (6, 8)),
                                                ((13, 17), (2, 1), (7, 11)), ((480, 640), (16, 32), (224, 288))],
                         ids=lambda s: "x".join(map(str, s)) if s else "full")
def test_depth_restatement_is_numpy_and_interpolate_nearest(shape, margins, size):
    raw = ref.depth_frames(1, *shape, 9)[0]
    got = ref.depth(raw, margins=margins, size=size)
    want = raw.astype(np.float32) * (1 / 5000)                                       # DepthScale: float32 array times a Python float
    assert want.dtype == np.float32
    want[want > 10] = 0.0                                                            # DepthFilter
    want = want[margins[0]:shape[0] - margins[0], margins[1]:shape[1] - margins[1]]
    if size is not None:
        want = F.interpolate(torch.from_numpy(np.ascontiguousarray(want))[None, None], size=size, mode="nearest")[0, 0].numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got == 0).any() and (got > 9).any() and (raw.astype(np.float64) / 5000 > 10).any()


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    import abi_header
    from super_primitive_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp_hip.h")).read()
    for cite in ("data/tum_undistort.py:113", "data/image_transforms.py:36-60", "frontend/process_frame.py:170-189",
                 "frontend/process_frame.py:257-270", "tool/camera.py:13-22", "data/tum_undistort.py:16-36", "odometery/odometery.py:152-156"):
        assert cite in header, cite
    prototypes = abi_header.parse()[0]
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and prototypes[name][2][-1] == "stream", name      # (void* stream, last: the rule for every launch)
    assert len(_lib.SpCamera._fields_) == 12                                   # fx fy cx cy and OpenCV's eight coefficients


def test_argument_checks():
    """Everything the entry points refuse is refused before any device work, so this runs without a GPU: the device addresses are
    never dereferenced (the camera is host memory and real)."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    one, other = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    cam = _lib.SpCamera(500.0, 500.0, 320.0, 240.0)
    pc = ctypes.addressof(cam)

    def image(raw=one, B=1, H=48, W=64, cam=pc, top=2, left=4, Hc=44, Wc=56, Ho=22, Wo=28, out=other):
        return lib.sp_frame_ingest(raw, B, H, W, cam, top, left, Hc, Wc, Ho, Wo, 1, out, None)

    def depth(raw=one, B=1, H=48, W=64, top=2, left=4, Hc=44, Wc=56, Ho=22, Wo=28, out=other):
        return lib.sp_depth_ingest(raw, B, H, W, 0.0002, 10.0, top, left, Hc, Wc, Ho, Wo, out, None)

    assert image(cam=None) == -1
    for call in (image, depth):
        assert call(raw=None) == -1 and call(out=None) == -1
        assert call(out=one) == -1                                                   # out must not be raw itself
        for size in ("B", "H", "W", "Hc", "Wc", "Ho", "Wo"):
            assert call(**{size: 0}) == -1 and call(**{size: -3}) == -1, size
        assert call(top=-1) == -1 and call(left=-1) == -1                            # a crop that leaves the frame
        assert call(top=5) == -1 and call(left=9) == -1 and call(Hc=47) == -1 and call(Wc=61) == -1
        assert call(top=2 ** 31 - 1) == -1 and call(left=2 ** 31 - 1) == -1
        assert call(W=32768, Wc=56) == -2
        assert call(H=65539, W=32767) == -2 and call(H=70000, W=32000) == -2         # H W >= 2^31
        assert call(B=65536) == -2
        assert call(Ho=65536) == -2
    for fx, fy in ((0.0, 500.0), (500.0, -1.0), (float("nan"), 500.0), (500.0, float("inf"))):
        bad = _lib.SpCamera(fx, fy, 320.0, 240.0)
        assert image(cam=ctypes.addressof(bad)) == -2, (fx, fy)
    assert image(B=0, cam=ctypes.addressof(_lib.SpCamera(0.0, 0.0, 0.0, 0.0))) == -1  # EINVAL comes first


def test_host_tensors_wrong_types_and_shapes_are_refused():
    from super_primitive_amd.frontend.frame_ingest import FrameIngest
    from super_primitive_amd.odometery import depth_init
    from super_primitive_amd.image.keyframe import KeyFrame
    fi = FrameIngest(ref.small_camera(12, 16), ref.MILD, size=(12, 16), crop=(1, 2))
    raw = torch.from_numpy(ref.noise_frames(2, 12, 16, 0))
    raw16 = torch.from_numpy(ref.depth_frames(2, 12, 16, 0))
    for call, arg in ((fi.images, raw), (fi.images, raw[0]), (fi.supp_keyframes, raw), (fi.supp_keyframe, raw[0]), (fi.depth, raw16),
                      (fi.depth, raw16[0])):
        with pytest.raises(RuntimeError, match="HIP-only"):
            call(arg)
        with pytest.raises(RuntimeError, match="HIP-only"):
            call(arg.numpy())
    kf = KeyFrame(torch.zeros(3, 4, 6), torch.eye(3), torch.zeros(2, 4, 6), torch.zeros(2, 2), torch.ones(2, 4, 6, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="HIP-only"):
        depth_init.keypoint_logdepths_from_depth(kf, torch.ones(4, 6))
    with pytest.raises(RuntimeError, match="HIP-only"):
        depth_init.keypoint_logdepths_from_depth(kf, np.ones((4, 6), dtype=np.float32))
