"""-m gpu: the frame ingest (sp_frame_ingest, sp_depth_ingest) through ``FrameIngest`` against the float64 restatement
tests/frame_ingest_ref.py (pinned to torch's float64 ops and an analytic pinhole image by test_frame_ingest_host.py), and the
ground-truth-depth start built on it.

Images are compared at EVERY pixel: bilinear sampling with a zero border is continuous in the map, so there is no knife edge to
excuse.  Bound 2e-6: the weights come from float64 coordinates and the value is a float32 convex combination of <= 16 taps in
[0, 255] followed by one division -- <= 16 roundings of 2^-24 relative, about 1e-6, taken twice.  Depth is bitwise."""
import functools

import numpy as np
import pytest
import torch

from gpu_util import T, npy
import frame_ingest_ref as ref
import segment_depth_ref

pytestmark = pytest.mark.gpu

BOUND = 2e-6


def _ingest(case, **over):
    from super_primitive_amd.frontend.frame_ingest import FrameIngest
    c = dict(case, **over)
    return FrameIngest(c["K"], c["dist"], size=c["size"], crop=c["margins"], downsample_pow=c["downsample_pow"], bgr=c.get("bgr", True))


def _want(case, raw, bgr=True):
    return ref.ingest(raw, case["K"], case["dist"], case["margins"], case["downsample_pow"], bgr=bgr)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_images_match_the_float64_restatement_at_every_pixel(name):
    case = ref.CASES[name]
    raw = ref.noise_frames(1, *case["size"], 100)[0]
    fi = _ingest(case)
    got = fi.images(T(raw))
    want = _want(case, raw)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == want.shape == (3, *fi.out_size)
    err = np.abs(npy(got).astype(np.float64) - want).max()
    print(f"{name}: max abs error {err:.2e}")
    assert err <= BOUND
    if name == "7x9_rational_p0":
        assert (want == 0).any() and (want > 0.5).any()                             # taps that left the frame, and ones that did not


def test_rgb_input_keeps_the_channel_order():
    case = ref.CASES["12x16_crop_p1"]
    raw = ref.noise_frames(1, *case["size"], 101)[0]
    rgb, bgr = _ingest(case, bgr=False).images(T(raw)), _ingest(case, bgr=True).images(T(raw))
    assert np.abs(npy(rgb).astype(np.float64) - _want(case, raw, bgr=False)).max() <= BOUND
    assert torch.equal(rgb.flip(0), bgr) and not torch.equal(rgb, bgr)


@pytest.mark.parametrize("name", ["12x16_crop_p1", "40x70_wave_tail_p0"])
def test_a_batch_is_its_single_launches_bit_for_bit(name):
    case = ref.CASES[name]
    raw = ref.noise_frames(3, *case["size"], 102)
    fi = _ingest(case)
    batch = fi.images(T(raw))
    assert tuple(batch.shape) == (3, 3, *fi.out_size)
    singles = [fi.images(T(raw[b])) for b in range(3)]
    assert not torch.equal(singles[0], singles[1]) and not torch.equal(singles[1], singles[2])
    for b in range(3):
        assert torch.equal(batch[b], singles[b]), b
        assert np.abs(npy(batch[b]).astype(np.float64) - _want(case, raw[b])).max() <= BOUND


def test_the_working_size_with_the_fixtures_camera():
    """480 x 640 -> crop 32 / 16 -> 224 x 288, once; downsample_pow=0 of the same object gives the full undistorted crop."""
    case = ref.tum_case()
    raw = ref.noise_frames(1, *case["size"], 103)[0]
    fi = _ingest(case)
    assert fi.out_size == (224, 288)
    got = fi.images(T(raw))
    err = np.abs(npy(got).astype(np.float64) - _want(case, raw)).max()
    full = fi.images(T(raw), downsample_pow=0)
    err0 = np.abs(npy(full).astype(np.float64) - _want(dict(case, downsample_pow=0), raw)).max()
    print(f"480x640 -> 224x288: max abs error {err:.2e}; -> 448x576: {err0:.2e}")
    assert tuple(full.shape) == (3, 448, 576)
    assert err <= BOUND and err0 <= BOUND


def test_identity_ingest_is_image_tt_bit_for_bit():
    from super_primitive_amd.frontend.frame_ingest import FrameIngest
    from super_primitive_amd.tool.etc import image_tt
    raw = ref.noise_frames(2, 40, 70, 104)
    assert len(np.unique(raw)) == 256                                              # every byte value
    for dist in (None, (0.0,) * 8):
        fi = FrameIngest(ref.small_camera(40, 70), dist, size=(40, 70), downsample_pow=0, bgr=False)
        got = fi.images(T(raw))
        for b in range(2):
            assert torch.equal(got[b], image_tt(raw[b], "cuda:0"))
    flipped = FrameIngest(ref.small_camera(40, 70), None, size=(40, 70), downsample_pow=0, bgr=True).images(T(raw[0]))
    assert torch.equal(flipped, image_tt(np.ascontiguousarray(raw[0][..., ::-1]), "cuda:0"))


@pytest.mark.parametrize("shape,margins,size", [((12, 16), (0, 0), None), ((12, 16), (1, 2), (5, 6)), ((13, 17), (0, 0), (6, 8)),
                                                ((13, 17), (2, 1), (7, 11)), ((40, 70), (0, 1), (20, 67)), ((480, 640), (16, 32), (224, 288))],
                         ids=lambda s: "x".join(map(str, s)) if s else "full")
def test_depth_is_the_restatement_bit_for_bit(shape, margins, size):
    from super_primitive_amd.frontend.frame_ingest import FrameIngest
    raw = ref.depth_frames(2, *shape, 105)
    fi = FrameIngest(ref.small_camera(*shape), None, size=shape, crop=margins)
    got = fi.depth(T(raw), size=size)
    want = np.stack([ref.depth(raw[b], margins=margins, size=size) for b in range(2)])
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(_bits(npy(got)), _bits(want))
    metres = raw[:, margins[0]:shape[0] - margins[0], margins[1]:shape[1] - margins[1]].astype(np.float64) / 5000
    assert (metres > 10.001).any() and ((metres > 5) & (metres < 9.999)).any() and (metres == 0).any()       # both sides of max_depth
    one = fi.depth(T(raw[1]), size=size)
    assert one.dim() == 2 and torch.equal(one, got[1])
    # another scale and threshold
    near = fi.depth(T(raw[0]), scale=1e-3, max_depth=3.5, size=size)
    assert np.array_equal(_bits(npy(near)), _bits(ref.depth(raw[0], 1e-3, 3.5, margins, size)))


@functools.lru_cache(maxsize=None)
def _reinit_keyframe():
    from super_primitive_amd.image.keyframe import KeyFrame
    masks, L, keypoints, est, _ = segment_depth_ref.reinit_keyframe()
    N, H, W = masks.shape
    kf = KeyFrame(torch.zeros(3, H, W, device="cuda:0"), T(np.eye(3, dtype=np.float32)), T(L), T(keypoints), T(masks))
    return kf, keypoints, est


def _keypoint_pixels(keypoints, shape):
    """tool/point_utils.py:37-40 in numpy: align-corners de-normalisation, rounded half to even."""
    dims = np.array(shape, dtype=np.float32)
    return np.rint(np.float32(0.5) * (dims - 1) * (keypoints + 1)).astype(np.int64)


def test_keypoint_logdepths_are_the_log_of_the_depth_at_the_keypoints():
    from super_primitive_amd.odometery.depth_init import keypoint_logdepths_from_depth
    kf, keypoints, _ = _reinit_keyframe()
    depth = np.random.default_rng(106).uniform(0.4, 9.0, (96, 160)).astype(np.float32)       # twice the keyframe's size, all valid
    kp = _keypoint_pixels(keypoints, depth.shape)
    assert len(np.unique(kp, axis=0)) > 5
    got = keypoint_logdepths_from_depth(kf, T(depth))
    want = torch.log(T(depth[kp[:, 0], kp[:, 1]]))
    assert got.dtype == torch.float32 and torch.equal(got, want)


def test_keypoint_logdepths_fall_back_to_the_segment_median_on_an_invalid_depth():
    """Every pixel of the hand-made estimate twice along both axes: the keypoints land on its invalid pixels, the nearest resize to
    the keyframe's 48 x 80 gives the estimate back, and the result is segment_based_depth_reinit's median (pinned in
    test_gpu_segment_depth.py)."""
    from super_primitive_amd.odometery.depth_init import keypoint_logdepths_from_depth, segment_based_depth_reinit
    kf, keypoints, est = _reinit_keyframe()
    depth = np.repeat(np.repeat(est, 2, axis=0), 2, axis=1)
    kp = _keypoint_pixels(keypoints, depth.shape)
    assert (depth[kp[:, 0], kp[:, 1]] < 1e-6).any()
    resized = depth[ref.nearest_axis(96, 48)][:, ref.nearest_axis(160, 80)]
    assert np.array_equal(resized, est)
    got = keypoint_logdepths_from_depth(kf, T(depth))
    want = segment_based_depth_reinit(T(resized), kf, mode="median")
    assert torch.equal(got, want) and bool(torch.isfinite(got).all()) and len(torch.unique(got)) > 5
    # one invalid keypoint is enough
    ok = np.full((96, 160), np.float32(2.0))
    ok[kp[3, 0], kp[3, 1]] = 0.0
    got = keypoint_logdepths_from_depth(kf, T(ok))
    assert torch.equal(got, segment_based_depth_reinit(T(ok[ref.nearest_axis(96, 48)][:, ref.nearest_axis(160, 80)]), kf, mode="median"))


def test_supp_keyframes_are_keyframes_the_pyramid_accepts():
    from super_primitive_amd.image.keyframe import KeyFrame, keyframe_pyramid
    case = ref.CASES["40x70_wave_tail_p0"]
    raw = ref.noise_frames(3, *case["size"], 107)
    fi = _ingest(case, downsample_pow=1)
    frames = fi.supp_keyframes(T(raw))
    images = fi.images(T(raw))
    assert len(frames) == 3 and fi.out_size == (20, 35)
    for b, kf in enumerate(frames):
        assert isinstance(kf, KeyFrame) and kf.is_supporting()
        assert torch.equal(kf.image, images[b]) and kf.image.is_contiguous()
        assert kf.K.dtype == torch.float32 and kf.K.is_cuda and np.array_equal(_bits(npy(kf.K)), _bits(fi.K_kf.numpy()))
        assert np.array_equal(npy(kf.K), ref.intrinsics(case["K"], case["size"], case["margins"], 1))
    levels = keyframe_pyramid(frames[1], 0, 2)
    assert len(levels) == 2 and tuple(levels[-1].image.shape) == (3, 20, 35)
    one = fi.supp_keyframe(T(raw[2]))
    assert torch.equal(one.image, frames[2].image) and torch.equal(one.K, frames[2].K)


def test_wrong_types_and_shapes_are_refused():
    case = ref.CASES["12x16_crop_p1"]
    fi = _ingest(case)
    raw = T(ref.noise_frames(1, 12, 16, 108)[0])
    raw16 = T(ref.depth_frames(1, 12, 16, 108)[0])
    for bad in (raw.float(), raw[:, :, :2], raw[:10], raw[None, None], raw[0]):                  # dtype, channels, size, dimensions
        with pytest.raises(ValueError):
            fi.images(bad)
    for bad in (T(np.zeros((12, 16), np.float32)), T(np.zeros((12, 16), np.int16)), raw16[:10], raw16[None, None], raw16[0]):
        with pytest.raises(ValueError):
            fi.depth(bad)
    with pytest.raises(ValueError):
        fi.supp_keyframes(raw)
    with pytest.raises(ValueError):
        fi.supp_keyframe(raw[None])
    with pytest.raises(RuntimeError, match="SP_EINVAL"):
        fi.depth(raw16, size=(0, 4))
