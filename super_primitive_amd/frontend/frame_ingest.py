"""Raw camera frames on the device -> ``KeyFrame``-ready images, intrinsics and depth maps, one native launch per batch of frames.

What the reference does on the host for every tracked frame (``frontend/process_frame.py:257-270`` ``process_to_supp_kf``; ``:207-255``
for keyframes): ``cv2.undistort`` of the 8-bit BGR frame (``data/tum_undistort.py:113``; ``data/image_transforms.py:36-60``), the
margin crop with ``cx - mw``, ``cy - mh`` and BGR -> RGB (``data/tum_undistort.py:86-90,127-130``), ``tool/etc.py`` ``image_tt`` and
``_downsample_to_target`` (``frontend/process_frame.py:170-189``: bilinear ``F.interpolate`` to ``(H // 2^p, W // 2^p)``, intrinsics
scaled per axis as ``tool/camera.py:13-22``).  Here that is ``sp_frame_ingest`` (include/sp_hip.h has the definition; DESIGN.md §4
"Frame ingest" what is and is not pinned), and ``sp_depth_ingest`` for the 16-bit depth of the ground-truth-depth start
(``data/tum_undistort.py:16-36,128``, ``odometery/odometery.py:152-156``).

The package ships no camera preset: calibration numbers are the caller's arguments."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _lib
from ..image.keyframe import KeyFrame


def _device_frames(raw, dtype, pixel_dims, what):
    """``raw`` as a contiguous batch on the device, and whether it came without the batch dimension."""
    if not torch.is_tensor(raw):
        raise RuntimeError(f"super_primitive_amd: the frame ingest is HIP-only; got a host array for {what}. "
                           "Pass a cuda tensor (no CPU fallback exists).")
    _lib.require_device(raw)
    if raw.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, got {raw.dtype}")
    single = raw.dim() == pixel_dims
    if raw.dim() not in (pixel_dims, pixel_dims + 1):
        raise ValueError(f"{what} must have {pixel_dims} or {pixel_dims + 1} dimensions, got {tuple(raw.shape)}")
    raw = raw.detach().contiguous()
    return (raw[None] if single else raw), single


class FrameIngest:
    """One camera: ``K`` (3,3), ``dist`` = OpenCV's ``(k1, k2, p1, p2[, k3[, k4, k5, k6]])`` or None, raw frames of ``size=(H,W)``,
    symmetric margins ``crop=(mh,mw)`` cut after undistortion (the reference's ``[mh:-mh, mw:-mw]``; (0,0): none), the keyframe size
    ``(Hc // 2^p, Wc // 2^p)`` for ``p = downsample_pow``, and whether raw frames are BGR (what ``cv2.imread`` gives).

    ``K_crop`` (the cropped frame's intrinsics), ``K_kf`` (the keyframe's) are float32 (3,3) host tensors, ``out_size`` is the
    keyframe's ``(Ho, Wo)``, ``camera`` the ``SpCamera`` record the native call reads."""

    def __init__(self, K, dist=None, size=None, crop=(0, 0), downsample_pow=1, bgr=True):
        K = np.array(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64)
        if K.shape != (3, 3):
            raise ValueError(f"K must be (3,3), got {K.shape}")
        d = np.zeros(0) if dist is None else np.array(dist, dtype=np.float64).ravel()
        if d.size not in (0, 4, 5, 8):
            raise ValueError(f"dist must hold 4, 5 or 8 coefficients (k1, k2, p1, p2[, k3[, k4, k5, k6]]), got {d.size}")
        if size is None:
            raise ValueError("size=(H, W) of the raw frames is required")
        self.size = (int(size[0]), int(size[1]))
        self.margins = (int(crop[0]), int(crop[1]))
        H, W = self.size
        mh, mw = self.margins
        if mh < 0 or mw < 0 or H - 2 * mh <= 0 or W - 2 * mw <= 0:
            raise ValueError(f"crop {self.margins} leaves nothing of a {H} x {W} frame")
        self.crop_size = (H - 2 * mh, W - 2 * mw)
        self.downsample_pow = int(downsample_pow)
        self.bgr = bool(bgr)
        self._K = K
        self.camera = _lib.SpCamera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], *d, *([0.0] * (8 - d.size)))
        self.K_crop = self.intrinsics(0)
        self.K_kf = self.intrinsics()
        self.out_size = self.output_size()
        self._K_dev = {}

    def output_size(self, downsample_pow=None):
        p = self.downsample_pow if downsample_pow is None else int(downsample_pow)
        Hc, Wc = self.crop_size
        Ho, Wo = Hc // 2 ** p, Wc // 2 ** p
        if p < 0 or Ho <= 0 or Wo <= 0:
            raise ValueError(f"downsample_pow {p} leaves nothing of a {Hc} x {Wc} frame")
        return Ho, Wo

    def intrinsics(self, downsample_pow=None):
        """float32 (3,3) intrinsics of the image ``images(raw, downsample_pow)`` returns: the principal point moved by the margins,
        then row 0 times ``Wo / Wc`` and row 1 times ``Ho / Hc``, all in float64."""
        Ho, Wo = self.output_size(downsample_pow)
        Hc, Wc = self.crop_size
        K = self._K.copy()
        K[0, 2] -= self.margins[1]
        K[1, 2] -= self.margins[0]
        K[0] *= Wo / Wc
        K[1] *= Ho / Hc
        return torch.from_numpy(K).float()

    def images(self, raw, downsample_pow=None):
        """``raw`` (H,W,3) or (B,H,W,3) uint8 on the device -> (3,Ho,Wo) or (B,3,Ho,Wo) float32 in [0,1], RGB.
        ``downsample_pow=0``: the full-resolution undistorted image (what ``keyframe_from_sam`` / ``keyframe_from_normals`` take)."""
        raw, single = _device_frames(raw, torch.uint8, 3, "raw")
        B, H, W, C = raw.shape
        if (H, W, C) != (*self.size, 3):
            raise ValueError(f"raw frames must be {(*self.size, 3)}, got {(H, W, C)}")
        Ho, Wo = self.output_size(downsample_pow)
        out = torch.empty(B, 3, Ho, Wo, dtype=torch.float32, device=raw.device)
        rc = _lib.load().sp_frame_ingest(_lib.ptr(raw), B, H, W, ctypes.addressof(self.camera), self.margins[0], self.margins[1],
                                         *self.crop_size, Ho, Wo, int(self.bgr), _lib.ptr(out), _lib.stream_ptr())
        _lib.check(rc, "sp_frame_ingest")
        return out[0] if single else out

    def _K_on(self, device):
        K = self._K_dev.get(device)
        if K is None:
            K = self._K_dev[device] = self.K_kf.to(device)
        return K

    def supp_keyframes(self, raw_batch):
        """``KeyFrame(image, K=K_kf)`` per frame of a (B,H,W,3) batch -- ``process_to_supp_kf`` with ``include_normals: False``;
        the list is what ``run_sequence`` / ``run_sequences`` take as ``frames``."""
        images = self.images(raw_batch)
        if images.dim() != 4:
            raise ValueError(f"raw_batch must be (B,H,W,3), got {tuple(raw_batch.shape)}")
        Ks = self._K_on(images.device).repeat(images.shape[0], 1, 1)
        return [KeyFrame(image, K=K) for image, K in zip(images, Ks)]

    def supp_keyframe(self, raw):
        """``supp_keyframes`` of one (H,W,3) frame."""
        image = self.images(raw)
        if image.dim() != 3:
            raise ValueError(f"raw must be (H,W,3), got {tuple(raw.shape)}")
        return KeyFrame(image, K=self._K_on(image.device).clone())

    def depth(self, raw_u16, scale=1 / 5000, max_depth=10.0, size=None):
        """``raw_u16`` (H,W) or (B,H,W) uint16 on the device -> float32 metres: ``v * scale`` in float32, values beyond ``max_depth``
        zeroed, the margins cut; ``size=(Ho,Wo)``: nearest-resized as ``F.interpolate(mode='nearest')`` does."""
        raw, single = _device_frames(raw_u16, torch.uint16, 2, "raw_u16")
        B, H, W = raw.shape
        if (H, W) != self.size:
            raise ValueError(f"raw depth frames must be {self.size}, got {(H, W)}")
        Ho, Wo = self.crop_size if size is None else (int(size[0]), int(size[1]))
        out = torch.empty(B, Ho, Wo, dtype=torch.float32, device=raw.device)
        rc = _lib.load().sp_depth_ingest(_lib.ptr(raw), B, H, W, float(scale), float(max_depth), self.margins[0], self.margins[1],
                                         *self.crop_size, Ho, Wo, _lib.ptr(out), _lib.stream_ptr())
        _lib.check(rc, "sp_depth_ingest")
        return out[0] if single else out
