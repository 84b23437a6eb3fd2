"""float64 numpy restatement of the frame ingest (include/sp_hip.h "Frame ingest"), written from its formulae: the undistortion map
(OpenCV's initUndistortRectifyMap with R = I, newCameraMatrix = K), the bilinear remap with a zero border, the crop, the
align_corners=False bilinear resize, and the depth scale / filter / crop / nearest resize.  Plus the seeded input makers and the
shapes the tests use.  cv2 itself is not available to the tests, so this -- checked against torch's own float64 ops and an analytic
pinhole image in test_frame_ingest_host.py -- is the yardstick of the device kernels."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def camera_matrix(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def tum_camera():
    """The one real calibration (settings-only fixture): dict(size=(H,W), K, dist, margins=(mh,mw))."""
    with open(os.path.join(GOLDEN, "tum_fr1_camera.json")) as f:
        c = json.load(f)
    return dict(size=(c["height"], c["width"]), K=camera_matrix(c["fx"], c["fy"], c["cx"], c["cy"]), dist=tuple(c["dist"]),
                margins=(c["margin_h"], c["margin_w"]))


def coefficients(dist):
    """(k1, k2, p1, p2, k3, k4, k5, k6); absent ones are 0."""
    d = np.zeros(8)
    if dist is not None:
        d[:len(dist)] = dist
    return d


def distort(x, y, dist):
    """Normalised pinhole coordinates -> normalised distorted coordinates."""
    k1, k2, p1, p2, k3, k4, k5, k6 = coefficients(dist)
    r2 = x * x + y * y
    kr = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    return (x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x),
            y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)


def undistort_map(H, W, K, dist):
    """(mx, my), each (H,W) float64: where pixel (u, v) of the undistorted frame samples the raw one."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xd, yd = distort((u - cx) / fx, (v - cy) / fy, dist)
    return fx * xd + cx, fy * yd + cy


def remap(image, mx, my):
    """Bilinear sample of image (H,W,C) at (mx, my): taps floor and floor + 1, a tap outside the frame contributes 0.  float64."""
    H, W = image.shape[:2]
    img = image.astype(np.float64)
    x0, y0 = np.floor(mx), np.floor(my)
    ax, ay = mx - x0, my - y0
    out = np.zeros(mx.shape + image.shape[2:])
    for dy, wy in ((0, 1 - ay), (1, ay)):
        for dx, wx in ((0, 1 - ax), (1, ax)):
            # (clip before the integer cast: a strong distortion sends the map far outside)
            px, py = np.clip(x0 + dx, -1, W).astype(np.int64), np.clip(y0 + dy, -1, H).astype(np.int64)
            inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
            tap = img[np.where(inside, py, 0), np.where(inside, px, 0)]
            out += np.where(inside, wy * wx, 0.0)[..., None] * tap
    return out


def taps_leaving(mx, my, H, W):
    """Pixels whose footprint has at least one tap outside the frame."""
    return (np.floor(mx) < 0) | (np.floor(mx) + 1 > W - 1) | (np.floor(my) < 0) | (np.floor(my) + 1 > H - 1)


def resize_axis(n_in, n_out):
    """F.interpolate(bilinear, align_corners=False) along one axis: i0, i1, weight of i1."""
    s = np.maximum((np.arange(n_out) + 0.5) * n_in / n_out - 0.5, 0.0)
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, n_in - 1), s - i0


def resize_bilinear(image, Ho, Wo):
    """image (Hc,Wc,C) float64 -> (Ho,Wo,C)."""
    i0, i1, wi = resize_axis(image.shape[0], Ho)
    j0, j1, wj = resize_axis(image.shape[1], Wo)
    rows = (1 - wi)[:, None, None] * image[i0] + wi[:, None, None] * image[i1]
    return (1 - wj)[None, :, None] * rows[:, j0] + wj[None, :, None] * rows[:, j1]


def two_by_two_mean(image):
    """The shortcut that is NOT the resize for sizes not divisible by 2."""
    H, W = image.shape[0] // 2, image.shape[1] // 2
    return image[:2 * H, :2 * W].reshape(H, 2, W, 2, -1).mean((1, 3))


def ingest(raw, K, dist, margins=(0, 0), downsample_pow=0, bgr=True):
    """raw (H,W,3) uint8 -> (3,Ho,Wo) float64 in [0,1]: undistort, crop, resize, / 255, channels reversed when bgr."""
    H, W = raw.shape[:2]
    mh, mw = margins
    mx, my = undistort_map(H, W, K, dist)
    cropped = remap(raw, mx, my)[mh:H - mh, mw:W - mw]
    Ho, Wo = cropped.shape[0] // 2 ** downsample_pow, cropped.shape[1] // 2 ** downsample_pow
    out = resize_bilinear(cropped, Ho, Wo) / 255.0
    return np.moveaxis(out[..., ::-1] if bgr else out, -1, 0)


def intrinsics(K, size, margins=(0, 0), downsample_pow=0):
    """float32 (3,3) of the ingested image, computed in float64."""
    Hc, Wc = size[0] - 2 * margins[0], size[1] - 2 * margins[1]
    Ho, Wo = Hc // 2 ** downsample_pow, Wc // 2 ** downsample_pow
    K = np.array(K, dtype=np.float64)
    K[0, 2] -= margins[1]
    K[1, 2] -= margins[0]
    K[0] *= Wo / Wc
    K[1] *= Ho / Hc
    return K.astype(np.float32)


def nearest_axis(n_in, n_out):
    """torch's nearest rule along one axis (float32 scale)."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def depth(raw, scale=1 / 5000, max_depth=10.0, margins=(0, 0), size=None):
    """raw (H,W) uint16 -> float32 metres: scaled in float32, far values zeroed, cropped, nearest-resized to ``size``."""
    H, W = raw.shape
    d = raw.astype(np.float32) * np.float32(scale)
    d[d > np.float32(max_depth)] = 0.0
    d = d[margins[0]:H - margins[0], margins[1]:W - margins[1]]
    if size is not None:
        d = d[nearest_axis(d.shape[0], size[0])][:, nearest_axis(d.shape[1], size[1])]
    return np.ascontiguousarray(d)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def noise_frames(B, H, W, seed):
    """Independent uniform bytes: the worst case for the weights (neighbouring taps differ by up to 255)."""
    return np.random.default_rng(seed).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)


def depth_frames(B, H, W, seed):
    """uint16 depths of 0 .. 65535: at the default scale 0 .. 13.1 m, so both sides of max_depth = 10 occur, zeros included."""
    raw = np.random.default_rng(seed).integers(0, 65536, size=(B, H, W), dtype=np.uint16)
    raw[:, ::3, ::4] = 0
    raw[:, 1::5, 2::7] = 50000                                     # 10 m at 1 / 5000, to a float32 rounding: the filter's own edge
    return raw


def small_camera(H, W, focal=0.9):
    """A camera for an H x W test frame: focal length ``focal`` widths, principal point off the centre and off the pixel grid."""
    return camera_matrix(focal * W, focal * W * 1.01, 0.5 * W - 0.3, 0.5 * H + 0.2)


MILD = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)                  # five coefficients
RATIONAL = (0.9, -0.4, 0.05, -0.04, 0.3, 0.2, -0.1, 0.05)         # eight, strong: at f = 0.6 W the map leaves the frame at the rim

# name -> dict(size, K, dist, margins, downsample_pow): the smallest shapes that exercise each way of going wrong
CASES = {
    "7x9_rational_p0": dict(size=(7, 9), K=small_camera(7, 9, 0.6), dist=RATIONAL, margins=(0, 0), downsample_pow=0),
    "12x16_crop_p1": dict(size=(12, 16), K=small_camera(12, 16), dist=MILD, margins=(1, 2), downsample_pow=1),
    "13x17_odd_p1": dict(size=(13, 17), K=small_camera(13, 17), dist=MILD, margins=(0, 0), downsample_pow=1),
    "21x30_p2": dict(size=(21, 30), K=small_camera(21, 30), dist=MILD[:4], margins=(0, 0), downsample_pow=2),
    "40x70_wave_tail_p0": dict(size=(40, 70), K=small_camera(40, 70), dist=MILD, margins=(0, 0), downsample_pow=0),
}


def tum_case():
    c = tum_camera()
    return dict(size=c["size"], K=c["K"], dist=c["dist"], margins=c["margins"], downsample_pow=1)


def pinhole_pattern(u, v):
    """The analytic image of the direction test, (..., 3) in [0.05, 0.95]."""
    c = np.arange(3.0)
    u, v = u[..., None], v[..., None]
    return 0.5 + 0.25 * np.sin(2 * np.pi * (u / 32 + v / 57 + c / 3)) + 0.2 * np.cos(2 * np.pi * (u / 71 - v / 29 + c / 5))


def undistort_points(ud, vd, K, dist, iterations=50):
    """Raw pixel (ud, vd) -> pinhole pixel (u, v): the inverse of the map by fixed-point iteration on the normalised coordinates."""
    k1, k2, p1, p2, k3, k4, k5, k6 = coefficients(dist)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    xd, yd = (ud - cx) / fx, (vd - cy) / fy
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        inv_kr = (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3) / (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3)
        dx, dy = 2 * p1 * x * y + p2 * (r2 + 2 * x * x), p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - dx) * inv_kr, (yd - dy) * inv_kr
    return fx * x + cx, fy * y + cy
