"""Independent reference of the point-table set-up (include/sp_hip.h, "Segment table construction" and "Batched preparation"): numpy,
float64 unless stated, written from the header's contracts and the reference formulas it names -- not from the kernels.

    table_ref          the compacted points of a keyframe on a pixel lattice: torch.where order, pixel words, log-depths, kp_L
    padded_layout      where those points sit in a batch's padded tables
    source_ref         a point's depth, its re-projection into its own frame (xn, yn), the validity bit and its distance from the band
    sample_ref         bilinear sample of a pyramid level at (xn, yn) with a PER-POINT error bound
    blur_decimate_ref  one pyramid step          pack_ref  planar -> HWC3
    position_replay_f32  the float32 operation order of the contract, for the host test that fixes C_POS
    check_*            the comparisons of tests/test_gpu_point_table.py (the host test feeds them planted errors)

The error bound of a colour.  The device computes the sampling position in float32, the reference in float64; at level 0 the exact
position of every ordinary point is an integer pixel, so the float32 position falls on either side of a cell edge and NO pair of
implementations takes the same four taps.  Zeros-padded bilinear interpolation is continuous and piecewise bilinear, so a position error
(ex, ey) moves the value by at most ex Sx + ey Sy, where Sx (Sy) is the largest absolute difference of horizontally (vertically) adjacent
taps of the cells the two positions can lie in: the 3 x 3 pixels around the pixel nearest to the exact position, on the level padded with
zeros.  Hence, per point and channel,

    bound = dx Sx + dy Sy + C_ARITH 2^-24 max|tap|,     dx = C_POS 2^-24 W,  dy = C_POS 2^-24 H   (W, H: the FULL-resolution size)

C_ARITH = 8.  With the position given, the contract's interpolation is  nw (1-wx)(1-wy) + ne wx (1-wy) + sw (1-wx) wy + se wx wy,  summed
left to right.  wx = ix - floor(ix) is exact.  Each of the four terms carries at most 4 roundings in a chain (1 - wx, 1 - wy, the weight
product, the product with the tap) and the three additions one each, on partial sums no larger than max|tap| (the weights sum to 1):
7 units of 2^-24 to first order -- a fused multiply-add only removes roundings -- and 8 covers the second-order terms.

C_POS = 6.1.  tests/test_point_table_ref_host.py replays the contract's float32 operation order (position_replay_f32) on every point of
every case at every level, with exp moved by -2, 0 and +2 ulp, against the float64 position: the worst distance it finds is 3.048 in units of
2^-24 dim (dim = W for columns, H for rows; reached on 50 x 84).  C_POS is twice that figure, rounded up to the next tenth; the host test
fails if the replay ever exceeds C_POS / 2.
"""
import numpy as np

f32 = np.float32
C_ARITH = 8.0
C_POS = 6.1
U24 = 2.0 ** -24
BAND = 0.99


# ---------------------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------------------
def keypoint_pixel(kp, dim, _alter=None):
    """round_half_even(0.5 (dim - 1) (kp + 1)) in float32, a negative index wrapped once, then clamped."""
    v = (f32(0.5) * f32(dim - 1)) * (np.asarray(kp, f32) + f32(1.0))
    idx = (np.floor(v.astype(np.float64) + 0.5) if _alter == "half_up" else np.rint(v)).astype(np.int64)
    idx = np.where(idx < 0, idx + dim, idx)
    return np.clip(idx, 0, dim - 1)


def table_ref(masks, logdepth, keypoints, stride=1, _alter=None):
    """The table of the mask pixels whose row and column are multiples of ``stride``: dict(counts (N,) int64, seg (P,) segment of every
    point, pix (P,) uint32 words (row << 16) | col, baseL (P,) float32 -- the log-depths themselves --, kp_L (N,) float32), points in
    torch.where order: segment by segment, row-major."""
    masks = np.asarray(masks, bool)
    N, H, W = masks.shape
    on_r, on_c = np.arange(H) % stride == (1 if _alter == "lattice_1" and stride > 1 else 0), np.arange(W) % stride == 0
    lat = masks & on_r[None, :, None] & on_c[None, None, :]
    if _alter == "column_major":
        seg, col, row = np.nonzero(lat.transpose(0, 2, 1))
    else:
        seg, row, col = np.nonzero(lat)
    L = np.asarray(logdepth, f32)
    kr, kc = keypoint_pixel(keypoints[:, 0], H, _alter), keypoint_pixel(keypoints[:, 1], W, _alter)
    return dict(counts=np.bincount(seg, minlength=N).astype(np.int64), seg=seg, pix=((row.astype(np.uint32) << np.uint32(16)) | col.astype(np.uint32)),
                baseL=L[seg, row, col], kp_L=L[np.arange(N), kr, kc])


def padded_layout(counts, granule):
    """Every segment's run starts at a multiple of ``granule``: (pos (P,) table position of every real point, pad (total,) bool mask of
    the padding, total)."""
    counts = np.asarray(counts, np.int64)
    pc = (counts + granule - 1) // granule * granule
    start = np.concatenate(([0], np.cumsum(pc)))
    own = np.concatenate(([0], np.cumsum(counts)))
    pos = np.repeat(start[:-1] - own[:-1], counts) + np.arange(int(counts.sum()))
    pad = np.ones(int(start[-1]), bool)
    pad[pos] = False
    return pos, pad, int(start[-1])


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry of a table point in its own frame
# ---------------------------------------------------------------------------------------------------------------------------------
def source_ref(table, K, kld, H, W, _band=BAND):
    """d = exp(L + kld_n - kp_L_n); the point back-projected with d and re-projected into its own frame, with the reference's
    ``zinv = 1e-6`` branch for |d| <= 1e-6 (such a point lands on the principal point); xn, yn in [-1, 1] (align-corners);
    ok = |xn| <= 0.99 and |yn| <= 0.99 and d > 1e-7.  Returns dict(d, xn, yn, ok, margin): margin = min(||xn| - 0.99|, ||yn| - 0.99|)."""
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    seg = table["seg"]
    col, row = (table["pix"] & 0xffff).astype(np.float64), ((table["pix"] >> 16) & 0x7fff).astype(np.float64)
    shift = np.asarray(kld, f32).astype(np.float64) - table["kp_L"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.exp(table["baseL"].astype(np.float64) + shift[seg])
        x, y = (col - cx) * d / fx, (row - cy) * d / fy
        zinv = np.where(np.abs(d) > 1e-6, 1.0 / np.where(d == 0, 1.0, d), 1e-6)
        u, v = x * fx * zinv + cx, y * fy * zinv + cy
        xn, yn = 2.0 * u / (W - 1) - 1.0, 2.0 * v / (H - 1) - 1.0
        ok = (np.abs(xn) <= _band) & (np.abs(yn) <= _band) & (d > 1e-7)
        margin = np.minimum(np.abs(np.abs(xn) - BAND), np.abs(np.abs(yn) - BAND))
    return dict(d=d, xn=xn, yn=yn, ok=ok, margin=margin)


def level_position(xn, size):
    """grid_sample's align-corners pixel coordinate of a normalised one at a level ``size`` pixels wide"""
    return (xn + 1.0) * 0.5 * (size - 1)


def position_replay_f32(table, K, kld, H, W, Hl, Wl, exp_ulps=0):
    """(ix, iy) of every point as the contract's operation order gives them in float32, every operation rounded once (numpy float32
    arrays): back-projection (col - cx) d / fx, pinhole x fx zinv + cx, 2 u (1 / (W - 1)) - 1, ((xn + 1) 0.5) (Wl - 1).  ``exp_ulps`` moves
    the exponential by that many float32 steps (a device exp is not correctly rounded)."""
    K = np.asarray(K, f32)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    seg = table["seg"]
    col, row = (table["pix"] & 0xffff).astype(f32), ((table["pix"] >> 16) & 0x7fff).astype(f32)
    shift = np.asarray(kld, f32) - table["kp_L"]
    d = np.exp((table["baseL"] + shift[seg]).astype(np.float64)).astype(f32)
    for _ in range(abs(exp_ulps)):
        d = np.nextafter(d, f32(np.inf if exp_ulps > 0 else 0.0))
    zinv = np.where(np.abs(d) > f32(1e-6), f32(1.0) / d, f32(1e-6))
    out = []
    for p, c, f, dim, dim_l in ((col, cx, fx, W, Wl), (row, cy, fy, H, Hl)):
        x = ((p - c) * d) / f
        u = (x * f) * zinv + c
        n = (f32(2.0) * u) * (f32(1.0) / f32(dim - 1)) - f32(1.0)
        out.append(((n + f32(1.0)) * f32(0.5)) * f32(dim_l - 1))
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------------------
def sample_ref(image_level, xn, yn, full_hw, _alter=None):
    """Bilinear sample (align-corners, taps outside the level read as zero) of a planar (C,Hl,Wl) level at the normalised positions:
    (value (C,P) float64, bound (C,P)) -- see the module docstring for the bound; ``full_hw`` = the full-resolution (H, W).  Positions must
    lie within a pixel of the level (every table point does: it re-projects onto its own pixel or onto the principal point); a NaN position
    gives a NaN value and bound."""
    img = np.asarray(image_level, np.float64)
    C, Hl, Wl = img.shape
    R = 3                                                   # rings of padding: zeros (or, planted error, the border replicated)
    pad = np.pad(img, ((0, 0), (R, R), (R, R)), mode="edge" if _alter == "replicate" else "constant")
    zpad = np.pad(img, ((0, 0), (R, R), (R, R)))
    nan = np.isnan(xn) | np.isnan(yn)
    ix, iy = level_position(np.where(nan, 0.0, xn), Wl), level_position(np.where(nan, 0.0, yn), Hl)
    assert (ix > -1.5).all() and (ix < Wl + 0.5).all() and (iy > -1.5).all() and (iy < Hl + 0.5).all()
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    wx, wy = ix - x0, iy - y0
    tap = lambda dy, dx: pad[:, y0 + dy + R, x0 + dx + R]
    nw, ne, sw, se = tap(0, 0), tap(0, 1), tap(1, 0), tap(1, 1)
    if _alter == "swap_ne_sw":
        ne, sw = sw, ne
    val = nw * ((1 - wx) * (1 - wy)) + ne * (wx * (1 - wy)) + sw * ((1 - wx) * wy) + se * (wx * wy)
    # the 3 x 3 pixels around the nearest pixel of the exact position, on the zero-padded level
    rx, ry = np.rint(ix).astype(np.int64), np.rint(iy).astype(np.int64)
    T = np.stack([np.stack([zpad[:, ry + dy + R, rx + dx + R] for dx in (-1, 0, 1)], axis=-1) for dy in (-1, 0, 1)], axis=-2)      # (C,P,3,3)
    Sx = np.abs(np.diff(T, axis=-1)).max(axis=(-1, -2))
    Sy = np.abs(np.diff(T, axis=-2)).max(axis=(-1, -2))
    H, W = full_hw
    bound = C_POS * U24 * (W * Sx + H * Sy) + C_ARITH * U24 * np.abs(T).max(axis=(-1, -2))
    val[:, nan], bound[:, nan] = np.nan, np.nan
    return val, bound


def blur_decimate_ref(img, _alter=None):
    """(C,H,W) -> (C,ceil(H/2),ceil(W/2)): reflect pad 1, [1 2 1; 2 4 2; 1 2 1] / 16, keep even rows and columns.  A dimension of one pixel
    has nothing to reflect onto and pads with the pixel itself (a 1-pixel level blurs to itself)."""
    img = np.asarray(img, np.float64)
    C, H, W = img.shape
    mode = lambda n: "edge" if n == 1 else ("symmetric" if _alter == "reflect_off_by_one" else "reflect")
    p = np.pad(img, ((0, 0), (1, 1), (0, 0)), mode=mode(H))
    p = np.pad(p, ((0, 0), (0, 0), (1, 1)), mode=mode(W))
    w = (1.0, 2.0, 1.0)
    acc = np.zeros_like(img)
    for dy in range(3):
        for dx in range(3):
            acc += (w[dy] * w[dx] / 16.0) * p[:, dy:dy + H, dx:dx + W]
    return acc[:, 0::2, 0::2]


def pyramid_ref(img, n_levels):
    out = [np.asarray(img, np.float64)]
    for _ in range(n_levels - 1):
        out.append(blur_decimate_ref(out[-1]))
    return out


def pack_ref(chw):
    """planar (3,H,W) -> HWC3"""
    return np.ascontiguousarray(np.asarray(chw).transpose(1, 2, 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# comparisons (what the GPU test asserts; every point takes part in every one of them)
# ---------------------------------------------------------------------------------------------------------------------------------
def check_table(counts, pix, baseL, kp_L, ref, what=""):
    """counts, pixel words (validity bit masked off), log-depths and kp_L equal the reference's exactly (floats bit for bit)"""
    assert np.array_equal(np.asarray(counts, np.int64), ref["counts"]), f"{what}: counts"
    got = np.asarray(pix).view(np.uint32) & np.uint32(0x7fffffff)
    assert got.shape == ref["pix"].shape and np.array_equal(got, ref["pix"]), f"{what}: pixel words"
    if baseL is not None:
        assert np.array_equal(np.asarray(baseL, f32).view(np.uint32), ref["baseL"].view(np.uint32)), f"{what}: log-depths"
    if kp_L is not None:
        assert np.array_equal(np.asarray(kp_L, f32).view(np.uint32), ref["kp_L"].view(np.uint32)), f"{what}: kp_L"


def check_validity(pix, ok, what=""):
    """bit 31 of every pixel word equals the reference's validity"""
    got = (np.asarray(pix).view(np.uint32) >> np.uint32(31)) == 1
    bad = np.nonzero(got != ok)[0]
    assert bad.size == 0, f"{what}: validity bit differs on {bad.size} points, first at {bad[:5]}"


def check_rgb(rgb, val, bound, what=""):
    """|rgb - val| <= bound on every point and channel (rgb (P,3) float32 of the device, val / bound (3,P)); returns the worst err / bound"""
    if rgb.shape[0] == 0:
        return 0.0
    err = np.abs(np.asarray(rgb, np.float64).T - val)
    assert np.isfinite(err).all() and (bound > 0).all(), f"{what}: non-finite colour"
    ratio = err / bound
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: err / bound = {worst:.3g} at point {int(ratio.max(axis=0).argmax())}"
    return worst


def check_bitwise(got, ref, what=""):
    """a float32 device array equals the float64 reference, which must itself be exact in float32"""
    ref = np.asarray(ref, np.float64)
    assert np.array_equal(ref.astype(f32).astype(np.float64), ref), f"{what}: the reference is not exact in float32"
    got = np.asarray(got, f32)
    assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.astype(f32).view(np.uint32)), f"{what}: not bitwise the reference"


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference of one case of tests/point_table_cases.py, computed once per process and shared by the tests (read-only)
# ---------------------------------------------------------------------------------------------------------------------------------
class CaseRef:
    def __init__(self, c, n_levels=3):
        import point_table_cases as cases
        self.c, self.n_levels = c, n_levels
        self._tables, self._sources, self._samples = {}, {}, {}
        self.kld = c["kld"] if "kld" in c else cases.seeds(c, self.table(1)["kp_L"])
        self.levels = pyramid_ref(c["image"], n_levels)
        self.trg_levels = pyramid_ref(c["trg_image"], n_levels)

    def table(self, stride):
        if stride not in self._tables:
            self._tables[stride] = table_ref(self.c["masks"], self.c["logdepth"], self.c["keypoints"], stride)
        return self._tables[stride]

    def source(self, stride):
        if stride not in self._sources:
            self._sources[stride] = source_ref(self.table(stride), self.c["K"], self.kld, self.c["H"], self.c["W"])
        return self._sources[stride]

    def sample(self, stride, level):
        """(value, bound) of every point of the stride's table at a pyramid level"""
        if (stride, level) not in self._samples:
            s = self.source(stride)
            self._samples[(stride, level)] = sample_ref(self.levels[level], s["xn"], s["yn"], (self.c["H"], self.c["W"]))
        return self._samples[(stride, level)]


_CASE_REFS = {}


def case_ref(name):
    import point_table_cases as cases
    if name not in _CASE_REFS:
        _CASE_REFS[name] = CaseRef(cases.nan_case() if name == "nan" else cases.case(name))
    return _CASE_REFS[name]
