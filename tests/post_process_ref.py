"""Yardstick of the keyframe post-processing stage (csrc/sp_frontend.hip: sp_depth_discontinuity, sp_label_components, sp_collect_parts,
sp_build_part_masks, sp_kth_mask_pixel and sp_mask_count as their scan), written from the contract in include/sp_hip.h -- numpy and
scipy.ndimage.label (which oracle/frontend_oracle.py already uses), no GPU.  The full stage is ``oracle.frontend_oracle.fix_disconnected``,
which the reference's own goldens pin; this file restates the pieces so that each entry point can be compared on every pixel.

``discontinuity_ref``  float64:  depth = exp(L) (L is the float32 input, widened), -1 at invalid pixels;  pooled = fs x fs max, stride 1,
    -inf outside the image (a NaN wins, like max_pool2d);  reflect padding by 1 (index -1 -> 1, n -> n - 2);  gx, gy = the Scharr pair
    [[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]] / 32 and its transpose, all nine taps multiplied (0 * inf = NaN, like conv2d);
    g = sqrt(gx^2 + gy^2);  discontinuity = valid & (g > threshold), threshold rounded to float32 first, as the device and torch read it.

``disc_bound``  how far a float32 evaluation of g may lie from the float64 one: DISC_C * U * max(1, max |pooled| over the 3 x 3 window),
    U = 2^-24.  One float32 rounding moves x by at most U |x|; contraction to FMA only removes roundings.  With M = that maximum:
      taps     expf is documented at 1 ulp by HIP's math API (<= 2 U |x|); the max selects, it does not round; -1 is exact.  The six weighted
               taps of one gradient carry |weights| = 32 in all: 2 U M * 32 = 64 U M on the unscaled sum
      scaling  3 v and 10 v round once each: U (3 + 10 + 3 + 3 + 10 + 3) M = 32 U M
      sums     five additions; the partial sums are bounded by the running |weights| (6, 16, 26, 29, 32) M for gx and (13, 16, 19, 29, 32) M
               for gy: 109 U M either way
      1 / 32   a power of two: exact.  E = (64 + 32 + 109) / 32 U M = 6.41 U M on gx and on gy
      g        the magnitude is 1-Lipschitz in (gx, gy): sqrt(2) E = 9.06 U M;  the two squares (U each, relative), their sum (U) and sqrtf
               (documented at 1 ulp = 2 U; halved and added): 3 U g relative, and g <= sqrt(2) M because |gx|, |gy| <= 32 M / 32:
               4.25 U M
    DISC_C = ceil(9.06 + 4.25) = 14.  A valid pixel is ``ambiguous`` when |g - threshold| <= disc_bound: there, and only there, a float32
    evaluation may decide the other way.

``label_ref``  per slice, 4-connected: labels = 1 + the smallest linear index (over the whole (N, H, W) array) of the pixel's component,
    0 on background; sizes[root] = pixels of the component, 0 everywhere else.
"""
import numpy as np
import scipy.ndimage

U = 2.0 ** -24
DISC_C = 14
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
SCHARR = np.array([[-3.0, 0.0, 3.0], [-10.0, 0.0, 10.0], [-3.0, 0.0, 3.0]]) / 32.0


def _reflect_pad(a):
    """(N, H, W) -> (N, H + 2, W + 2), index -1 -> 1 and n -> n - 2 (torch's 'reflect'; at n = 2 both fold onto the other pixel)."""
    H, W = a.shape[-2:]
    rows = [1] + list(range(H)) + [H - 2]
    cols = [1] + list(range(W)) + [W - 2]
    return a[:, rows][:, :, cols]


def max_pool(depth, fs):
    """fs x fs maximum, stride 1, -inf outside; a NaN in the window wins."""
    N, H, W = depth.shape
    h = fs // 2
    p = np.full((N, H + 2 * h, W + 2 * h), -np.inf)
    p[:, h:h + H, h:h + W] = depth
    out = np.full((N, H, W), -np.inf)
    for dy in range(fs):
        for dx in range(fs):
            out = np.maximum(out, p[:, dy:dy + H, dx:dx + W])        # np.maximum propagates NaN
    return out


def disc_bound(pooled):
    """DISC_C * U * max(1, max |pooled|) over the reflect-padded 3 x 3 window of every pixel."""
    N, H, W = pooled.shape
    a = _reflect_pad(np.abs(pooled))
    m = np.ones((N, H, W))
    for dy in range(3):
        for dx in range(3):
            m = np.maximum(m, a[:, dy:dy + H, dx:dx + W])
    return DISC_C * U * m


def discontinuity_ref(L, valid, filter_size=3, threshold=0.1):
    """Returns dict(g, pooled, disc, split, ambiguous, bound, threshold) -- float64 / bool arrays of shape (N, H, W)."""
    L = np.asarray(L, np.float32).astype(np.float64)
    valid = np.asarray(valid, bool)
    N, H, W = L.shape
    thr = float(np.float32(threshold))
    with np.errstate(all="ignore"):
        depth = np.where(valid, np.exp(L), -1.0)
        pooled = max_pool(depth, int(filter_size))
        p = _reflect_pad(pooled)
        gx, gy = np.zeros((N, H, W)), np.zeros((N, H, W))
        for dy in range(3):
            for dx in range(3):
                tap = p[:, dy:dy + H, dx:dx + W]
                gx = gx + SCHARR[dy, dx] * tap
                gy = gy + SCHARR[dx, dy] * tap
        g = np.sqrt(gx * gx + gy * gy)
        bound = disc_bound(pooled)
        disc = valid & (g > thr)
        ambiguous = valid & (np.abs(g - thr) <= bound)
    return dict(g=g, pooled=pooled, disc=disc, split=valid & ~disc, ambiguous=ambiguous, bound=bound, threshold=thr)


def label_ref(fg):
    """(labels int32 (N, H, W), sizes int32 (N * H * W)) as sp_label_components defines them."""
    fg = np.asarray(fg, bool)
    N, H, W = fg.shape
    labels = np.zeros((N, H, W), np.int32)
    sizes = np.zeros(N * H * W, np.int32)
    lin = np.arange(N * H * W).reshape(N, H, W)
    for n in range(N):
        lab, k = scipy.ndimage.label(fg[n], structure=FOUR)
        if k == 0:
            continue
        idx = np.arange(1, k + 1)
        roots = scipy.ndimage.minimum(lin[n], lab, idx).astype(np.int64)
        count = scipy.ndimage.sum(np.ones((H, W)), lab, idx).astype(np.int64)
        labels[n] = np.where(lab > 0, roots[np.maximum(lab, 1) - 1] + 1, 0)
        sizes[roots] = count
    return labels, sizes


def flood_fill_labels(fg):
    """The same contract without scipy: scan in linear order, flood every unlabelled foreground pixel's component from it (so the seed IS
    the smallest linear index)."""
    fg = np.asarray(fg, bool)
    N, H, W = fg.shape
    labels = np.zeros((N, H, W), np.int32)
    sizes = np.zeros(N * H * W, np.int32)
    for n in range(N):
        for r0 in range(H):
            for c0 in range(W):
                if not fg[n, r0, c0] or labels[n, r0, c0]:
                    continue
                root = (n * H + r0) * W + c0
                stack = [(r0, c0)]
                labels[n, r0, c0] = root + 1
                while stack:
                    r, c = stack.pop()
                    sizes[root] += 1
                    for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                        if 0 <= rr < H and 0 <= cc < W and fg[n, rr, cc] and not labels[n, rr, cc]:
                            labels[n, rr, cc] = root + 1
                            stack.append((rr, cc))
    return labels, sizes


def renumber(labels):
    """Consecutive numbers in (slice, row, col) scan order of the roots -- ndimage.label's numbering, slice after slice."""
    flat = np.asarray(labels).reshape(-1)
    roots = np.unique(flat[flat > 0])
    out = np.searchsorted(roots, flat) + 1
    return np.where(flat > 0, out, 0).reshape(np.shape(labels)).astype(np.int32), len(roots)


def collect_parts_ref(labels, sizes, masks, split):
    """(set of (slice, root, size), n_parts, bg_sizes (N)): one triple per root pixel; bg_sizes[n] = |masks[n] & !split[n]|."""
    labels, masks, split = np.asarray(labels), np.asarray(masks, bool), np.asarray(split, bool)
    N, H, W = labels.shape
    flat = labels.reshape(-1)
    roots = np.nonzero(flat == np.arange(flat.size) + 1)[0]
    parts = {(int(r // (H * W)), int(r), int(np.asarray(sizes).reshape(-1)[r])) for r in roots}
    return parts, len(roots), (masks & ~split).reshape(N, -1).sum(1).astype(np.int32)


def part_masks_ref(masks, split, labels, desc):
    """desc rows {slice, kind, root}: kind 0 = masks & (labels == root + 1), 1 = masks & !split, 2 = masks."""
    masks, split, labels = np.asarray(masks, bool), np.asarray(split, bool), np.asarray(labels)
    out = []
    for n, kind, root in np.asarray(desc).reshape(-1, 3):
        out.append(masks[n] & (labels[n] == root + 1) if kind == 0 else masks[n] & ~split[n] if kind == 1 else masks[n].copy())
    return np.stack(out)


def kth_pixel_ref(mask, kth):
    """(row, col) of the kth set pixel in raster order."""
    return np.argwhere(np.asarray(mask, bool))[kth]


def mask_count_ref(masks):
    """(row_counts (K * H): exclusive per-mask scan of the per-row counts, counts (K), seg_off (K + 1)) of sp_mask_count."""
    masks = np.asarray(masks, bool)
    per_row = masks.sum(2)
    row_counts = np.cumsum(per_row, 1) - per_row
    counts = per_row.sum(1)
    return row_counts.reshape(-1).astype(np.int32), counts.astype(np.int32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
