"""The truth for the four SE(3) device functions of super_primitive_amd/csrc/sp_solve_device.h (se3_exp_times, se3_retract_left, se3_exp_d,
renormalise_rotation), independent of their formulas -- numpy / scipy, no GPU.

Exponential.  ``exp_se3`` is scipy's matrix exponential of the 4x4 twist matrix in float64 and ``d_exp_se3`` its derivative by the complex
step (h = 1e-30): neither has a branch on theta.  ``retract`` / ``retract_grad`` are T = Exp(xi) X and ga_k = sum_ij (d_k Exp(xi) X)_ij G_ij
over the top 3x4.  tests/test_se3_ref_host.py holds both against mpmath at 80 digits.

Magnitude companion (``magnitudes``).  The same expressions with every term replaced by its absolute value: the sum a float32 evaluation
could lose against.  With W = [phi]x, t = theta^2 and the three coefficient functions A(t), B(t), C(t) (f_j(t) = sum_k (-t)^k / (2k+1+j)!)

    mag E = I + Am |W| + Bm |W||W|           mag V = I + Bm |W| + Cm |W||W|
    mag T = mag E |X_R|   |   mag E |X_t| + mag V |tau|
    dmag_k E = A'm 2|phi_k| |W| + Am |G_k| + B'm 2|phi_k| |W||W| + Bm (|G_k||W| + |W||G_k|)        (k rotational; G_k = d W / d phi_k)
    dmag_k T = dmag_k E |X_R|  |  dmag_k E |X_t| + dmag_k V |tau|   (k rotational),     column k of mag V in the translation (k translational)

where a coefficient's magnitude is Am = |A| + |t A'| and A'm = |A'| + |t A''|: the device evaluates A at ITS theta^2, a float32 sum of three
float32 squares, so every rounding of that sum moves A by |t A'| 2^-24 whatever |A| is (near theta = pi, A = sin theta / theta vanishes and
t A' = -1/2 does not).  Without that term no count of roundings bounds a correct float32 evaluation near pi.

Bound on a device entry: OPS * 2^-24 * magnitude, OPS = the float32 roundings that can reach that kind of entry, counted from se3_exp_times
and k_se3_retract (not measured).  Rules: a product carries the roundings of both factors + 1, a sum those of its worse term + 1 (relative
to the sum of absolute values); a product with an exact 0 or +-1 and a sum with an exact 0 do not round; FMA contraction only removes
roundings.  nv = roundings in a value, nd = in a derivative part of the dual number:

    t = a3 a3 + a4 a4 + a5 a5            nv 3 (product 1, two sums)      nd 0 (2 a_k, exact)
    A, B, C (float64, rounded once)      nv 4 = t's 3 + 1
    dA/dt, ... (the same)                4;  chain(): dA * t.d           nd 5
    W                                    exact
    W2 = 3 products, 2 sums              nv 3                            nd 3 (a.d b.v + a.v b.d: exact products, 1 sum; 2 sums)
    A W                                  nv 5 = 4 + 0 + 1                nd 7 = max(5 + 0, 4 + 0) + 2
    B W2                                 nv 8 = 4 + 3 + 1                nd 10 = max(5 + 3, 4 + 3) + 2
    E = (I + A W) + B W2                 nv 9 = max(5 + 1, 8) + 1        nd 11 = max(7, 10) + 1     (I.d = 0: the first sum is exact)
    V                                    the same
    T_rot = X E + X E + X E              nv 12 = 9 + 1 + 2               nd 14 = 11 + 1 + 2
    dt = V a + V a + V a                 nv 12 = 9 + 1 + 2               nd 15 = max(11 + 0 + 1, 9) + 1 + 2
    T_trans = (X E + X E + X E) + dt     nv 13                           nd 16 = max(14, 15) + 1
    ga_k = fmaf chain over 12 entries    each entry's nd + one rounding per non-zero G entry (fmaf(d, 0, s) = s is exact)

Renormalisation.  The float32 restatement and its count are window_gn_step_ref.renormalise_rotation / RENORM_OPS (imported, not copied);
``renormalise_rotation_f64`` evaluates the same definition in float64 with the same candidate.  The 0.1 clamp of the definition cannot be
reached: the four radicands sum to 4 for every finite input, so the largest root is at least 1 -- there is no case for it.

Edge tables: ``edge_twists()`` (every theta^2 at which se3_exp_times changes method or loses digits, x 3 axis directions x 4 translation
sizes), ``POSES`` (identity and a general pose) and ``rotation_table()`` (every quaternion candidate clean and noisy, and two exact ties).

The float32 restatement of the device's algorithm (``exp_times_f32``, ``retract_grad_f32``) is written from the formulas in the header's
comments; the host file proves that it stays inside the bounds, so the bounds are ones the correct algorithm meets, and that each planted
error (``plant=``) leaves them on a listed case.
"""
import numpy as np
from scipy.linalg import expm

from window_gn_step_ref import RENORM_OPS, renormalise_rotation  # noqa: F401  (re-exported)

f32 = np.float32
U = 2.0 ** -24          # unit roundoff of float32
H = 1e-30               # complex step
REF_REL = 1e-13         # the truth's own error, relative to the largest magnitude of a matrix (ref_error)

OPS_ROT, OPS_TRANS = 12, 13                  # value of a rotation / translation entry of Exp(a) X (table above)
OPS_D_ROT, OPS_D_TRANS = 14, 16              # derivative part of the same
PAIR_ULPS = 2           # se3_retract_left from the identity: one rounding of the float64 product + the solve's 1e-9 on entries down to 1e-6
FOLD_ULPS = 1           # se3_exp_d from the identity: a float64 product rounded once


# ---------------------------------------------------------------------------------------------------------------------------------
# the truth
# ---------------------------------------------------------------------------------------------------------------------------------
def hat(xi):
    """4x4 twist matrix of xi = [tau, phi] (..., 6), real or complex."""
    xi = np.asarray(xi)
    M = np.zeros(xi.shape[:-1] + (4, 4), xi.dtype if np.iscomplexobj(xi) else np.float64)
    x, y, z = xi[..., 3], xi[..., 4], xi[..., 5]
    M[..., 0, 1], M[..., 0, 2], M[..., 1, 0], M[..., 1, 2], M[..., 2, 0], M[..., 2, 1] = -z, y, z, -x, -y, x
    M[..., :3, 3] = xi[..., :3]
    return M


def exp_se3(xi):
    """Exp of the twist(s) xi (..., 6) -> (..., 4, 4), float64."""
    return expm(hat(np.asarray(xi, np.float64)))


def d_exp_se3(xi):
    """d Exp(xi) / d xi_k, k = 0..5 -> (..., 6, 4, 4), by the complex step."""
    xi = np.asarray(xi, np.float64)
    out = np.empty(xi.shape[:-1] + (6, 4, 4))
    for k in range(6):
        z = xi.astype(np.complex128)
        z[..., k] += 1j * H
        out[..., k, :, :] = expm(hat(z)).imag / H
    return out


def retract(xi, X):
    """Exp(xi) X, float64 (..., 4, 4)."""
    return exp_se3(xi) @ np.asarray(X, np.float64)


def retract_jacobian(xi, X):
    """d (Exp(xi) X) / d xi_k (..., 6, 4, 4)."""
    return d_exp_se3(xi) @ np.asarray(X, np.float64)[..., None, :, :]


def retract_grad(xi, X, G):
    """ga_k = sum over the top 3x4 of (d_k Exp(xi) X) G (..., 6)."""
    return (retract_jacobian(xi, X)[..., :3, :] * np.asarray(G, np.float64)[..., None, :3, :]).sum((-1, -2))


# ---------------------------------------------------------------------------------------------------------------------------------
# the magnitude companion and the bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def coefficient_table(t, terms=48):
    """f[j][o] = the o-th derivative (o = 0, 1, 2) with respect to t of f_j(t) = sum_k (-t)^k / (2k+1+j)!, j = 0, 1, 2 (A, B, C), by the plain
    series.  Only ever used for magnitudes (its own cancellation, 1e-14 at t = 50, is of no account there)."""
    t = np.asarray(t, np.float64)
    f = [[np.zeros_like(t) for _ in range(3)] for _ in range(3)]
    for j in range(3):
        fact = 1.0
        for i in range(2, 2 + j):
            fact *= i                                  # (1 + j)!
        for k in range(terms):
            if k:
                fact *= (2 * k + j) * (2 * k + 1 + j)
            c = (-1.0) ** k / fact
            f[j][0] = f[j][0] + c * t ** k
            if k >= 1:
                f[j][1] = f[j][1] + c * k * t ** (k - 1)
            if k >= 2:
                f[j][2] = f[j][2] + c * k * (k - 1) * t ** (k - 2)
    return f


GEN_ABS = np.abs(np.array([[[0, 0, 0], [0, 0, -1], [0, 1, 0]], [[0, 0, 1], [0, 0, 0], [-1, 0, 0]], [[0, -1, 0], [1, 0, 0], [0, 0, 0]]], np.float64))


def magnitudes(xi, X):
    """(mag (n, 3, 4), dmag (n, 6, 3, 4)) of T = Exp(xi) X and of dT / d xi_k for twists xi (n, 6) and poses X (n, 4, 4) or (4, 4)."""
    xi = np.abs(np.asarray(xi, np.float64)).reshape(-1, 6)
    n = len(xi)
    X = np.abs(np.broadcast_to(np.asarray(X, np.float64), (n, 4, 4)))
    tau, phi = xi[:, :3], xi[:, 3:]
    t = (phi * phi).sum(1)
    f = coefficient_table(t)
    cm = [(np.abs(f[j][0]) + t * np.abs(f[j][1]))[:, None, None] for j in range(3)]
    dm = [(np.abs(f[j][1]) + t * np.abs(f[j][2]))[:, None, None] for j in range(3)]
    W = np.einsum("nk,kij->nij", phi, GEN_ABS)
    W2 = W @ W
    I = np.eye(3)
    Em, Vm = I + cm[0] * W + cm[1] * W2, I + cm[1] * W + cm[2] * W2
    Rm, tm = X[:, :3, :3], X[:, :3, 3:]
    mag = np.concatenate([Em @ Rm, Em @ tm + Vm @ tau[:, :, None]], 2)
    dmag = np.zeros((n, 6, 3, 4))
    for k in range(3):
        dmag[:, k, :, 3] = Vm[:, :, k]
        s = 2 * phi[:, k, None, None]
        G = GEN_ABS[k]
        dW2 = G @ W + W @ G
        dE = dm[0] * s * W + cm[0] * G + dm[1] * s * W2 + cm[1] * dW2
        dV = dm[1] * s * W + cm[1] * G + dm[2] * s * W2 + cm[2] * dW2
        dmag[:, 3 + k] = np.concatenate([dE @ Rm, dE @ tm + dV @ tau[:, :, None]], 2)
    return mag, dmag


VALUE_OPS = np.array([OPS_ROT, OPS_ROT, OPS_ROT, OPS_TRANS], np.float64)
DERIV_OPS = np.array([OPS_D_ROT, OPS_D_ROT, OPS_D_ROT, OPS_D_TRANS], np.float64)


def ref_error(mag):
    """What the truth itself may be off by: scipy's expm is accurate relative to the LARGEST entry of a matrix, not to each entry (an entry
    of 1e-13 next to a translation of 30 carries 1e-16 of the 30), so 1e-13 of the largest magnitude of each 3x4; the host file holds
    exp_se3 and d_exp_se3 to exactly this against mpmath."""
    return REF_REL * mag.max((-1, -2), keepdims=True)


def value_bound(mag):
    """Allowed distance of a device T entry (n, 3, 4) from the truth."""
    return VALUE_OPS * U * mag + ref_error(mag)


def jacobian_bound(dmag):
    """Allowed distance of one derivative entry (n, 6, 3, 4)."""
    return DERIV_OPS * U * dmag + ref_error(dmag)


def grad_bound(dmag, G):
    """Allowed distance of ga (n, 6) for the upstream G (n, 4, 4) or (4, 4): every entry's own count plus one rounding of the fmaf chain per
    non-zero G entry."""
    G = np.abs(np.broadcast_to(np.asarray(G, np.float64), (len(dmag), 4, 4)))[:, None, :3, :]
    nnz = (G != 0).sum((-1, -2, -3))[:, None]
    return ((U * (DERIV_OPS + nnz[:, :, None, None]) * dmag + ref_error(dmag)) * G).sum((-1, -2))


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 restatement of se3_exp_times on dual numbers (from the header's comments), with the errors the host file plants
# ---------------------------------------------------------------------------------------------------------------------------------
def coefficients_device(t, plant=None):
    """A, B, C and their derivatives with respect to t = theta^2 the way the header states them: float64, a 10-term Horner series in t for
    t < 0.5 (A = sum (-t)^k / (2k+1)!, B = ... / (2k+2)!, C = ... / (2k+3)!), else sin / cos closed forms with d/dt = (1 / 2 theta) d/dtheta."""
    t = np.asarray(t, np.float64)
    ia, ib, ic = np.zeros(10), np.zeros(10), np.zeros(10)
    fact = 1.0
    for k in range(10):
        if k:
            fact *= (2 * k) * (2 * k + 1)
        ia[k], ib[k], ic[k] = 1 / fact, 1 / fact / (2 * k + 2), 1 / fact / (2 * k + 2) / (2 * k + 3)
    if plant == "ia3":
        ia[3] *= 1.1
    v, w = [np.zeros_like(t) for _ in range(3)], [np.zeros_like(t) for _ in range(3)]
    for k in range(9, -1, -1):
        sg = -1.0 if k & 1 else 1.0
        for i, c in enumerate((ia, ib, ic)):
            w[i] = w[i] * t + v[i]
            v[i] = v[i] * t + sg * c[k]
    with np.errstate(all="ignore"):
        th = np.sqrt(t)
        sn, cs = np.sin(th), np.cos(th)
        closed = [sn / th, (1 - cs) / t, (th - sn) / (t * th), (cs * th - sn) / (2 * t * th), (sn * th - 2 * (1 - cs)) / (2 * t * t),
                  ((1 - cs) * th - 3 * (th - sn)) / (2 * t * t * th)]
    if plant == "dc_sign":
        closed[5] = -closed[5]
    series = t < (5.0 if plant == "threshold" else 0.5)
    return [np.where(series, s, c) for s, c in zip(v + w, closed)]


class Dual:
    """float32 value (n,) and ND derivative parts (n, ND), with the operation order of the header's Dual<ND>."""

    def __init__(self, v, d):
        self.v, self.d = v, d
        assert v.dtype == f32 and d.dtype == f32

    def __add__(self, o):
        return Dual(self.v + o.v, self.d + o.d)

    def __neg__(self):
        return Dual(-self.v, -self.d)

    def __mul__(self, o):
        return Dual(self.v * o.v, self.d * o.v[:, None] + self.v[:, None] * o.d)

    def scaled(self, c):
        return Dual(c * self.v, c[:, None] * self.d)


def exp_times_f32(xi, X, plant=None):
    """(T (n, 3, 4), dT/da (n, 6, 3, 4)) in float32 the way se3_exp_times<6> forms Exp(a) X (no FMA: contraction only removes roundings)."""
    xi = np.asarray(xi, f32).reshape(-1, 6)
    n = len(xi)
    X = np.ascontiguousarray(np.broadcast_to(np.asarray(X, f32), (n, 4, 4)))
    eye = np.eye(6, dtype=f32)
    a = [Dual(xi[:, i].copy(), np.broadcast_to(eye[i], (n, 6)).copy()) for i in range(6)]
    const = lambda c: Dual(np.full(n, c, f32), np.zeros((n, 6), f32))
    th2 = a[3] * a[3] + a[4] * a[4] + a[5] * a[5]
    A, B, C, dA, dB, dC = (c.astype(f32) for c in coefficients_device(th2.v.astype(np.float64), plant))
    chain = lambda val, der: Dual(val, der[:, None] * th2.d)
    dA_, dB_, dC_ = chain(A, dA), chain(B, dB), chain(C, dC)
    z, one = const(0), const(1)
    W = [z, -a[5], a[4], a[5], z, -a[3], -a[4], a[3], z]
    W2 = [W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j] for i in range(3) for j in range(3)]
    E = [(one if i % 4 == 0 else z) + dA_ * W[i] + dB_ * W2[i] for i in range(9)]
    V = [(one if i % 4 == 0 else z) + dB_ * W[i] + dC_ * W2[i] for i in range(9)]
    T, D = np.zeros((n, 3, 4), f32), np.zeros((n, 6, 3, 4), f32)
    for i in range(3):
        dt = V[3 * i] * a[0] + V[3 * i + 1] * a[1] + V[3 * i + 2] * a[2]
        for j in range(4):
            r = E[3 * i].scaled(X[:, 0, j]) + E[3 * i + 1].scaled(X[:, 1, j]) + E[3 * i + 2].scaled(X[:, 2, j])
            if j == 3:
                r = r + dt
            T[:, i, j], D[:, :, i, j] = r.v, r.d
    return T, D


def retract_grad_f32(D, G):
    """k_se3_retract's fmaf chain over the 12 entries: ga (n, 6) float32 from the float32 derivative parts D (n, 6, 3, 4)."""
    G = np.broadcast_to(np.asarray(G, f32), (len(D), 4, 4))
    s = np.zeros((len(D), 6), f32)
    for i in range(3):
        for j in range(4):          # the product of two float32 is exact in float64: one rounding, as fmaf
            s = (D[:, :, i, j].astype(np.float64) * G[:, None, i, j].astype(np.float64) + s.astype(np.float64)).astype(f32)
    return s


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 restatement of se3_retract_left / se3_exp_d (the 2-, 3-term series and the closed form), with the errors the host file plants
# ---------------------------------------------------------------------------------------------------------------------------------
def exp_branches_f64(xi, which, plant=None):
    """Exp(xi) (4x4 float64) the way se3_retract_left (which = "retract": t < 1e-12 two terms, < 1e-4 three terms, else closed form) and
    se3_exp_d (which = "exp_d": t < 1e-4 three terms, else closed form) state it."""
    xi = np.asarray(xi, np.float64)
    wx, wy, wz = xi[3:]
    t = wx * wx + wy * wy + wz * wz
    s6, s24 = (8.0 if plant == "exp_d_6" else 6.0), (20.0 if plant == "retract_24" else 24.0)
    if which == "retract" and t < 1e-12:
        A, B, C = 1 - t / 6, 0.5 - t / s24, 1 / 6 - t / 120
    elif t < 1e-4:
        A, B, C = 1 - t / s6 * (1 - t / 20), 0.5 - t / s24 * (1 - t / 30), 1 / 6 - t / 120 * (1 - t / 42)
    else:
        th = np.sqrt(t)
        A, B, C = np.sin(th) / th, (1 - np.cos(th)) / t, (th - np.sin(th)) / (t * th)
    W = np.array([[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + A * W + B * W @ W
    M[:3, 3] = (np.eye(3) + B * W + C * W @ W) @ xi[:3]
    return M


# ---------------------------------------------------------------------------------------------------------------------------------
# renormalisation in float64
# ---------------------------------------------------------------------------------------------------------------------------------
def radicands(T16, dtype=np.float64):
    """The four radicands 1 +- m00 +- m11 +- m22 in the definition's order of operations."""
    M = np.asarray(T16, f32).ravel().astype(dtype)
    one = dtype(1)
    return np.array([one + M[0] + M[5] + M[10], one + M[0] - M[5] - M[10], one - M[0] + M[5] - M[10], one - M[0] - M[5] + M[10]], dtype)


def renormalise_rotation_f64(T16, plant=None):
    """window_gn_step_ref.renormalise_rotation's definition evaluated in float64 on the float32 input (the first maximum of the float64
    roots; the host file shows it is the float32 choice on every rotation of the table).  Returns (16 float64, candidate)."""
    M = np.asarray(T16, f32).ravel().astype(np.float64)
    q = np.sqrt(np.maximum(radicands(T16), 0))
    best = 0
    for i in (1, 2, 3):
        if (q[i] >= q[best]) if plant == "argmax_ge" else (q[i] > q[best]):
            best = i
    m01, m02, m10, m12, m20, m21 = M[1], M[2], M[4], M[6], M[8], M[9]
    a, b, c, d, e, f = m21 - m12, m02 - m20, m10 - m01, m10 + m01, m02 + m20, m12 + m21
    cand = [[q[0] * q[0], a, b, c], [a, q[1] * q[1], d, e], [b, d, q[2] * q[2], f], [c, e, f, q[3] * q[3]]][best]
    if plant == "ef_swap" and best in (1, 2):          # e <-> f in the fourth component
        cand[3] = f if best == 1 else e
    den = 2 * max(q[best], 0.1)
    r, x, y, z = (v / den for v in cand)
    s = 2 / (r * r + x * x + y * y + z * z)
    M[0], M[1], M[2] = 1 - s * (y * y + z * z), s * (x * y - z * r), s * (x * z + y * r)
    M[4], M[5], M[6] = s * (x * y + z * r), 1 - s * (x * x + z * z), s * (y * z - x * r)
    M[8], M[9], M[10] = s * (x * z - y * r), s * (y * z + x * r), 1 - s * (x * x + y * y)
    return M, best


def renorm_ulps(got16, want16):
    """Distance of the nine rotation entries in float32 ulp taken at max(|entry|, 1)."""
    g = np.asarray(got16, np.float64).reshape(-1, 16)[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]
    w = np.asarray(want16, np.float64).reshape(-1, 16)[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]
    return np.abs(g - w) / np.spacing(np.maximum(np.abs(w), 1).astype(f32)).astype(np.float64)


def own_ulps(got, want):
    """Distance in float32 ulp of every entry's OWN magnitude (an exact zero must be met exactly: inf otherwise)."""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    sp = np.spacing(np.abs(w).astype(f32)).astype(np.float64)
    d = np.abs(g - w)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, np.where(w == 0, np.inf, d / sp))


# ---------------------------------------------------------------------------------------------------------------------------------
# edge tables
# ---------------------------------------------------------------------------------------------------------------------------------
PI2, TAU2 = np.pi ** 2, (2 * np.pi) ** 2
THETA2 = [("0", 0.0),
          ("1e-12-", 1e-12 * (1 - 1e-3)), ("1e-12", 1e-12), ("1e-12+", 1e-12 * (1 + 1e-3)),
          ("1e-6-", 1e-6 * (1 - 1e-3)), ("1e-6", 1e-6), ("1e-6+", 1e-6 * (1 + 1e-3)),
          ("0.25", 0.25), ("0.49", 0.49), ("0.5-", 0.5 * (1 - 2.0 ** -20)), ("0.5", 0.5), ("0.5+", 0.5 * (1 + 2.0 ** -20)), ("0.51", 0.51),
          ("2", 2.0), ("pi2-", PI2 - 1e-3), ("pi2+", PI2 + 1e-3), ("4pi2-", TAU2 - 1e-3), ("4pi2+", TAU2 + 1e-3), ("50", 50.0)]
AXES = [("z", (0.0, 0.0, 1.0)), ("xz", (0.6, 0.0, -0.8)), ("xyz", (1 / 3, -2 / 3, 2 / 3))]          # axis-aligned, one zero component, general
# theta^2 = 0.5 exactly: 0.25 + 0.25 is exact in float32 with or without FMA, t < 0.5 is false -> the closed form
HALF_EXACT = [("xy", (0.5, 0.5, 0.0)), ("yz", (0.0, 0.5, -0.5)), ("zx", (-0.5, 0.0, 0.5))]
TRANSLATIONS = [0.0, 1e-3, 1.0, 30.0]
TAU_DIR = np.array([0.36, -0.48, 0.8])


def theta2_f32(phi):
    """theta^2 as the kernel sums it: float32 products, float32 sums, left to right."""
    p = np.asarray(phi, f32)
    return p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1] + p[..., 2] * p[..., 2]


def edge_twists():
    """(names, a (n, 6) float32): every theta^2 of THETA2 in three axis directions with translations of size 0, 1e-3, 1, 30."""
    names, rows = [], []
    for tname, t in THETA2:
        for aname, axis in (HALF_EXACT if tname == "0.5" else AXES):
            phi = np.asarray(axis) if tname == "0.5" else np.asarray(axis) * np.sqrt(t)
            for size in TRANSLATIONS:
                names.append(f"theta2={tname} axis={aname} |tau|={size:g}")
                rows.append(np.concatenate([TAU_DIR * size, phi]))
    return names, np.array(rows).astype(f32)


def general_pose():
    """A pose with a general rotation and |t| around 3, float32."""
    X = exp_se3(np.array([1.5, -2.0, 1.6, 0.4, -0.7, 0.9])).astype(f32)
    X[3] = (0, 0, 0, 1)
    return X


POSES = [("identity", np.eye(4, dtype=f32)), ("general", general_pose())]


def _rotation(axis, angle):
    axis = np.asarray(axis, np.float64)
    return exp_se3(np.concatenate([np.zeros(3), axis / np.linalg.norm(axis) * angle]))[:3, :3]


def rotation_table():
    """[(name, 4x4 float32, candidate, least lead of the winning radicand)]: each quaternion candidate with a lead of at least 0.1, clean and
    with 1e-3 noise on all nine entries, and two exact ties (float32-exact diagonal, noisy off-diagonals) that the first maximum decides."""
    rng = np.random.default_rng(11)
    out = []
    clean = [(0, _rotation((1, 2, 3), 0.4)), (1, _rotation((1, 0.02, -0.03), np.pi - 0.05)), (2, _rotation((0.03, 1, 0.02), np.pi - 0.04)),
             (3, _rotation((-0.02, 0.03, 1), np.pi - 0.03))]
    for cand, R in clean:
        for noisy in (0, 1):
            M = np.eye(4)
            M[:3, :3] = R + (rng.uniform(-1e-3, 1e-3, (3, 3)) if noisy else 0)
            M[:3, 3] = rng.uniform(-3, 3, 3)
            out.append((f"candidate {cand}" + (" noisy" if noisy else ""), M.astype(f32), cand, 0.1))
    for name, R, cand in (("tie 120 deg about (1,1,1)", [[0, 0, 1], [1, 0, 0], [0, 1, 0]], 0), ("tie 180 deg about (1,1,0)", [[0, 1, 0], [1, 0, 0], [0, 0, -1]], 1)):
        M = np.eye(4)
        M[:3, :3] = np.asarray(R, np.float64) + rng.uniform(-1e-3, 1e-3, (3, 3)) * (1 - np.eye(3))
        M[:3, 3] = rng.uniform(-3, 3, 3)
        out.append((name, M.astype(f32), cand, 0.0))
    return out


# the twists that steer se3_retract_left (the pair step) and se3_exp_d (the window's fold-in) into each of their branches.  The direction
# with a zero component makes R01 = B phi_x phi_y a pure second-order entry: from the identity pose it shows a wrong B at its own size.
# (Below theta^2 = 1e-4 only the general direction: such an entry would be 1e-13 there, where the truth's own 1e-16 is not negligible.)
GENERAL_DIR, ZERO_COMPONENT_DIR = np.array([1 / 3, -2 / 3, 2 / 3]), np.array([0.6, 0.8, 0.0])
BRANCH_TAU = np.array([0.25, -0.125, 0.0625])


def _branch_twists(theta2s, second_order_from):
    out = []
    for name, t in theta2s:
        for dname, d in (("general", GENERAL_DIR), ("zero component", ZERO_COMPONENT_DIR)):
            if dname == "general" or t >= second_order_from:
                out.append((f"theta2={name} {dname}", np.concatenate([BRANCH_TAU, d * np.sqrt(t)]).astype(f32).astype(np.float64)))
    return out


def pair_step_twists():
    """[(name, xi)] for se3_retract_left: theta^2 = 0 (tau != 0), either side of 1e-12, 1e-8, either side of 1e-4, 0.3."""
    return _branch_twists([("0", 0.0), ("1e-12-", 1e-12 * (1 - 1e-3)), ("1e-12+", 1e-12 * (1 + 1e-3)), ("1e-8", 1e-8), ("1e-4-", 1e-4 * (1 - 1e-3)),
                           ("1e-4+", 1e-4 * (1 + 1e-3)), ("0.3", 0.3)], 0.9e-4)


def fold_in_twists():
    """[(name, a)] for se3_exp_d: theta^2 = 1e-10, either side of 1e-4, 0.3 and 9."""
    return _branch_twists([("1e-10", 1e-10), ("1e-4-", 1e-4 * (1 - 1e-3)), ("1e-4+", 1e-4 * (1 + 1e-3)), ("0.3", 0.3), ("9", 9.0)], 0.9e-4)
