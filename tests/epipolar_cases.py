"""Six named epipolar geometries for the F-dependent kernels.  numpy only; no fixture.

synth.make_scene has one camera pair, so every kernel that reads F or an epipole has only ever seen epipoles near
(5500, 1125) and (9246, 1435): far to the right of the image, positive coordinates, one sign of F.  The cases here move
the epipoles into the image, next to the origin, to the left, and out to 1e6 px:

    far_right        synth's K, R, t                           the control
    in_image         synth's K, R; t = (0.02, -0.03, 1)        e2 = (520, 470), e1 ~ (600, 499); 8 rows within 1 px of one
    unit             e1 = (0.6, 0.8), e2 = (-0.8, 0.6)         |e| = 1: the reference's f1 = f2 = 1 (M/MultiH.cpp:1127-1128)
                                                               is TRUE, step 1 is the textbook optimal triangulation
    near_origin      e1 = (3, -2), e2 = (-1, 4)                corrections of 1e-3 .. 1e-1 px, mixed-sign coordinates
    far_left         synth's K, R; t = (-0.40, -0.05, 0.08)    negative epipole coordinates; F multiplied by -1
    nearly_sideways  synth's K, R; t = (1, 0.1, 0.001)         |e| ~ 1e6: how much accuracy is left

A camera case has F = K^-T [t]x R K^-1, e2 = K t, e1 = K R^T t; the two constructed ones have
F = [e2]x A (I - e1 e1^T / e1^T e1) with A drawn from the case's own generator.  F has unit Frobenius norm, e1 and e2 are
the exact null vectors it was built from (third coordinate 1).

An epipole exactly at infinity (third coordinate 0: pure sideways translation with R = I) is OUT OF SCOPE: the reference
divides by that coordinate (M/MultiH.cpp:793, :799) and nothing downstream is defined.

scene(n, seed) -> src, dst, aff, gt.  Three planes H_k = [e2]x F + e2 v_k^T (every homography compatible with F has this
form), v_k fixed by three correspondences that move a point of the region by at most a tenth of its size along its
epipolar line; a v_k whose denominator changes sign over the region (or comes within a fifth of its largest corner value
of zero) is rejected and drawn again.  dst = H(src) + N(0, noise); affinities are the Jacobian of H_k at src times
1 +- 1 %; 15 % of the rows are gross outliers (uniform dst, affinity I + N(0, 0.2)), gt = -1 there.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

K = np.array([[1000.0, 0.0, 500.0], [0.0, 1000.0, 500.0], [0.0, 0.0, 1.0]])
OUTLIERS = 0.15
PLANES = 3


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


R = rot(0.03, -0.08, 0.02)                                    # synth.make_scene's pair


def cross(e):
    return np.array([[0.0, -e[2], e[1]], [e[2], 0.0, -e[0]], [-e[1], e[0], 0.0]])


def apply_h(H, pts):
    p = np.concatenate([pts, np.ones((pts.shape[0], 1))], axis=1) @ np.asarray(H).reshape(3, 3).T
    return p[:, :2] / p[:, 2:3]


def jacobian_h(H, pts):
    h = np.asarray(H).reshape(9)
    x, y = pts[:, 0], pts[:, 1]
    s = h[6] * x + h[7] * y + h[8]
    u = (h[0] * x + h[1] * y + h[2]) / s
    v = (h[3] * x + h[4] * y + h[5]) / s
    return np.stack([(h[0] - h[6] * u) / s, (h[1] - h[7] * u) / s, (h[3] - h[6] * v) / s, (h[4] - h[7] * v) / s], axis=1)


@dataclass(frozen=True)
class Case:
    name: str
    F: np.ndarray          # (9,) row-major, unit Frobenius norm
    e1: np.ndarray         # (2,) exact, third coordinate 1
    e2: np.ndarray         # (2,)
    lo: float              # the points live in [lo, hi]^2
    hi: float
    noise: float
    near_epipole_rows: int = 0

    def _plane(self, rng):
        """One H = [e2]x F + e2 v^T whose denominator keeps its sign over the region."""
        F = self.F.reshape(3, 3)
        e2h = np.array([self.e2[0], self.e2[1], 1.0])
        M = cross(e2h) @ F
        size = self.hi - self.lo
        corners = np.array([[self.lo, self.lo, 1.0], [self.lo, self.hi, 1.0], [self.hi, self.lo, 1.0], [self.hi, self.hi, 1.0]])
        for _ in range(1000):
            x = np.concatenate([rng.uniform(self.lo, self.hi, size=(3, 2)), np.ones((3, 1))], axis=1)
            s = np.empty(3)
            for i in range(3):
                # the target: x_i moved by at most size / 10, dropped onto its epipolar line l = F x_i
                l = F @ x[i]
                y = x[i, :2] + rng.uniform(-0.1, 0.1, size=2) * size
                y = y - l[:2] * (l[:2] @ y + l[2]) / (l[:2] @ l[:2])
                # y ~ M x_i + s e2: the third coordinates fix the scale, the larger of the other two fixes s
                m = M @ x[i]
                j = int(np.argmax(np.abs(e2h[:2] - y)))
                s[i] = (y[j] * m[2] - m[j]) / (e2h[j] - y[j])
            v = np.linalg.solve(x, s)
            H = M + np.outer(e2h, v)
            den = corners @ H[2]
            if (den > 0).all() or (den < 0).all():
                if np.abs(den).min() > 0.2 * np.abs(den).max():
                    return (H / H[2, 2]).reshape(9)
        raise RuntimeError(f"{self.name}: no plane found")

    def planes(self, seed):
        rng = np.random.default_rng([seed, 0x9E3779B9])
        return np.stack([self._plane(rng) for _ in range(PLANES)])

    def scene(self, n, seed):
        rng = np.random.default_rng(seed)
        H = self.planes(seed)
        src = rng.uniform(self.lo, self.hi, size=(n, 2))
        gt = rng.integers(0, PLANES, size=n).astype(np.int32)
        k = self.near_epipole_rows if n >= 2 * self.near_epipole_rows else 0
        if k:
            # the last k rows: half with src within 1 px of e1 (their dst then lies next to e2), half with dst within
            # 1 px of e2 (set below, after the noise)
            ang, rad = rng.uniform(0, 2 * np.pi, size=k), rng.uniform(0.05, 1.0, size=k)
            off = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
            src[n - k:n - k // 2] = self.e1 + off[:k - k // 2]
        dst = np.empty_like(src)
        aff = np.empty((n, 4))
        for j in range(PLANES):
            m = gt == j
            dst[m] = apply_h(H[j], src[m])
            aff[m] = jacobian_h(H[j], src[m])
        dst += rng.normal(0.0, self.noise, size=dst.shape)
        aff *= 1.0 + rng.normal(0.0, 0.01, size=aff.shape)
        out = rng.random(n) < OUTLIERS
        if k:
            out[n - k:] = False
        dst[out] = rng.uniform(self.lo, self.hi, size=(int(out.sum()), 2))
        aff[out] = np.array([1.0, 0.0, 0.0, 1.0]) + rng.normal(0.0, 0.2, size=(int(out.sum()), 4))
        gt[out] = -1
        if k:
            dst[n - k // 2:] = self.e2 + off[k - k // 2:]
        return src, dst, aff, gt


def _camera(name, t, sign=1.0, **kw):
    t = np.asarray(t, dtype=np.float64)
    Kinv = np.linalg.inv(K)
    F = Kinv.T @ cross(t) @ R @ Kinv
    F = sign * F / np.linalg.norm(F)
    e2, e1 = K @ t, K @ R.T @ t
    return Case(name, F.reshape(9).copy(), e1[:2] / e1[2], e2[:2] / e2[2], 0.0, 1000.0, 0.5, **kw)


def _constructed(name, e1, e2, half, noise, seed):
    e1h, e2h = np.array([e1[0], e1[1], 1.0]), np.array([e2[0], e2[1], 1.0])
    A = np.random.default_rng(seed).normal(size=(3, 3))
    F = cross(e2h) @ A @ (np.eye(3) - np.outer(e1h, e1h) / (e1h @ e1h))
    F = F / np.linalg.norm(F)
    return Case(name, F.reshape(9).copy(), e1h[:2].copy(), e2h[:2].copy(), -half, half, noise)


CASES = {c.name: c for c in (
    _camera("far_right", (0.40, 0.05, 0.08)),
    _camera("in_image", (0.02, -0.03, 1.0), near_epipole_rows=8),
    _constructed("unit", (0.6, 0.8), (-0.8, 0.6), 300.0, 0.5, 101),
    _constructed("near_origin", (3.0, -2.0), (-1.0, 4.0), 20.0, 0.05, 102),
    _camera("far_left", (-0.40, -0.05, 0.08), sign=-1.0),
    _camera("nearly_sideways", (1.0, 0.1, 0.001)),
)}
NAMES = tuple(CASES)

# The seed of every scene the two front-half test files build: the reference alone leaves at most 0.5 % of the rows of
# any case undecidable with it (asserted in test_front_half_cpu.py).
SEED = 7
