"""Thin Keplerian accretion disk: parameters and the float64 numpy statement of its physics.

The GPU path is lt_render_disk / lt_trace_batch_kerr_disk (include/ltrace.h states the convention); the functions here
restate its closed forms in numpy, so that the tests can check the kernels against them and callers can post-process
the (r_hit, phi_hit, g) the renderer returns.

    Omega = sqrt(M) / (r^1.5 + a sqrt(M))                                      (orbit in +phi, signed a)
    u^t   = (r^1.5 + a sqrt(M)) / (r^0.75 sqrt(r^1.5 - 3 M r^0.5 + 2 a sqrt(M)))
    g     = 1 / (u^t (1 - Omega xi))                                           (E = 1, xi = p_phi of the camera's ray)
    I     = exposure g^4 (r_in / r)^q,  s = g (r_in / r)^0.75,  rgb = clamp(I ramp(s), 0, 1)

The optically thin disk (TransparentDisk; lt_render_disk_images) keeps every crossing of the annulus and adds the light
of the first max_images of them to the pixel: rgb = clamp(base + sum_j I_j ramp(s_j), 0, 1) (shade_images).
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np


@dataclass
class ThinDisk:
    """Geometrically thin, optically thick disk in the equatorial plane, r_in <= r <= r_out.
    r_in None: the ISCO of the orbit direction (+phi).  q: emissivity index; exposure: brightness scale."""
    r_in: Optional[float] = None
    r_out: float = 20.0
    q: float = 3.0
    exposure: float = 1.0

    def to_lt(self):
        """The lt_disk struct of this disk (ltrace.Disk)."""
        import ltrace
        return ltrace.default_disk(r_in=0.0 if self.r_in is None else float(self.r_in), r_out=float(self.r_out),
                                   q=float(self.q), exposure=float(self.exposure))

    def inner_edge(self, M, a):
        return isco(M, a) if self.r_in is None or self.r_in <= 0 else float(self.r_in)


@dataclass
class TransparentDisk(ThinDisk):
    """The same disk, optically thin: it emits and does not absorb, so a ray records every crossing of the annulus and
    goes on (lt_render_disk_images).  The picture then shows the higher-order images -- the photon ring -- as well as
    the direct one.  max_images: how many hits per ray are kept (1 ... 8)."""
    max_images: int = 3


def isco(M, a):
    """Bardeen-Press-Teukolsky ISCO of the circular equatorial orbit in +phi (prograde for a > 0, retrograde for a < 0)."""
    M = np.asarray(M, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    x = np.abs(a) / M
    z1 = 1.0 + np.cbrt(1.0 - x * x) * (np.cbrt(1.0 + x) + np.cbrt(1.0 - x))
    z2 = np.sqrt(3.0 * x * x + z1 * z1)
    sgn = np.where(a < 0.0, -1.0, 1.0)
    return M * (3.0 + z2 - sgn * np.sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2)))


def omega(M, a, r):
    """Angular velocity d phi / dt of the circular equatorial geodesic at r."""
    r = np.asarray(r, dtype=np.float64)
    sM = np.sqrt(M)
    return sM / (r * np.sqrt(r) + a * sM)


def u_t(M, a, r):
    """Time component u^t of the circular equatorial geodesic at r (r outside the photon orbit)."""
    r = np.asarray(r, dtype=np.float64)
    sM, sr = np.sqrt(M), np.sqrt(r)
    r15 = r * sr
    return (r15 + a * sM) / (np.sqrt(r15) * np.sqrt(r15 - 3.0 * M * sr + 2.0 * a * sM))


def redshift(M, a, r, xi):
    """g = nu_obs / nu_em of a photon with E = 1 and p_phi = xi emitted by the disk at r."""
    return 1.0 / (u_t(M, a, r) * (1.0 - omega(M, a, r) * np.asarray(xi, dtype=np.float64)))


def shade(r, g, r_in, q=3.0, exposure=1.0, channels=3):
    """Disk colour of the renderer, float32: (..., 3), or (...) for a 1-channel background (the mean of the three).
    Evaluated in float64 from r and g as given (the renderer uses the float32 values it returns)."""
    r = np.asarray(r, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    x = r_in / r
    intensity = exposure * g ** 4 * x ** q
    s = g * x ** 0.75
    ramp = np.stack([np.clip(2.0 * s - 0.5 * i, 0.0, 1.0) for i in range(3)], axis=-1)
    rgb = np.clip(intensity[..., None] * ramp, 0.0, 1.0)
    if channels == 1:
        return ((rgb[..., 0] + rgb[..., 1] + rgb[..., 2]) / 3.0).astype(np.float32)
    return rgb.astype(np.float32)


def shade_images(base, images, n_hits, r_in, q=3.0, exposure=1.0, channels=3):
    """Colour of the optically thin disk's renderer, float32, restated: base (..., 3) or (...) for a 1-channel background
    (the pixel without the disk; 0 for a render without background), images (..., max_images, 3) (r_hit, phi_hit, g),
    n_hits (...).  Each stored hit j < min(n_hits, max_images) adds E_j = exposure g^4 (r_in / r)^q ramp(s), unclamped
    (1 channel: the mean of the three); rgb = clamp(base + sum_j E_j, 0, 1), summed in float64, base first, then the
    slots in order, then rounded to float32.  A pixel without a stored hit keeps base."""
    images = np.asarray(images)
    m = images.shape[-2]
    ns = np.minimum(np.asarray(n_hits).astype(np.int64), m)
    base = np.asarray(base, dtype=np.float32)
    acc = base.astype(np.float64)
    for j in range(m):
        on = ns > j
        r = np.where(on, images[..., j, 0].astype(np.float64), 1.0)
        g = np.where(on, images[..., j, 2].astype(np.float64), 0.0)
        x = r_in / r
        intensity = exposure * g ** 4 * x ** q
        s = g * x ** 0.75
        e = np.stack([intensity * np.clip(2.0 * s - 0.5 * i, 0.0, 1.0) for i in range(3)], axis=-1)
        if channels == 1:
            acc = np.where(on, acc + (e[..., 0] + e[..., 1] + e[..., 2]) / 3.0, acc)
        else:
            acc = np.where(on[..., None], acc + e, acc)
    lit = ns > 0 if channels == 1 else (ns > 0)[..., None]
    return np.where(lit, np.clip(acc, 0.0, 1.0).astype(np.float32), base)
