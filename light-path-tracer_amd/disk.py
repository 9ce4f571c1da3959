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

lt_trace_disk_hits stores the light-travel time of every hit as well (step_time restates the rule it integrates with), so
that a moving source -- HotSpot, a bright spot on a circular orbit -- can be re-shaded at any observer time from one
trace (shade_hotspot) and reduced to a light curve (lightcurve).
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


# ---- hit times and the orbiting hot spot (lt_trace_disk_hits, lt_shade_hotspot, lt_hotspot_lightcurve) -------------
@dataclass
class HotSpot:
    """A bright spot of Gaussian profile (width sigma) on the circular equatorial orbit at r_spot, at azimuth phi0 at
    coordinate time 0.  with_disk: add the stationary disk's light as the thin-disk renderer does."""
    r_spot: float = 8.0
    phi0: float = 0.0
    sigma: float = 1.0
    exposure: float = 1.0
    with_disk: bool = True

    def to_lt(self):
        """The lt_hotspot struct of this spot (ltrace.HotSpot)."""
        import ltrace
        return ltrace.default_hotspot(r_spot=float(self.r_spot), phi0=float(self.phi0), sigma=float(self.sigma),
                                      exposure=float(self.exposure), with_disk=int(bool(self.with_disk)))


def time_rates(M, a, L, r, th, pr, pth):
    """dt/dlambda, dr/dlambda, dtheta/dlambda of a null geodesic with E = 1, p_phi = L (include/ltrace.h, "Time")."""
    r, th = np.asarray(r, dtype=np.float64), np.asarray(th, dtype=np.float64)
    s2 = np.sin(th) ** 2
    ra = r * r + a * a
    sigma = ra - a * a * s2
    delta = ra - 2.0 * M * r
    p = ra - a * L
    return (ra * p / delta + a * (L - a * s2)) / sigma, delta * np.asarray(pr) / sigma, np.asarray(pth) / sigma


def _hermite(y0, hd0, y1, hd1, t):
    t2, t3 = t * t, t * t * t
    return y0 + (3.0 * t2 - 2.0 * t3) * (y1 - y0) + (t3 - 2.0 * t2 + t) * hd0 + (t3 - t2) * hd1


def step_time(M, a, L, y0, y1, h, tau=1.0):
    """Elapsed coordinate time on [0, tau] of the step y0 -> y1 of length h, the device's rule in float64: Simpson on the
    step's cubic Hermite in (r, theta), tau h / 6 (t'(0) + 4 t'(tau / 2) + t'(tau)).  y0, y1: (..., 4) (r, theta, p_r,
    p_theta); L, h, tau broadcast against the leading axes.  tau = 1: the whole step."""
    y0, y1 = np.asarray(y0, dtype=np.float64), np.asarray(y1, dtype=np.float64)
    h, tau, L = (np.asarray(x, dtype=np.float64) for x in (h, tau, L))
    t0, r0d, th0d = time_rates(M, a, L, y0[..., 0], y0[..., 1], y0[..., 2], y0[..., 3])
    _, r1d, th1d = time_rates(M, a, L, y1[..., 0], y1[..., 1], y1[..., 2], y1[..., 3])

    def rate_at(t):
        r = _hermite(y0[..., 0], h * r0d, y1[..., 0], h * r1d, t)
        th = _hermite(y0[..., 1], h * th0d, y1[..., 1], h * th1d, t)
        return time_rates(M, a, L, r, th, 0.0, 0.0)[0]

    with np.errstate(invalid="ignore", divide="ignore"):
        out = tau * h / 6.0 * (t0 + 4.0 * rate_at(0.5 * tau) + rate_at(tau))
    return np.where(h == 0.0, 0.0, out)


def _stored(hits, n_hits):
    hits = np.asarray(hits)
    m = hits.shape[-2]
    if n_hits is None:
        ok = ~np.isnan(hits[..., 0])
        return np.cumprod(ok, axis=-1).sum(axis=-1)
    return np.minimum(np.asarray(n_hits).astype(np.int64), m)


def spot_emission(M, a, hits, spot, t_obs):
    """E_spot (..., max_images, 3) float64 of every slot of `hits` (..., max_images, 4) float32 (r, phi, g, dt), unclamped:
    exposure g^4 exp(-d^2 / 2 sigma^2) ramp(g), d the distance in the plane to the spot at t_obs - dt."""
    h = np.asarray(hits).astype(np.float64)
    r, ph, g, dt = h[..., 0], h[..., 1], h[..., 2], h[..., 3]
    phi_s = spot.phi0 + omega(M, a, spot.r_spot) * (t_obs - dt)
    d2 = r * r + spot.r_spot * spot.r_spot - 2.0 * r * spot.r_spot * np.cos(ph - phi_s)
    inten = spot.exposure * (g * g) ** 2 * np.exp(-d2 * (1.0 / (2.0 * spot.sigma * spot.sigma)))
    return np.stack([inten * np.clip(2.0 * g - 0.5 * i, 0.0, 1.0) for i in range(3)], axis=-1)


def shade_hotspot(M, a, hits, n_hits, disk, spot, t_obs, base=None, channels=3):
    """lt_shade_hotspot restated: float32 (..., 3), or (...) for channels = 1.  hits (..., max_images, 4) float32, n_hits
    (...) or None, disk a ThinDisk (its inner edge resolved for M, a), spot a HotSpot.  rgb = clamp(base + sum_j
    (with_disk E_j^disk + E_j^spot), 0, 1) in float64, base first, then the slots in order, disk before spot; a pixel
    without a stored hit keeps base."""
    hits = np.asarray(hits)
    m = hits.shape[-2]
    ns = _stored(hits, n_hits)
    r_in = disk.inner_edge(M, a)
    shape = hits.shape[:-2] if channels == 1 else hits.shape[:-2] + (3,)
    base = np.zeros(shape, dtype=np.float32) if base is None else np.asarray(base, dtype=np.float32)
    acc = base.astype(np.float64)
    es = spot_emission(M, a, hits, spot, t_obs)
    for j in range(m):
        on = ns > j
        terms = []
        if spot.with_disk:
            r = np.where(on, hits[..., j, 0].astype(np.float64), 1.0)
            g = np.where(on, hits[..., j, 2].astype(np.float64), 0.0)
            x = r_in / r
            inten = disk.exposure * (g * g) ** 2 * x ** disk.q
            s = g * x ** 0.75
            terms.append(np.stack([inten * np.clip(2.0 * s - 0.5 * i, 0.0, 1.0) for i in range(3)], axis=-1))
        terms.append(np.where(on[..., None], es[..., j, :], 0.0))
        for e in terms:
            if channels == 1:
                acc = np.where(on, acc + (e[..., 0] + e[..., 1] + e[..., 2]) / 3.0, acc)
            else:
                acc = np.where(on[..., None], acc + e, acc)
    lit = ns > 0 if channels == 1 else (ns > 0)[..., None]
    return np.where(lit, np.clip(acc, 0.0, 1.0).astype(np.float32), base)


def lightcurve(M, a, hits, n_hits, spot, times):
    """lt_hotspot_lightcurve restated: (len(times), 3) float64, per time the sums of e, e ix, e iy over the pixels of
    hits (R, W, max_images, 4) and their stored slots, e the mean of E_spot's three channels."""
    hits = np.asarray(hits)
    R, W, m = hits.shape[:3]
    on = _stored(hits, n_hits)[..., None] > np.arange(m)
    iy, ix = np.mgrid[0:R, 0:W].astype(np.float64)
    out = np.empty((len(times), 3))
    for i, t in enumerate(times):
        es = spot_emission(M, a, hits, spot, float(t))
        e = np.where(on, (es[..., 0] + es[..., 1] + es[..., 2]) / 3.0, 0.0).sum(axis=-1)
        out[i] = e.sum(), (e * ix).sum(), (e * iy).sum()
    return out
