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
trace (shade_hotspot) and reduced to a light curve (lightcurve).  DiskMap is the general moving source: an emissivity
table on the disk that turns with it (shade_diskmap, diskmap_lightcurve; spiral_map and spots_map make tables), and
DiskMovie a sequence of such tables that change with time (shade_diskmovie, diskmovie_lightcurve, diskmovie_spectrum,
diskmovie_visibility; flare_movie makes one).

The same records binned by g give the energy-resolved light: Spectrum is the grid, spectrum_bin the bin rule, and
disk_spectrum / hotspot_spectrum / diskmap_spectrum the broadened line and the dynamic spectra (lt_*_spectrum).
The same weights taken with a phase per pixel give what an interferometer measures: Baselines holds the (u, v) points,
visibility_phase is the phase rule, and disk_visibility / hotspot_visibility / diskmap_visibility the complex
visibilities per image order (lt_*_visibility).  disk_visibility_stokes / hotspot_visibility_stokes carry the polarization
records through the same sums (I, Q, U per baseline; lt_*_visibility_stokes), and fractional_polarization divides them.

The thermal continuum gives the disk a temperature: novikov_thorne_flux is the relativistic thin disk's radial flux,
ThermalDisk a tabulated flux profile with its temperature scale, thermal_coeffs the rule that makes a stored hit a
blackbody, and thermal_spectrum / shade_thermal the multi-colour blackbody spectrum and the band images
(lt_disk_thermal_spectrum, lt_shade_thermal).  Atmosphere gives the disk's surface a scattering atmosphere -- limb darkening
and a polarization degree, both tabulated on mu --, atmosphere_weights is the rule that turns a polarization record into the
three Stokes weights, thermal_spectrum_stokes / shade_thermal_stokes carry them through the same sums
(lt_disk_thermal_spectrum_stokes, lt_shade_thermal_stokes), and polarization_degree_angle divides the result.

Reverberation bins the records by delay as well as by g: TransferGrid is the delay grid, transfer_bin its bin rule and
disk_transfer the delay-energy transfer function of a flash above the disk (lt_disk_transfer); Lamppost / lamppost_tables
trace a point source on the spin axis to the two radial tables the rule reads, and impulse_response, reverberation_line
and lag_frequency reduce a transfer function further.
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
    g = np.asarray(hits).astype(np.float64)[..., 2]
    inten = spot_intensity(M, a, hits, spot, t_obs)
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


def shade_hotspot_aa(M, a, hits, n_hits, disk, spot, t_obs, samples, base=None, channels=3):
    """lt_shade_hotspot_aa restated: shade_hotspot of the FINE records (R S, W S, max_images, 4) (base at the fine size),
    resolved by the rule of aa.resolve -> float32 (R, W, 3), or (R, W) for channels = 1."""
    import aa
    return aa.resolve(shade_hotspot(M, a, hits, n_hits, disk, spot, t_obs, base=base, channels=channels), samples)


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


# ---- a rotating emissivity map on the disk (lt_shade_diskmap, lt_shade_diskmap_aa, lt_diskmap_lightcurve) ----------------
TWO_PI = 6.283185307179586


@dataclass
class DiskMap:
    """An emissivity table on the disk at coordinate time 0: texels (n_r, n_phi), texel (i, k) at radius
    r_min + (i + 1/2)(r_max - r_min) / n_r and azimuth (k + 1/2) 2 pi / n_phi, looked up bilinearly (constant beyond the
    first and last radial centres, periodic in azimuth, 0 outside [r_min, r_max]).  rotation "kepler": every radius turns
    at the disk's own Omega(r), so the pattern shears; "rigid": all of it at the pattern speed omega_p.  with_disk: add
    the stationary disk's light as the thin-disk renderer does."""
    texels: np.ndarray
    r_min: float = 6.0
    r_max: float = 20.0
    rotation: str = "kepler"
    omega_p: float = 0.0
    exposure: float = 1.0
    with_disk: bool = True

    def __post_init__(self):
        self.texels = np.ascontiguousarray(self.texels, dtype=np.float32)
        if self.texels.ndim != 2 or self.texels.size == 0:
            raise ValueError("texels must be (n_r, n_phi)")
        if self.rotation not in ("kepler", "rigid"):
            raise ValueError('rotation must be "kepler" or "rigid"')

    def to_lt(self):
        """The lt_diskmap struct of this map (ltrace.DiskMap); the table itself is .texels."""
        import ltrace
        return ltrace.default_diskmap(r_min=float(self.r_min), r_max=float(self.r_max), omega_p=float(self.omega_p),
                                      exposure=float(self.exposure), n_r=self.texels.shape[0], n_phi=self.texels.shape[1],
                                      rotation=self.rotation, with_disk=int(bool(self.with_disk)))


def wrap_2pi(ph):
    """phi wrapped to [0, 2 pi), the device's statement."""
    ph = np.asarray(ph, dtype=np.float64)
    w = ph - TWO_PI * np.floor(ph * (1.0 / TWO_PI))
    return np.where((w >= TWO_PI) | (w < 0.0), 0.0, w)


def sample_map(dmap, r, psi):
    """The table's value m at radius r and unwound azimuth psi in [0, 2 pi), float64 (include/ltrace.h, "a rotating
    emissivity map", steps 3 to 5): bilinear, 0 where r < r_min, r > r_max or r is NaN."""
    T = dmap.texels.astype(np.float64)
    n_r, n_phi = T.shape
    r, psi = np.broadcast_arrays(np.asarray(r, dtype=np.float64), np.asarray(psi, dtype=np.float64))
    inside = (r >= dmap.r_min) & (r <= dmap.r_max)
    rr = np.where(inside, r, dmap.r_min)
    ps = np.where(inside & np.isfinite(psi), psi, 0.0)
    v = np.clip((rr - dmap.r_min) / (dmap.r_max - dmap.r_min) * float(n_r) - 0.5, 0.0, float(n_r - 1))
    i0 = np.minimum(np.floor(v).astype(np.int64), n_r - 1)
    i1 = np.minimum(i0 + 1, n_r - 1)
    f_r = v - i0
    u = ps * (n_phi / TWO_PI) - 0.5
    fl = np.floor(u)
    k0 = np.mod(fl.astype(np.int64), n_phi)
    k1 = np.mod(k0 + 1, n_phi)
    f_p = u - fl
    m = (1.0 - f_r) * ((1.0 - f_p) * T[i0, k0] + f_p * T[i0, k1]) + f_r * ((1.0 - f_p) * T[i1, k0] + f_p * T[i1, k1])
    return np.where(inside, m, 0.0)


def map_emission(M, a, hits, dmap, t_obs):
    """E_map (..., max_images, 3) float64 of every slot of `hits` (..., max_images, 4) float32 (r, phi, g, dt), unclamped:
    exposure g^4 m ramp(g), m the table at the hit's radius and at psi = wrap_2pi(phi - Omega (t_obs - dt)), Omega the
    disk's own rate at the hit's r ("kepler") or omega_p ("rigid")."""
    g = np.asarray(hits).astype(np.float64)[..., 2]
    inten = map_intensity(M, a, hits, dmap, t_obs)
    return np.stack([inten * np.clip(2.0 * g - 0.5 * i, 0.0, 1.0) for i in range(3)], axis=-1)


def _shade_table(M, a, hits, n_hits, disk, with_disk, es, base, channels):
    """The frame of a table's light es (..., max_images, 3) (map_emission, movie_emission): rgb = clamp(base + sum_j
    (with_disk E_j^disk + es_j), 0, 1) in float64, base first, then the slots in order, disk before table; a pixel
    without a stored hit keeps base."""
    hits = np.asarray(hits)
    m = hits.shape[-2]
    ns = _stored(hits, n_hits)
    r_in = disk.inner_edge(M, a)
    shape = hits.shape[:-2] if channels == 1 else hits.shape[:-2] + (3,)
    base = np.zeros(shape, dtype=np.float32) if base is None else np.asarray(base, dtype=np.float32)
    acc = base.astype(np.float64)
    for j in range(m):
        on = ns > j
        terms = []
        if with_disk:
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


def shade_diskmap(M, a, hits, n_hits, disk, dmap, t_obs, base=None, channels=3):
    """lt_shade_diskmap restated: float32 (..., 3), or (...) for channels = 1.  shade_hotspot with the map's light in the
    spot's place: rgb = clamp(base + sum_j (with_disk E_j^disk + E_j^map), 0, 1) in float64, base first, then the slots
    in order, disk before map; a pixel without a stored hit keeps base."""
    return _shade_table(M, a, hits, n_hits, disk, dmap.with_disk, map_emission(M, a, hits, dmap, t_obs), base, channels)


def shade_diskmap_aa(M, a, hits, n_hits, disk, dmap, t_obs, samples, base=None, channels=3):
    """lt_shade_diskmap_aa restated: shade_diskmap of the FINE records (R S, W S, max_images, 4) (base at the fine size),
    resolved by the rule of aa.resolve -> float32 (R, W, 3), or (R, W) for channels = 1."""
    import aa
    return aa.resolve(shade_diskmap(M, a, hits, n_hits, disk, dmap, t_obs, base=base, channels=channels), samples)


def diskmap_lightcurve(M, a, hits, n_hits, dmap, times):
    """lt_diskmap_lightcurve restated: (len(times), 3) float64, per time the sums of e, e ix, e iy over the pixels of
    hits (R, W, max_images, 4) and their stored slots, e the mean of E_map's three channels."""
    hits = np.asarray(hits)
    R, W, m = hits.shape[:3]
    on = _stored(hits, n_hits)[..., None] > np.arange(m)
    iy, ix = np.mgrid[0:R, 0:W].astype(np.float64)
    out = np.empty((len(times), 3))
    for i, t in enumerate(times):
        es = map_emission(M, a, hits, dmap, float(t))
        e = np.where(on, (es[..., 0] + es[..., 1] + es[..., 2]) / 3.0, 0.0).sum(axis=-1)
        out[i] = e.sum(), (e * ix).sum(), (e * iy).sum()
    return out


def _texel_centres(n_r, n_phi, r_min, r_max):
    r = r_min + (np.arange(n_r) + 0.5) * (r_max - r_min) / n_r
    ph = (np.arange(n_phi) + 0.5) * TWO_PI / n_phi
    return r[:, None], ph[None, :]


def spiral_map(n_r, n_phi, arms=2, pitch=0.35, contrast=0.8, r_min=6.0, r_max=20.0):
    """Texels (n_r, n_phi) float32 of `arms` logarithmic spiral arms of pitch angle `pitch` (rad) on [r_min, r_max]:
    1 + contrast cos(arms (phi - ln(r / r_min) / tan(pitch))) at the texel centres, 0 <= contrast <= 1."""
    if not 0.0 <= contrast <= 1.0:
        raise ValueError("spiral_map: contrast must be in [0, 1]")
    r, ph = _texel_centres(n_r, n_phi, r_min, r_max)
    return (1.0 + contrast * np.cos(arms * (ph - np.log(r / r_min) / np.tan(pitch)))).astype(np.float32)


def spots_map(n_r, n_phi, r_min, r_max, spots):
    """Texels (n_r, n_phi) float32 of a sum of Gaussians on [r_min, r_max]: spots is a sequence of (r_s, phi_s, sigma) or
    (r_s, phi_s, sigma, amplitude); each adds amplitude exp(-d^2 / 2 sigma^2), d the distance in the plane to the texel
    centre -- the hot spot's profile at t = 0."""
    r, ph = _texel_centres(n_r, n_phi, r_min, r_max)
    out = np.zeros((n_r, n_phi))
    for sp in spots:
        r_s, phi_s, sigma = (float(x) for x in sp[:3])
        amp = float(sp[3]) if len(sp) > 3 else 1.0
        out += amp * np.exp(-(r * r + r_s * r_s - 2.0 * r * r_s * np.cos(ph - phi_s)) / (2.0 * sigma * sigma))
    return out.astype(np.float32)


# ---- energy-resolved light (lt_disk_spectrum, lt_hotspot_spectrum, lt_diskmap_spectrum) -----------------------------------
SPECTRUM_MAX_BINS = 512


@dataclass
class Spectrum:
    """A linear grid in g = E_obs / E_rest (include/ltrace.h, "energy-resolved light"): n_bins half-open bins on
    [g_min, g_max), an underflow column before them and an overflow column after.  split_orders: one plane per stored
    slot (image order) instead of one for all."""
    g_min: float = 0.0625
    g_max: float = 1.5625
    n_bins: int = 96
    split_orders: bool = False

    def __post_init__(self):
        if not (0.0 < self.g_min < self.g_max and np.isfinite(self.g_max)):
            raise ValueError("Spectrum needs 0 < g_min < g_max, both finite")
        if int(self.n_bins) != self.n_bins or not 1 <= self.n_bins <= SPECTRUM_MAX_BINS:
            raise ValueError(f"Spectrum n_bins must be 1 ... {SPECTRUM_MAX_BINS}")
        self.g_min, self.g_max, self.n_bins, self.split_orders = float(self.g_min), float(self.g_max), int(self.n_bins), bool(self.split_orders)

    def to_lt(self):
        """The lt_spectrum struct of this grid (ltrace.Spectrum)."""
        import ltrace
        return ltrace.default_spectrum(g_min=self.g_min, g_max=self.g_max, n_bins=self.n_bins, split_orders=int(self.split_orders))

    def planes(self, max_images):
        return int(max_images) if self.split_orders else 1

    def edges(self):
        """The n_bins + 1 edges of the bins proper, g_min ... g_max (columns 1 ... n_bins of a spectrum)."""
        e = self.g_min + (self.g_max - self.g_min) * np.arange(self.n_bins + 1) / self.n_bins
        e[-1] = self.g_max
        return e

    def energies(self, E_rest):
        """The bins' central photon energies for a line at E_rest, (n_bins,)."""
        e = self.edges()
        return 0.5 * (e[:-1] + e[1:]) * float(E_rest)


def _linear_bin(x, lo, hi, n):
    """The bin rule of both grids, vectorised over float64 x: n half-open bins on [lo, hi) -> int64 column; 0 the
    underflow, n + 1 the overflow, -1 for a NaN.  An infinity or a NaN is replaced before the floor."""
    inv_d = n / (hi - lo)
    nan = np.isnan(x)
    with np.errstate(invalid="ignore", over="ignore"):
        inner = np.floor((np.where(nan | np.isinf(x), lo, x) - lo) * inv_d)
    k = 1 + np.minimum(np.clip(inner, 0, n).astype(np.int64), n - 1)
    k = np.where(x < lo, 0, np.where(x >= hi, n + 1, k))
    return np.where(nan, -1, k)


def spectrum_bin(g, spec):
    """The header's bin rule, vectorised: the column (int64) of every g, float32 as stored, evaluated in float64;
    0 the underflow, n_bins + 1 the overflow, -1 for a NaN (skipped)."""
    return _linear_bin(np.asarray(g, dtype=np.float32).astype(np.float64), spec.g_min, spec.g_max, spec.n_bins)


def _keyed_sum(on, plane_slots, k_row, rows, k_col, cols, weights):
    """(planes, rows, cols) float64: the weights of the slots `on` (..., max_images) added to the key (plane . rows + row)
    . cols + column; plane_slots: one plane per slot (image order) instead of one for all.  The order is numpy's."""
    m = on.shape[-1]
    planes = m if plane_slots else 1
    plane = np.broadcast_to(np.arange(m), on.shape) if plane_slots else np.zeros(on.shape, dtype=np.int64)
    key = ((plane * rows + k_row) * cols + k_col)[on]
    return np.bincount(key, weights=np.asarray(weights, dtype=np.float64)[on], minlength=planes * rows * cols).reshape(planes, rows, cols)


def _bin_weights(hits, n_hits, spec, weights):
    """One row (planes, n_bins + 2) float64: weights (R, W, max_images) of the stored slots of hits binned by their g."""
    hits = np.asarray(hits)
    k = spectrum_bin(hits[..., 2], spec)
    on = (_stored(hits, n_hits)[..., None] > np.arange(hits.shape[-2])) & (k >= 0)
    return _keyed_sum(on, spec.split_orders, 0, 1, k, spec.n_bins + 2, weights)[:, 0]


def spot_intensity(M, a, hits, spot, t_obs):
    """exposure g^4 exp(-d^2 / 2 sigma^2) of every slot, (..., max_images) float64: spot_emission without the ramp."""
    h = np.asarray(hits).astype(np.float64)
    r, ph, g, dt = h[..., 0], h[..., 1], h[..., 2], h[..., 3]
    phi_s = spot.phi0 + omega(M, a, spot.r_spot) * (t_obs - dt)
    d2 = r * r + spot.r_spot * spot.r_spot - 2.0 * r * spot.r_spot * np.cos(ph - phi_s)
    return spot.exposure * (g * g) ** 2 * np.exp(-d2 * (1.0 / (2.0 * spot.sigma * spot.sigma)))


def map_intensity(M, a, hits, dmap, t_obs):
    """exposure g^4 m of every slot, (..., max_images) float64: map_emission without the ramp."""
    h = np.asarray(hits).astype(np.float64)
    r, ph, g, dt = h[..., 0], h[..., 1], h[..., 2], h[..., 3]
    with np.errstate(invalid="ignore"):
        om = dmap.omega_p if dmap.rotation == "rigid" else omega(M, a, r)
        m = sample_map(dmap, r, wrap_2pi(ph - om * (t_obs - dt)))
    return dmap.exposure * (g * g) ** 2 * m


def disk_spectrum(M, a, hits, n_hits, disk, spec):
    """lt_disk_spectrum restated: the stationary disk's line profile, (planes, n_bins + 2) float64 -- per stored slot
    disk.exposure g^4 (r_in / r)^q added to the column of its g (spectrum_bin); column 0 the underflow, the last the
    overflow; plane j the image order j with spec.split_orders."""
    h = np.asarray(hits).astype(np.float64)
    with np.errstate(invalid="ignore"):
        w = disk.exposure * (h[..., 2] * h[..., 2]) ** 2 * (disk.inner_edge(M, a) / h[..., 0]) ** disk.q
    return _bin_weights(hits, n_hits, spec, w)


def hotspot_spectrum(M, a, hits, n_hits, spot, spec, times):
    """lt_hotspot_spectrum restated: the spot's dynamic spectrum, (len(times), planes, n_bins + 2) float64; every image
    order is binned at its own emission time t - dt."""
    with np.errstate(invalid="ignore"):
        return np.stack([_bin_weights(hits, n_hits, spec, spot_intensity(M, a, hits, spot, float(t))) for t in times])


def diskmap_spectrum(M, a, hits, n_hits, dmap, spec, times):
    """lt_diskmap_spectrum restated: the map's dynamic spectrum, (len(times), planes, n_bins + 2) float64."""
    return np.stack([_bin_weights(hits, n_hits, spec, map_intensity(M, a, hits, dmap, float(t))) for t in times])


# ---- visibilities (lt_disk_visibility, lt_hotspot_visibility, lt_diskmap_visibility) -----------------------------------------
VISIBILITY_MAX_BASELINES = 1024


def sincospi_reduced(x):
    """(sin 2 pi x, cos 2 pi x) by the header's rule, float64: f = x - rint(x) (exact), then sincospi(2 f) -- the argument
    split into the nearest quarter turn k / 2 and a rest |r| <= 1/4 (exact), sin and cos of pi r, and the quarter turns
    applied by swapping and negating.  So whole and quarter cycles give exactly 0, 1 and -1."""
    x = np.asarray(x, dtype=np.float64)
    y = 2.0 * (x - np.rint(x))
    k = np.rint(2.0 * y)
    r = y - 0.5 * k
    s0, c0 = np.sin(np.pi * r), np.cos(np.pi * r)
    q = np.mod(k.astype(np.int64), 4)
    s = np.choose(q, [s0, c0, -s0, -c0])
    c = np.choose(q, [c0, -s0, -c0, s0])
    return s, c


def visibility_phase(uv, ix, iy):
    """exp(-2 pi i (u ix + v iy)) by the header's rule -> complex128 (n_baselines,) + ix.shape: x = u ix + v iy with both
    products rounded and then the sum, reduced by sincospi_reduced; the term of a weight w is w times this."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    ix, iy = np.broadcast_arrays(np.asarray(ix, dtype=np.float64), np.asarray(iy, dtype=np.float64))
    shape = (-1,) + (1,) * ix.ndim
    s, c = sincospi_reduced(uv[:, 0].reshape(shape) * ix + uv[:, 1].reshape(shape) * iy)
    return c - 1j * s


@dataclass
class Baselines:
    """The (u, v) points of an interferometer (include/ltrace.h, "visibilities"): uv (n, 2) float64 in cycles per pixel,
    |u|, |v| <= 0.5 (the Nyquist limit), 1 <= n <= 1024.  split_orders: one plane per stored slot (image order) instead of
    one for all.  The entry points take them per pixel of the record buffer; image_lens.render_sequence takes them per
    output pixel and refers the phase to the frame's centre (recentre)."""
    uv: np.ndarray
    split_orders: bool = False

    def __post_init__(self):
        uv = np.array(self.uv, dtype=np.float64)
        if uv.ndim != 2 or uv.shape[1] != 2:
            raise ValueError("Baselines: uv must be (n, 2)")
        if not 1 <= uv.shape[0] <= VISIBILITY_MAX_BASELINES:
            raise ValueError(f"Baselines: 1 ... {VISIBILITY_MAX_BASELINES} baselines")
        if not np.all(np.isfinite(uv)) or not np.all(np.abs(uv) <= 0.5):
            raise ValueError("Baselines: |u|, |v| <= 0.5 cycles per pixel, both finite")
        self.uv, self.split_orders = np.ascontiguousarray(uv), bool(self.split_orders)

    @classmethod
    def radial(cls, n, u_max, angle_deg, split_orders=False):
        """n baselines of lengths 0 ... u_max along the direction angle_deg (from +u towards +v)."""
        rho = float(u_max) * (np.arange(int(n)) / max(int(n) - 1, 1))
        th = np.radians(float(angle_deg))
        return cls(np.stack([rho * np.cos(th), rho * np.sin(th)], axis=-1), split_orders)

    @classmethod
    def grid(cls, n_u, n_v, u_max, split_orders=False):
        """n_u x n_v baselines on a regular grid over [-u_max, u_max]^2, v outer and u inner."""
        u, v = np.linspace(-float(u_max), float(u_max), int(n_u)), np.linspace(-float(u_max), float(u_max), int(n_v))
        vv, uu = np.meshgrid(v, u, indexing="ij")
        return cls(np.stack([uu.ravel(), vv.ravel()], axis=-1), split_orders)

    def __len__(self):
        return self.uv.shape[0]

    def planes(self, max_images):
        return int(max_images) if self.split_orders else 1

    def fine(self, samples=1):
        """The baselines in cycles per pixel of the fine records of `samples`: (u / S, v / S)."""
        return self.uv / np.float64(samples)

    def recentre(self, V, shape, samples=1):
        """V (..., n) as an entry point gives it for the fine records of an (H, W) = shape frame at fine(samples) -> the
        same in output-pixel units, referred to the centre of the output frame: multiplied by
        exp(2 pi i [u (x_c + 1/2 - 1/(2 S)) + v (y_c + 1/2 - 1/(2 S))]), x_c = (W - 1) / 2, y_c = (H - 1) / 2, u and v in
        cycles per output pixel (the factor by sincospi_reduced), and divided by S^2."""
        H, W = shape
        S = np.float64(samples)
        off = 0.5 - 0.5 / S
        s, c = sincospi_reduced(self.uv[:, 0] * ((W - 1) / 2.0 + off) + self.uv[:, 1] * ((H - 1) / 2.0 + off))
        return np.asarray(V) * (c + 1j * s) / (S * S)


def _visibility(hits, n_hits, uv, split_orders, weights):
    """(planes, n_baselines) complex128: weights (R, W, max_images) of the stored slots of hits whose g is not NaN, each
    plane's added over the pixels with visibility_phase."""
    hits = np.asarray(hits)
    R, W, m = hits.shape[:3]
    on = (_stored(hits, n_hits)[..., None] > np.arange(m)) & ~np.isnan(hits[..., 2])
    w = np.where(on, np.asarray(weights, dtype=np.float64), 0.0)
    w = w if split_orders else w.sum(axis=-1, keepdims=True)
    lit = np.nonzero(np.any(w != 0.0, axis=-1).ravel())[0]                # (a pixel without light adds exactly nothing)
    w = w.reshape(R * W, -1)[lit]
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((w.shape[1], uv.shape[0]), dtype=np.complex128)
    for b in range(0, uv.shape[0], 64):
        out[:, b:b + 64] = (w.T[:, None, :] * visibility_phase(uv[b:b + 64], lit % W, lit // W)[None]).sum(axis=-1)
    return out


def disk_visibility(M, a, hits, n_hits, disk, uv, split_orders=False):
    """lt_disk_visibility restated: (planes, n_baselines) complex128, per stored slot disk.exposure g^4 (r_in / r)^q times
    exp(-2 pi i (u ix + v iy)); uv in cycles per pixel of hits."""
    h = np.asarray(hits).astype(np.float64)
    with np.errstate(invalid="ignore"):
        w = disk.exposure * (h[..., 2] * h[..., 2]) ** 2 * (disk.inner_edge(M, a) / h[..., 0]) ** disk.q
    return _visibility(hits, n_hits, uv, split_orders, w)


def hotspot_visibility(M, a, hits, n_hits, spot, uv, split_orders, times):
    """lt_hotspot_visibility restated: (len(times), planes, n_baselines) complex128; every image order at its own
    emission time t - dt."""
    with np.errstate(invalid="ignore"):
        return np.stack([_visibility(hits, n_hits, uv, split_orders, spot_intensity(M, a, hits, spot, float(t))) for t in times])


def diskmap_visibility(M, a, hits, n_hits, dmap, uv, split_orders, times):
    """lt_diskmap_visibility restated: (len(times), planes, n_baselines) complex128."""
    return np.stack([_visibility(hits, n_hits, uv, split_orders, map_intensity(M, a, hits, dmap, float(t))) for t in times])


# ---- a disk movie: tables that change with time (lt_shade_diskmovie, lt_shade_diskmovie_aa, lt_diskmovie_*) ---------------
@dataclass
class DiskMovie:
    """Emissivity tables on the disk at evenly spaced coordinate times (include/ltrace.h, "a disk movie"): texels
    (n_frames, n_r, n_phi), frame q at t0 + q dt_frame, every frame laid out and looked up as a DiskMap's table.  Between
    two frames each is unwound from its own epoch by the rotation ("kepler" / "rigid" with omega_p, as DiskMap) and the two
    are blended linearly in time.  boundary "hold": the first and the last frame are held (and keep turning); "loop": the
    last frame blends into frame 0.  with_disk: add the stationary disk's light."""
    texels: np.ndarray
    t0: float = 0.0
    dt_frame: float = 1.0
    boundary: str = "hold"
    r_min: float = 6.0
    r_max: float = 20.0
    rotation: str = "kepler"
    omega_p: float = 0.0
    exposure: float = 1.0
    with_disk: bool = True

    def __post_init__(self):
        self.texels = np.ascontiguousarray(self.texels, dtype=np.float32)
        if self.texels.ndim != 3 or self.texels.size == 0:
            raise ValueError("texels must be (n_frames, n_r, n_phi)")
        if self.rotation not in ("kepler", "rigid"):
            raise ValueError('rotation must be "kepler" or "rigid"')
        if self.boundary not in ("hold", "loop"):
            raise ValueError('boundary must be "hold" or "loop"')
        if not (np.isfinite(self.t0) and np.isfinite(self.dt_frame) and self.dt_frame > 0.0):
            raise ValueError("t0 and dt_frame must be finite, dt_frame > 0")

    @property
    def n_frames(self):
        return self.texels.shape[0]

    def frame(self, k):
        """Frame k as a DiskMap (the same annulus, rotation and brightness)."""
        return DiskMap(self.texels[k], r_min=self.r_min, r_max=self.r_max, rotation=self.rotation, omega_p=self.omega_p,
                       exposure=self.exposure, with_disk=self.with_disk)

    def to_lt(self):
        """(lt_diskmap, lt_diskmovie) of this movie (ltrace.DiskMap, ltrace.DiskMovie); the tables are .texels."""
        import ltrace
        return self.frame(0).to_lt(), ltrace.default_diskmovie(t0=float(self.t0), dt_frame=float(self.dt_frame), n_frames=self.n_frames,
                                                               boundary=self.boundary)


def movie_pair(movie, t_em):
    """The header's steps 1 to 3: (q0, q1, f_t, k0, k1) of every emission time -- the frame pair as float64 epochs'
    indices, the blend weight, and the table indices (int64, clamped into the movie)."""
    t_em = np.asarray(t_em, dtype=np.float64)
    n = movie.n_frames
    with np.errstate(invalid="ignore"):
        s = (t_em - movie.t0) / movie.dt_frame
        nan = np.isnan(s)
        fl = np.floor(np.where(nan, 0.0, s))
        if movie.boundary == "hold":
            q0 = np.clip(fl, 0.0, float(n - 1))
            q1 = np.minimum(q0 + 1.0, float(n - 1))
            f_t = np.where(nan, 0.0, np.clip(s - q0, 0.0, 1.0))
            k0, k1 = q0, q1
        else:
            q0, q1 = fl, fl + 1.0
            f_t = np.where(nan, 0.0, s - q0)
            k0, k1 = (np.nan_to_num(np.clip(q - n * np.floor(q / n), 0.0, float(n - 1)), nan=0.0) for q in (q0, q1))
    return q0, q1, f_t, k0.astype(np.int64), k1.astype(np.int64)


def sample_movie(movie, r, phi, om, t_em):
    """The movie's value m at radius r and azimuth phi of material turning at rate om, at emission time t_em, float64
    (the header's steps 1 to 5 up to the blend): each frame of the pair looked up by sample_map at the azimuth unwound to
    its own epoch."""
    r, phi, om, t_em = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (r, phi, om, t_em)))
    q0, q1, f_t, k0, k1 = movie_pair(movie, t_em)

    def look(q, k):
        with np.errstate(invalid="ignore"):
            psi = wrap_2pi(phi - om * (t_em - (movie.t0 + q * movie.dt_frame)))
        out = np.zeros(r.shape)
        for f in np.unique(k):
            out = np.where(k == f, sample_map(movie.frame(int(f)), r, psi), out)
        return out

    m0, m1 = look(q0, k0), look(q1, k1)
    with np.errstate(invalid="ignore"):
        blend = (1.0 - f_t) * m0 + f_t * m1
    return np.where(q1 == q0, m0, blend) if movie.boundary == "hold" else blend


def movie_intensity(M, a, hits, movie, t_obs):
    """exposure g^4 m of every slot, (..., max_images) float64: movie_emission without the ramp."""
    h = np.asarray(hits).astype(np.float64)
    r, ph, g, dt = h[..., 0], h[..., 1], h[..., 2], h[..., 3]
    with np.errstate(invalid="ignore"):
        om = np.full(r.shape, movie.omega_p) if movie.rotation == "rigid" else omega(M, a, r)
        m = sample_movie(movie, r, ph, om, t_obs - dt)
    return movie.exposure * (g * g) ** 2 * m


def movie_emission(M, a, hits, movie, t_obs):
    """E (..., max_images, 3) float64 of every slot of `hits`, unclamped: exposure g^4 m ramp(g), m the movie at the slot's
    own emission time t_obs - dt."""
    g = np.asarray(hits).astype(np.float64)[..., 2]
    inten = movie_intensity(M, a, hits, movie, t_obs)
    return np.stack([inten * np.clip(2.0 * g - 0.5 * i, 0.0, 1.0) for i in range(3)], axis=-1)


def shade_diskmovie(M, a, hits, n_hits, disk, movie, t_obs, base=None, channels=3):
    """lt_shade_diskmovie restated: shade_diskmap with the movie's light in the map's place."""
    return _shade_table(M, a, hits, n_hits, disk, movie.with_disk, movie_emission(M, a, hits, movie, t_obs), base, channels)


def shade_diskmovie_aa(M, a, hits, n_hits, disk, movie, t_obs, samples, base=None, channels=3):
    """lt_shade_diskmovie_aa restated: shade_diskmovie of the FINE records, resolved by the rule of aa.resolve."""
    import aa
    return aa.resolve(shade_diskmovie(M, a, hits, n_hits, disk, movie, t_obs, base=base, channels=channels), samples)


def diskmovie_lightcurve(M, a, hits, n_hits, movie, times):
    """lt_diskmovie_lightcurve restated: (len(times), 3) float64, per time the sums of e, e ix, e iy over the pixels of
    hits (R, W, max_images, 4) and their stored slots, e the mean of the movie's three channels."""
    hits = np.asarray(hits)
    R, W, m = hits.shape[:3]
    on = _stored(hits, n_hits)[..., None] > np.arange(m)
    iy, ix = np.mgrid[0:R, 0:W].astype(np.float64)
    out = np.empty((len(times), 3))
    for i, t in enumerate(times):
        es = movie_emission(M, a, hits, movie, float(t))
        e = np.where(on, (es[..., 0] + es[..., 1] + es[..., 2]) / 3.0, 0.0).sum(axis=-1)
        out[i] = e.sum(), (e * ix).sum(), (e * iy).sum()
    return out


def diskmovie_spectrum(M, a, hits, n_hits, movie, spec, times):
    """lt_diskmovie_spectrum restated: the movie's dynamic spectrum, (len(times), planes, n_bins + 2) float64."""
    return np.stack([_bin_weights(hits, n_hits, spec, movie_intensity(M, a, hits, movie, float(t))) for t in times])


def diskmovie_visibility(M, a, hits, n_hits, movie, uv, split_orders, times):
    """lt_diskmovie_visibility restated: (len(times), planes, n_baselines) complex128."""
    return np.stack([_visibility(hits, n_hits, uv, split_orders, movie_intensity(M, a, hits, movie, float(t))) for t in times])


def flare_movie(n_frames, n_r, n_phi, r_min, r_max, r_s, phi_s, sigma, t_peak, t_width, dt_frame, t0=0.0, floor=0.1, amplitude=1.0,
                rotation="kepler", omega_p=0.0, M=1.0, a=0.0, **kw):
    """A DiskMovie of a flare, something a turning table cannot show: on a quiescent floor a Gaussian clump of width
    sigma whose amplitude rises and falls as a Gaussian in time, amplitude exp(-(T - t_peak)^2 / 2 t_width^2).  The clump is
    stated in the co-rotating sense: the material of radius r that carries it stands at azimuth phi_s + Omega (T - t_peak)
    in the frame of epoch T -- Omega the disk's own rate at r ("kepler": round at (r_s, phi_s) at t_peak, sheared before
    and after) or omega_p ("rigid") -- so the advected interpolation between two frames carries it instead of
    cross-fading two copies.  Frame q is at T = t0 + q dt_frame; further keywords (boundary, exposure, with_disk) go to
    DiskMovie."""
    r, ph = _texel_centres(n_r, n_phi, r_min, r_max)
    om = np.full(r.shape, float(omega_p)) if rotation == "rigid" else omega(M, a, r)
    T = float(t0) + float(dt_frame) * np.arange(int(n_frames))[:, None, None]
    d2 = r * r + r_s * r_s - 2.0 * r * r_s * np.cos(ph - (phi_s + om * (T - t_peak)))
    texels = floor + amplitude * np.exp(-(T - t_peak) ** 2 / (2.0 * t_width * t_width)) * np.exp(-d2 / (2.0 * sigma * sigma))
    return DiskMovie(texels.astype(np.float32), t0=float(t0), dt_frame=float(dt_frame), r_min=float(r_min), r_max=float(r_max),
                     rotation=rotation, omega_p=float(omega_p), **kw)


# ---- linear polarization (lt_trace_disk_pol, lt_shade_stokes, lt_hotspot_lightcurve_stokes) ------------------------
@dataclass
class BField:
    """Magnetic field with constant components in the disk material's orthonormal frame (e_r, e_phi, e_z; include/ltrace.h,
    "linear polarization"); only its direction matters.  pol_frac: the polarization fraction Pi in [0, 1]."""
    b_r: float = 0.0
    b_phi: float = 0.0
    b_z: float = 1.0
    pol_frac: float = 0.7

    def to_lt(self):
        """The lt_bfield struct of this field (ltrace.BField)."""
        import ltrace
        return ltrace.default_bfield(b_r=float(self.b_r), b_phi=float(self.b_phi), b_z=float(self.b_z),
                                     pol_frac=float(self.pol_frac))


def _raise_index(M, a, r, s, c, k):
    """Contravariant components of the covector k = (k_t, k_r, k_theta, k_phi) at (r, theta), s = sin theta, c = cos theta."""
    s2 = s * s
    sigma = r * r + a * a * c * c
    delta = r * r - 2 * M * r + a * a
    sd = sigma * delta
    gtt = -((r * r + a * a) ** 2 - a * a * delta * s2) / sd
    gtp = -2 * M * a * r / sd
    gpp = (delta - a * a * s2) / (sd * s2)
    return gtt * k[0] + gtp * k[3], delta / sigma * k[1], k[2] / sigma, gtp * k[0] + gpp * k[3]


def walker_penrose(a, r, s, c, k, f):
    """(Re, Im) of kappa = (A - i B)(r - i a cos theta) from the contravariant components of k and f at (r, theta)."""
    A = (k[0] * f[1] - k[1] * f[0]) + a * s * s * (k[1] * f[3] - k[3] * f[1])
    B = ((r * r + a * a) * (k[3] * f[2] - k[2] * f[3]) - a * (k[0] * f[2] - k[2] * f[0])) * s
    return A * r - B * a * c, -(A * a * c + B * r)


def emitter_frame(M, a, r):
    """Of the circular equatorial geodesic in +phi at r: (sqrt(Delta) / r, e_(phi)^t, e_(phi)^phi) -- e_(r) = (0, sqrt(Delta)
    / r, 0, 0), e_(z) = -d_theta / r, e_(phi) the unit vector of the t-phi plane orthogonal to u with positive phi part."""
    delta = r * r - 2 * M * r + a * a
    g_tt, g_tp, g_pp = -(1 - 2 * M / r), -2 * M * a / r, r * r + a * a + 2 * M * a * a / r
    sM, sr = np.sqrt(M), np.sqrt(r)
    r15 = r * sr
    om = sM / (r15 + a * sM)
    ut = (r15 + a * sM) / (np.sqrt(r15) * np.sqrt(r15 - 3 * M * sr + 2 * a * sM))
    u_t, u_p = ut * (g_tt + g_tp * om), ut * (g_tp + g_pp * om)
    n = np.sqrt(g_tt * u_p * u_p - 2 * g_tp * u_p * u_t + g_pp * u_t * u_t)
    return np.sqrt(delta) / r, u_p / n, -u_t / n


def emission_vector(M, a, L, hit_state, bfield, dtype=np.float64):
    """At a hit (r, p_r, p_theta of the backward ray; theta = pi / 2): the received photon's contravariant k, the electric
    vector f = (k^ x b^) / sin zeta lifted to coordinates, sin^2 zeta and mu = |k^ . e_(z)|."""
    hs = np.asarray(hit_state, dtype=dtype)
    L = np.asarray(L, dtype=dtype)
    M, a = dtype(M), dtype(a)
    r, pr, pth = hs[..., 0], hs[..., 1], hs[..., 2]
    er, ept, epp = emitter_frame(M, a, r)
    kr, kp, kz = -er * pr, epp * L - ept, pth / r      # k = (-1, -p_r, -p_theta, L) on e_(r), e_(phi), e_(z)
    kn = np.sqrt(kr * kr + kp * kp + kz * kz)
    kr, kp, kz = kr / kn, kp / kn, kz / kn
    b = np.array([bfield.b_r, bfield.b_phi, bfield.b_z], dtype=dtype)
    b = b / np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
    cr, cp, cz = kp * b[2] - kz * b[1], kz * b[0] - kr * b[2], kr * b[1] - kp * b[0]
    s2 = cr * cr + cp * cp + cz * cz
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = 1 / np.sqrt(s2)
    fr, fp, fz = cr * inv, cp * inv, cz * inv
    one, zero = np.ones_like(r), np.zeros_like(r)
    k = _raise_index(M, a, r, one, zero, (-one, -pr, -pth, L * one))
    f = (fp * ept, fr * er, -fz / r, fp * epp)
    return k, f, s2, np.abs(kz)


def camera_screen(M, a, r_obs, theta_obs, L, cam_state, dtype=np.float64):
    """At the static observer: the received photon's contravariant k and the screen vectors e_1, e_2 lifted to
    coordinates (north e_2 ~ -e_theta + n^theta n, e_1 = e_2 x n in the right-handed (r, theta, phi) tetrad).  cam_state:
    (p_r, p_theta) of the backward ray at the camera, the ray's own record."""
    cs = np.asarray(cam_state, dtype=dtype)
    L = np.asarray(L, dtype=dtype)
    M, a = dtype(M), dtype(a)
    r, th = np.asarray(r_obs, dtype=dtype), np.asarray(theta_obs, dtype=dtype)
    pr, pth = cs[..., 0], cs[..., 1]
    s, c = np.sin(th), np.cos(th)
    sigma = r * r + a * a * c * c
    delta = r * r - 2 * M * r + a * a
    g_tt = -(1 - 2 * M * r / sigma)
    g_tp = -2 * M * a * r * s * s / sigma
    g_pp = (r * r + a * a + 2 * M * a * a * r * s * s / sigma) * s * s
    w = -g_tp / g_tt
    n_phi = np.sqrt(g_pp - g_tp * g_tp / g_tt)
    e_r, e_th = np.sqrt(delta / sigma), 1 / np.sqrt(sigma)
    n = [-e_r * pr, -e_th * pth, (L - w) / n_phi]
    nn = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    n = [x / nn for x in n]
    e2 = [n[1] * n[0], n[1] * n[1] - 1, n[1] * n[2]]
    en = np.sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2])
    e2 = [x / en for x in e2]
    e1 = [e2[1] * n[2] - e2[2] * n[1], e2[2] * n[0] - e2[0] * n[2], e2[0] * n[1] - e2[1] * n[0]]
    lift = lambda e: (e[2] * w / n_phi, e[0] * e_r, e[1] * e_th, e[2] / n_phi)
    one = np.ones_like(pr)
    k = _raise_index(M, a, r * one, s * one, c * one, (-one, -pr, -pth, L * one))
    return k, lift(e1), lift(e2), (r * one, s * one, c * one)


def polarization(M, a, r_obs, theta_obs, L, hit_state, cam_state, bfield, dtype=np.float64):
    """The polarization record of a hit (include/ltrace.h, "linear polarization") -> (..., 4): q = cos 2 chi, u = sin 2 chi
    at the camera (chi from e_1 towards e_2), sin zeta and mu at the emitter.  hit_state (..., 3): r, p_r, p_theta of the
    backward ray at the hit; cam_state (..., 2): its p_r, p_theta at the camera; L its p_phi.  The Walker-Penrose
    constant of (k, f) at the hit is matched by x kappa(e_1) + y kappa(e_2) at the camera.  sin^2 zeta < 1e-24: q = u =
    sin zeta = 0.  dtype np.longdouble evaluates the same statement in extended precision."""
    M_, a_ = dtype(M), dtype(a)
    k, f, s2, mu = emission_vector(M, a, L, hit_state, bfield, dtype)
    r = np.asarray(hit_state, dtype=dtype)[..., 0]
    kh = walker_penrose(a_, r, np.ones_like(r), np.zeros_like(r), k, f)
    kc, f1, f2, (ro, so, co) = camera_screen(M, a, r_obs, theta_obs, L, cam_state, dtype)
    k1, k2 = walker_penrose(a_, ro, so, co, kc, f1), walker_penrose(a_, ro, so, co, kc, f2)
    with np.errstate(invalid="ignore", divide="ignore"):
        det = k1[0] * k2[1] - k2[0] * k1[1]
        x = (kh[0] * k2[1] - k2[0] * kh[1]) / det
        y = (k1[0] * kh[1] - kh[0] * k1[1]) / det
        n2 = x * x + y * y
        q, u = (x * x - y * y) / n2, 2 * x * y / n2
    dark = s2 < 1e-24
    out = np.stack(np.broadcast_arrays(np.where(dark, 0, q), np.where(dark, 0, u), np.where(dark, 0, np.sqrt(s2)), mu), axis=-1)
    return out.astype(dtype)


def _slot_means(M, a, hits, n_hits, disk, spot, t_obs, with_disk):
    """(on, e): the stored slots (..., max_images) and per slot the mean of the three channels of its light, the disk's
    (with_disk) plus the spot's, unclamped."""
    hits = np.asarray(hits)
    m = hits.shape[-2]
    on = _stored(hits, n_hits)[..., None] > np.arange(m)
    es = spot_emission(M, a, hits, spot, t_obs)
    e = (es[..., 0] + es[..., 1] + es[..., 2]) / 3.0
    if with_disk:
        r = np.where(on, hits[..., 0].astype(np.float64), 1.0)
        g = np.where(on, hits[..., 2].astype(np.float64), 0.0)
        x = disk.inner_edge(M, a) / r
        inten = disk.exposure * (g * g) ** 2 * x ** disk.q
        s = g * x ** 0.75
        ed = [inten * np.clip(2.0 * s - 0.5 * i, 0.0, 1.0) for i in range(3)]
        e = (ed[0] + ed[1] + ed[2]) / 3.0 + e
    return on, np.where(on, e, 0.0)


def _stokes_weights(pol, on, bfield):
    p = np.asarray(pol).astype(np.float64)
    w = np.where(on, bfield.pol_frac * p[..., 2] * p[..., 2], 0.0)
    return np.where(on, w * p[..., 0], 0.0), np.where(on, w * p[..., 1], 0.0)


def stokes_frame(M, a, hits, n_hits, pol, disk, spot, t_obs, bfield):
    """lt_shade_stokes restated: (..., 3) float32 (I, Q, U) at t_obs.  hits (..., max_images, 4) and n_hits as
    shade_hotspot's, pol (..., max_images, 4) float32 (q, u, sin zeta, mu).  Per stored slot, e the mean of the three
    channels of the slot's light (the disk's if spot.with_disk, plus the spot's): I += e, Q += Pi sin^2 zeta e q,
    U += Pi sin^2 zeta e u, in float64, the slots in order; no clamp, no base."""
    on, e = _slot_means(M, a, hits, n_hits, disk, spot, t_obs, spot.with_disk)
    wq, wu = _stokes_weights(pol, on, bfield)
    return np.stack([e.sum(axis=-1), (wq * e).sum(axis=-1), (wu * e).sum(axis=-1)], axis=-1).astype(np.float32)


def stokes_frame_aa(M, a, hits, n_hits, pol, disk, spot, t_obs, bfield, samples):
    """lt_shade_stokes_aa restated: stokes_frame of the FINE records, resolved by the rule of aa.resolve -> (R, W, 3)."""
    import aa
    return aa.resolve(stokes_frame(M, a, hits, n_hits, pol, disk, spot, t_obs, bfield), samples)


def stokes_lightcurve(M, a, hits, n_hits, pol, spot, times, bfield):
    """lt_hotspot_lightcurve_stokes restated: (len(times), 3) float64, per time the sums of I, Q, U of the spot alone over
    the pixels of hits (R, W, max_images, 4) and their stored slots.  Column 0 is lightcurve()'s column 0."""
    hits = np.asarray(hits)
    out = np.empty((len(times), 3))
    for i, t in enumerate(times):
        on, e = _slot_means(M, a, hits, n_hits, None, spot, float(t), False)
        wq, wu = _stokes_weights(pol, on, bfield)
        out[i] = e.sum(axis=-1).sum(), (wq * e).sum(axis=-1).sum(), (wu * e).sum(axis=-1).sum()
    return out


# ---- polarized visibilities (lt_disk_visibility_stokes, lt_hotspot_visibility_stokes) ---------------------------------------
def _visibility_stokes(hits, n_hits, pol, uv, split_orders, w_i, bfield):
    """(planes, 3, n_baselines) complex128: _visibility of w_I, ((Pi sz sz) q) w_I and ((Pi sz sz) u) w_I, the products in
    _stokes_weights' order, over the stored slots whose g is not NaN."""
    hits = np.asarray(hits)
    on = (_stored(hits, n_hits)[..., None] > np.arange(hits.shape[-2])) & ~np.isnan(hits[..., 2])
    wq, wu = _stokes_weights(pol, on, bfield)
    w_i = np.where(on, np.asarray(w_i, dtype=np.float64), 0.0)
    return np.stack([_visibility(hits, n_hits, uv, split_orders, w) for w in (w_i, wq * w_i, wu * w_i)], axis=1)


def disk_visibility_stokes(M, a, hits, n_hits, pol, disk, uv, bfield, split_orders=False):
    """lt_disk_visibility_stokes restated: (planes, 3, n_baselines) complex128, the Stokes axis (I, Q, U); plane I is
    disk_visibility's.  pol (R, W, max_images, 4) float32 (q, u, sin zeta, mu)."""
    h = np.asarray(hits).astype(np.float64)
    with np.errstate(invalid="ignore"):
        w = disk.exposure * (h[..., 2] * h[..., 2]) ** 2 * (disk.inner_edge(M, a) / h[..., 0]) ** disk.q
    return _visibility_stokes(hits, n_hits, pol, uv, split_orders, w, bfield)


def hotspot_visibility_stokes(M, a, hits, n_hits, pol, spot, uv, bfield, split_orders, times):
    """lt_hotspot_visibility_stokes restated: (len(times), planes, 3, n_baselines) complex128; plane I is
    hotspot_visibility's."""
    with np.errstate(invalid="ignore"):
        return np.stack([_visibility_stokes(hits, n_hits, pol, uv, split_orders, spot_intensity(M, a, hits, spot, float(t)), bfield)
                         for t in times])


def fractional_polarization(V):
    """m = (Q~ + i U~) / I~ of polarized visibilities V (..., 3, n_baselines) -> (..., n_baselines) complex128, NaN where
    I~ is 0.  |m| at (0, 0) is the image's net polarization fraction; on a long baseline it may exceed 1."""
    V = np.asarray(V, dtype=np.complex128)
    i, q, u = V[..., 0, :], V[..., 1, :], V[..., 2, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(i == 0, np.nan + 0j, (q + 1j * u) / np.where(i == 0, 1.0, i))


# ---- thermal continuum (lt_disk_thermal_spectrum, lt_shade_thermal) ----------------------------------------------------------
THERMAL_MAX_NODES, THERMAL_MAX_FREQS, THERMAL_MAX_BANDS = 65536, 1024, 16


def _nt_roots(astar):
    """(x1, x2, x3) of Page & Thorne (1974) eq. 15n: the roots of x^3 - 3 x + 2 a*.  x2 = 2 cos((acos a* + pi) / 3) is taken
    as 2 sin(asin(a*) / 3), the same number, which is exactly 0 at a* = 0 and keeps its relative accuracy near it."""
    ac = np.arccos(astar)
    return 2.0 * np.cos((ac - np.pi) / 3.0), 2.0 * np.sin(np.arcsin(astar) / 3.0), -2.0 * np.cos(ac / 3.0)


def novikov_thorne_terms(M, a, r):
    """The terms of the bracket of Page & Thorne (1974) eq. 15n at radii r, stacked on a new first axis (6, ...):
    x, -x0, -(3/2) a* ln(x / x0) and the three root terms -3 (x_i - a*)^2 / (x_i (x_i - x_j)(x_i - x_k)) ln((x - x_i) /
    (x0 - x_i)); x = sqrt(r / M), x0 = sqrt(r_isco / M), a* = a / M.  The x2 term is 0 at a* = 0, its limit.
    novikov_thorne_flux adds them; their absolute sum over the bracket is the flux's condition number (the bracket cancels
    towards the ISCO)."""
    M, a = float(M), float(a)
    astar = a / M
    x = np.sqrt(np.asarray(r, dtype=np.float64) / M)
    x0 = np.sqrt(float(isco(M, a)) / M)
    roots = _nt_roots(astar)
    terms = [x, np.full_like(x, -x0), -1.5 * astar * np.log(x / x0)]
    for i in range(3):
        xi, xj, xk = roots[i], roots[(i + 1) % 3], roots[(i + 2) % 3]
        if xi == 0.0:
            terms.append(np.zeros_like(x))
            continue
        coeff = 3.0 * (xi - astar) ** 2 / (xi * (xi - xj) * (xi - xk))
        terms.append(-coeff * np.log((x - xi) / (x0 - xi)))
    return np.stack(terms)


def novikov_thorne_flux(M, a, r):
    """The Novikov-Thorne flux of a relativistic thin disk around a Kerr hole, Page & Thorne (1974) eq. 15n with an
    accretion rate of 1 (G = c = 1): the energy per unit proper time and proper area a face of the disk radiates at r,
        F = 3 / (8 pi M^2) 1 / (x^4 (x^3 - 3 x + 2 a*)) [bracket],    x = sqrt(r / M),  a* = a / M
    (novikov_thorne_terms has the bracket).  The disk orbits in +phi, so a < 0 is the retrograde disk.  F = 0 for
    r <= r_isco: no torque at the inner edge.  |a| < M."""
    M, a = float(M), float(a)
    r = np.asarray(r, dtype=np.float64)
    r_in = float(isco(M, a))
    inside = r > r_in
    rr = np.where(inside, r, 2.0 * r_in)                                  # (a placeholder outside the ISCO where F is not evaluated)
    x = np.sqrt(rr / M)
    bracket = novikov_thorne_terms(M, a, rr).sum(axis=0)
    F = 3.0 / (8.0 * np.pi * M * M) / (x ** 4 * (x ** 3 - 3.0 * x + 2.0 * a / M)) * bracket
    return np.where(inside, np.maximum(F, 0.0), 0.0)


@dataclass
class ThermalDisk:
    """The thermal emitter (include/ltrace.h, "thermal continuum"): a radial flux table -- flux (n_r,) float64, node i at
    r_min + i (r_max - r_min) / (n_r - 1), linearly interpolated -- and a temperature scale T = t_max flux^(1/4), t_max a
    frequency (k T / h where flux = 1).  f_col: the colour-correction (hardening) factor; exposure: the brightness scale;
    split_orders: one plane per stored slot (image order) in the spectrum."""
    flux: np.ndarray
    r_min: float
    r_max: float
    t_max: float = 1.0
    f_col: float = 1.0
    exposure: float = 1.0
    split_orders: bool = False

    def __post_init__(self):
        flux = np.array(self.flux, dtype=np.float64)
        if flux.ndim != 1 or not 2 <= flux.size <= THERMAL_MAX_NODES:
            raise ValueError(f"ThermalDisk: flux must be (n_r,), n_r 2 ... {THERMAL_MAX_NODES}")
        if not (0.0 < self.r_min < self.r_max and np.isfinite(self.r_max)):
            raise ValueError("ThermalDisk needs 0 < r_min < r_max, both finite")
        if not (self.t_max > 0.0 and np.isfinite(self.t_max) and self.f_col > 0.0 and np.isfinite(self.f_col)):
            raise ValueError("ThermalDisk: t_max and f_col must be positive and finite")
        if not (self.exposure >= 0.0 and np.isfinite(self.exposure)):
            raise ValueError("ThermalDisk: exposure must be finite, >= 0")
        self.flux = np.ascontiguousarray(flux)
        self.r_min, self.r_max, self.t_max, self.f_col = float(self.r_min), float(self.r_max), float(self.t_max), float(self.f_col)
        self.exposure, self.split_orders = float(self.exposure), bool(self.split_orders)

    @property
    def n_r(self):
        return self.flux.size

    def nodes(self):
        """The radii of the table's nodes, (n_r,)."""
        return self.r_min + np.arange(self.n_r) * (self.r_max - self.r_min) / (self.n_r - 1)

    def planes(self, max_images):
        return int(max_images) if self.split_orders else 1

    def to_lt(self):
        """The lt_thermal struct of this emitter (ltrace.Thermal); the table itself is passed beside it."""
        import ltrace
        return ltrace.default_thermal(r_min=self.r_min, r_max=self.r_max, t_max=self.t_max, f_col=self.f_col, exposure=self.exposure,
                                      n_r=self.n_r, split_orders=int(self.split_orders))

    @classmethod
    def novikov_thorne(cls, M, a, r_out, n_r=4096, t_max=1.0, f_col=1.0, exposure=1.0, split_orders=False):
        """The Novikov-Thorne disk from isco(M, a) to r_out on n_r nodes: novikov_thorne_flux divided by its largest node,
        so that t_max is the peak effective temperature (as a frequency).  The first node, the ISCO, is 0."""
        r_in = float(isco(M, a))
        nodes = r_in + np.arange(int(n_r)) * (float(r_out) - r_in) / (int(n_r) - 1)
        flux = novikov_thorne_flux(M, a, nodes)
        flux[0] = 0.0
        return cls(flux / flux.max(), r_in, float(r_out), t_max=t_max, f_col=f_col, exposure=exposure, split_orders=split_orders)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """round(a b + c) with ONE rounding, float64, vectorised: numpy has no fused multiply-add, so this is Boldo and
    Melquiond's emulation -- the exact product and sum as pairs (Dekker, Knuth), the two low parts added with rounding to
    odd, and the high part added last.  Exact unless an intermediate overflows or the product's low part underflows
    (|a b| below 2^-969), which the tables here stay far from."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    v, e = _two_sum(tl, ul)
    even = (np.ascontiguousarray(v).view(np.int64) & 1) == 0
    v = np.where((e != 0.0) & even, np.nextafter(v, np.where(e > 0.0, np.inf, -np.inf)), v)
    return th + v


def thermal_coeffs(hits, n_hits, thermal):
    """The header's steps 1 to 4 for every slot of hits (..., max_images, 4) float32 -> (A, c, emits): A the call's
    amplitude exposure / f_col^4 (a float), c and emits (..., max_images): the slot's light at frequency nu is
    nu^3 A / expm1(nu c) where emits, and nothing elsewhere (c = 0 there).  Every operation is the header's, in its order
    and rounded as there (the interpolation by fma above)."""
    h = np.asarray(hits, dtype=np.float32)
    m = h.shape[-2]
    r, g = h[..., 0].astype(np.float64), h[..., 2].astype(np.float64)
    flux, n_r = thermal.flux, thermal.n_r
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        emits = (_stored(h, n_hits)[..., None] > np.arange(m)) & (g > 0.0) & (r >= thermal.r_min) & (r <= thermal.r_max)
        inv_dr = float(n_r - 1) / (thermal.r_max - thermal.r_min)
        v = (np.where(emits, r, thermal.r_min) - thermal.r_min) * inv_dr
        i0 = np.clip(np.floor(v).astype(np.int64), 0, n_r - 2)
        w = v - i0.astype(np.float64)
        F = fma(w, flux[i0 + 1] - flux[i0], flux[i0])
        emits = emits & (F > 0.0)
        T = thermal.t_max * np.sqrt(np.sqrt(np.where(emits, F, 1.0)))
        c = 1.0 / ((np.where(emits, g, 1.0) * thermal.f_col) * T)
    A = thermal.exposure / ((thermal.f_col * thermal.f_col) * (thermal.f_col * thermal.f_col))
    return A, np.where(emits, c, 0.0), emits


def thermal_term(nu, A, c):
    """Step 5 without its nu^3: A / expm1(nu c), the product rounded to float64 first."""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        return A / np.expm1(nu * c)


def _frequencies(nu, limit):
    nu = np.asarray(nu, dtype=np.float64).ravel()
    if nu.size > limit:
        raise ValueError(f"at most {limit} frequencies")
    return nu


def _thermal_planes(thermal, nu, A, c, emits, w=None):
    """The plane loop of both spectra -> (planes, n_freq), or (planes, 3, n_freq) with the slots' weights w (..., max_images,
    3): per plane and frequency ((nu nu) nu) times the sum of the emitting slots' terms, each times its weight where given."""
    out = np.zeros((thermal.planes(c.shape[-1]),) + (() if w is None else (3,)) + (nu.size,))
    for plane in range(out.shape[0]):
        on = emits[..., plane] if thermal.split_orders else emits
        cp = c[..., plane][on] if thermal.split_orders else c[on]
        wp = None if w is None else w[..., plane, :][on] if thermal.split_orders else w[on]
        for k in range(0, nu.size, 8):
            f = nu[k:k + 8, None]
            t = thermal_term(f, A, cp[None, :])
            if w is None:
                out[plane, k:k + 8] = ((f[:, 0] * f[:, 0]) * f[:, 0]) * t.sum(axis=-1)
            else:
                for x in range(3):
                    out[plane, x, k:k + 8] = ((f[:, 0] * f[:, 0]) * f[:, 0]) * (wp[None, :, x] * t).sum(axis=-1)
    return out


def _thermal_bands(nu, A, c, emits, w=None):
    """The band loop of both band images -> (n_freq, R, W) float32, or (n_freq, 3, R, W) with the slots' weights w: the emitting
    slots' terms added in slot order in float64, S + t, or S = fma(w_X, t, S) where given; times (nu nu) nu; one rounding."""
    out = np.zeros((nu.size,) + (() if w is None else (3,)) + c.shape[:-1], dtype=np.float32)
    for b, f in enumerate(nu):
        total = np.zeros(out.shape[1:])
        for j in range(c.shape[-1]):
            t = np.where(emits[..., j], thermal_term(f, A, np.where(emits[..., j], c[..., j], 1.0)), 0.0)
            if w is None:
                total = total + t
            else:
                for s_ in range(3):
                    total[s_] = np.where(emits[..., j], fma(w[..., j, s_], t, total[s_]), total[s_])
        out[b] = (((f * f) * f) * total).astype(np.float32)
    return out


def thermal_spectrum(hits, n_hits, thermal, nu):
    """lt_disk_thermal_spectrum restated: (planes, n_freq) float64, per plane and frequency ((nu nu) nu) times the sum of
    A / expm1(nu c) over the emitting slots of all pixels (the order of the sum is numpy's, not the kernel's); planes is 1,
    or max_images with thermal.split_orders."""
    nu = _frequencies(nu, THERMAL_MAX_FREQS)
    return _thermal_planes(thermal, nu, *thermal_coeffs(hits, n_hits, thermal))


def shade_thermal(hits, n_hits, thermal, nu):
    """lt_shade_thermal restated: (n_freq, R, W) float32 band images -- per pixel and band the emitting slots' A / expm1(nu c)
    added in slot order in float64, times (nu nu) nu, rounded once to float32.  A pixel without an emitting slot is +0.0."""
    if thermal.split_orders:
        raise ValueError("shade_thermal: a band image has one plane per band; split_orders must be off")
    nu = _frequencies(nu, THERMAL_MAX_BANDS)
    return _thermal_bands(nu, *thermal_coeffs(hits, n_hits, thermal))


# ---- polarized thermal continuum (lt_disk_thermal_spectrum_stokes, lt_shade_thermal_stokes) ----------------------------------
ATMOSPHERE_MAX_NODES = 4096


@dataclass
class Atmosphere:
    """A scattering atmosphere on the disk's surface (include/ltrace.h, "polarized thermal continuum"): two float64 tables of
    n_mu nodes, node i at mu = i / (n_mu - 1), linearly interpolated -- limb, the limb-darkening factor h(mu) with 1 meaning
    isotropic, and poldeg, the polarization degree delta(mu) of light leaving at the cosine mu to the normal.  The light is
    polarized parallel to the surface: the records it weights are those traced with the field (0, 0, 1)."""
    limb: np.ndarray
    poldeg: np.ndarray

    def __post_init__(self):
        limb, poldeg = np.array(self.limb, dtype=np.float64), np.array(self.poldeg, dtype=np.float64)
        if limb.ndim != 1 or limb.shape != poldeg.shape or not 2 <= limb.size <= ATMOSPHERE_MAX_NODES:
            raise ValueError(f"Atmosphere: limb and poldeg must both be (n_mu,), n_mu 2 ... {ATMOSPHERE_MAX_NODES}")
        self.limb, self.poldeg = np.ascontiguousarray(limb), np.ascontiguousarray(poldeg)

    @property
    def n_mu(self):
        return self.limb.size

    def nodes(self):
        """The cosines of the tables' nodes, (n_mu,)."""
        return np.arange(self.n_mu) / float(self.n_mu - 1)

    def to_lt(self):
        """The lt_atmosphere struct of these tables (ltrace.Atmosphere); the tables themselves are passed beside it."""
        import ltrace
        return ltrace.Atmosphere(self.n_mu, 0)

    @classmethod
    def isotropic(cls, n_mu=2):
        """No atmosphere: h = 1 and delta = 0 at every node.  The I plane is then the unpolarized continuum's, Q and U are 0."""
        return cls(np.ones(int(n_mu)), np.zeros(int(n_mu)))

    @classmethod
    def chandrasekhar(cls, n_mu=257):
        """A pure electron-scattering atmosphere by a closed-form fit: h proportional to 1 + 2.3 mu - 0.3 mu^2, normalized so that
        2 int_0^1 h mu dmu = 1 (h = (1 + 2.3 mu - 0.3 mu^2) / (143 / 60): the atmosphere redistributes the flux and does not
        change it), and delta = 0.1171 (1 - mu) / (1 + 3.582 mu), 11.71 % at grazing emission and 0 along the normal.
        The fit's coefficients are quoted from memory of the literature and were not checked against Chandrasekhar's table
        when this was written: callers who hold the table pass it to Atmosphere(limb, poldeg) themselves."""
        mu = np.arange(int(n_mu)) / float(int(n_mu) - 1)
        return cls((1.0 + 2.3 * mu - 0.3 * mu * mu) / (143.0 / 60.0), 0.1171 * (1.0 - mu) / (1.0 + 3.582 * mu))


def atmosphere_weights(pol, atmosphere):
    """The header's steps 6 and 7 for every slot of pol (..., max_images, 4) float32 (q, u, sin zeta, mu) -> (w, ok): w
    (..., max_images, 3) float64, the weights (w_I, w_Q, w_U) = (h, (h d) q, (h d) u) with h and d interpolated at mu by fma,
    and ok (..., max_images), whether the slot's mu lies in [0, 1] (w = 0 elsewhere).  Every operation is the header's, in
    its order and rounded as there."""
    p = np.asarray(pol, dtype=np.float32).astype(np.float64)
    mu, n = p[..., 3], atmosphere.n_mu
    with np.errstate(invalid="ignore"):
        ok = (mu >= 0.0) & (mu <= 1.0)
    v = np.where(ok, mu, 0.0) * float(n - 1)
    i0 = np.clip(np.floor(v).astype(np.int64), 0, n - 2)
    wt = v - i0.astype(np.float64)
    limb, poldeg = atmosphere.limb, atmosphere.poldeg
    h = fma(wt, limb[i0 + 1] - limb[i0], limb[i0])
    d = fma(wt, poldeg[i0 + 1] - poldeg[i0], poldeg[i0])
    hd = h * d
    with np.errstate(invalid="ignore"):
        w = np.stack([h, hd * p[..., 0], hd * p[..., 1]], axis=-1)
    return np.where(ok[..., None], w, 0.0), ok


def thermal_spectrum_stokes(hits, n_hits, pol, thermal, atmosphere, nu):
    """lt_disk_thermal_spectrum_stokes restated: (planes, 3, n_freq) float64, per plane, Stokes parameter (I, Q, U) and frequency
    ((nu nu) nu) times the sum of w_X A / expm1(nu c) over the emitting slots of all pixels (the products are rounded and the
    order of the sum is numpy's, where the kernel adds by fma in its own order); planes as thermal_spectrum's."""
    nu = _frequencies(nu, THERMAL_MAX_FREQS)
    A, c, emits = thermal_coeffs(hits, n_hits, thermal)
    w, ok = atmosphere_weights(pol, atmosphere)
    return _thermal_planes(thermal, nu, A, c, emits & ok, w)


def shade_thermal_stokes(hits, n_hits, pol, thermal, atmosphere, nu):
    """lt_shade_thermal_stokes restated: (n_freq, 3, R, W) float32 band images -- per pixel, band and Stokes parameter the emitting
    slots' w_X A / expm1(nu c) added in slot order in float64 by fma, times (nu nu) nu, rounded once to float32."""
    if thermal.split_orders:
        raise ValueError("shade_thermal_stokes: a band image has one plane per band; split_orders must be off")
    nu = _frequencies(nu, THERMAL_MAX_BANDS)
    A, c, emits = thermal_coeffs(hits, n_hits, thermal)
    w, ok = atmosphere_weights(pol, atmosphere)
    return _thermal_bands(nu, A, c, emits & ok, w)


def polarization_degree_angle(iqu, axis=-2):
    """(sqrt(Q^2 + U^2) / I, atan2(U, Q) / 2) of Stokes parameters whose axis `axis` is (I, Q, U) -- the last but one of
    thermal_spectrum_stokes' (planes, 3, n_freq); axis=1 for the band images' (n_bands, 3, R, W).  The degree is NaN where I is
    0; the angle, in radians in (-pi/2, pi/2], is counted from the screen's e_1 towards e_2 as (q, u) of the records are."""
    iqu = np.moveaxis(np.asarray(iqu, dtype=np.float64), axis, 0)
    i, q, u = iqu[0], iqu[1], iqu[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        deg = np.where(i == 0, np.nan, np.hypot(q, u) / np.where(i == 0, 1.0, i))
    return deg, 0.5 * np.arctan2(u, q)


# ---- reverberation (lt_disk_transfer) ---------------------------------------------------------------------------------------------
TRANSFER_MAX_TAU, TRANSFER_MAX_KEYS = 1024, 32768


@dataclass
class TransferGrid:
    """A linear grid in the delay tau between the direct flash and its echo (include/ltrace.h, "reverberation"): n_tau
    half-open bins on [tau_min, tau_max), an underflow row before them and an overflow row after.  tau_min may be negative."""
    tau_min: float = 0.0
    tau_max: float = 256.0
    n_tau: int = 64

    def __post_init__(self):
        if not (np.isfinite(self.tau_min) and np.isfinite(self.tau_max) and self.tau_min < self.tau_max):
            raise ValueError("TransferGrid needs tau_min < tau_max, both finite")
        if int(self.n_tau) != self.n_tau or not 1 <= self.n_tau <= TRANSFER_MAX_TAU:
            raise ValueError(f"TransferGrid n_tau must be 1 ... {TRANSFER_MAX_TAU}")
        self.tau_min, self.tau_max, self.n_tau = float(self.tau_min), float(self.tau_max), int(self.n_tau)

    def edges(self):
        """The n_tau + 1 edges of the bins proper, tau_min ... tau_max (rows 1 ... n_tau of a transfer function)."""
        e = self.tau_min + (self.tau_max - self.tau_min) * np.arange(self.n_tau + 1) / self.n_tau
        e[-1] = self.tau_max
        return e

    def centres(self):
        e = self.edges()
        return 0.5 * (e[:-1] + e[1:])

    def to_lt(self, r_min, r_max, n_r, t_ref):
        """The lt_transfer struct of this grid and of tables of n_r nodes on [r_min, r_max] (ltrace.Transfer)."""
        import ltrace
        return ltrace.default_transfer(tau_min=self.tau_min, tau_max=self.tau_max, n_tau=self.n_tau, n_r=int(n_r), r_min=float(r_min),
                                       r_max=float(r_max), t_ref=float(t_ref))


def transfer_bin(tau, grid):
    """The header's step 4, vectorised: the row (int64) of every float64 delay; 0 the underflow, n_tau + 1 the overflow,
    -1 for a NaN (it contributes nothing)."""
    return _linear_bin(np.asarray(tau, dtype=np.float64), grid.tau_min, grid.tau_max, grid.n_tau)


def transfer_slots(hits, n_hits, exposure, spec, grid, r_min, r_max, delay, emis, t_ref):
    """The header's steps 1 to 5 for every slot of hits (..., max_images, 4) float32 -> (on, k_tau, k_g, weight), each
    (..., max_images): which slots contribute, their row and column, and their weight (0 where nothing contributes).  Every
    operation is the header's, in its order and rounded as there (the interpolations by fma)."""
    h = np.asarray(hits, dtype=np.float32)
    m = h.shape[-2]
    r, g, dt = h[..., 0].astype(np.float64), h[..., 2].astype(np.float64), h[..., 3].astype(np.float64)
    delay, emis = np.asarray(delay, dtype=np.float64), np.asarray(emis, dtype=np.float64)
    n_r = delay.size
    if delay.shape != (n_r,) or emis.shape != (n_r,) or n_r < 2:
        raise ValueError("delay and emis must both be (n_r,), n_r >= 2")
    r_min, r_max, t_ref, exposure = float(r_min), float(r_max), float(t_ref), float(exposure)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        on = (_stored(h, n_hits)[..., None] > np.arange(m)) & (g > 0.0) & ~np.isnan(dt) & (r >= r_min) & (r <= r_max)      # step 1
        inv_dr = float(n_r - 1) / (r_max - r_min)
        v = (np.where(on, r, r_min) - r_min) * inv_dr                                                                    # step 2
        i0 = np.clip(v.astype(np.int64), 0, n_r - 2)
        w = v - i0.astype(np.float64)
        eps = fma(w, emis[i0 + 1] - emis[i0], emis[i0])                                                                  # step 3
        on = on & (eps > 0.0)
        t_ld = fma(w, delay[i0 + 1] - delay[i0], delay[i0])
        tau = (t_ld + np.where(on, dt, 0.0)) - t_ref                                                                     # step 4
        k_tau = transfer_bin(tau, grid)
        on = on & (k_tau >= 0)
        k_g = spectrum_bin(h[..., 2], spec)
        g2 = g * g
        weight = np.where(on, exposure * (g2 * g2) * np.where(on, eps, 0.0), 0.0)                                        # step 5
        on = on & ~(weight == 0.0)
    return on, np.where(on, k_tau, 0), np.where(on, k_g, 0), weight


def disk_transfer(hits, n_hits, exposure, spec, grid, r_min, r_max, delay, emis, t_ref):
    """lt_disk_transfer restated: the delay-energy transfer function, (planes, n_tau + 2, n_bins + 2) float64 -- per stored
    slot exposure g^4 eps(r) added to the key (image order, row of tau = t_ld(r) + dt - t_ref, column of g); the order of
    the sums is numpy's, not the kernel's.  planes is 1, or max_images with spec.split_orders."""
    on, k_tau, k_g, weight = transfer_slots(hits, n_hits, exposure, spec, grid, r_min, r_max, delay, emis, t_ref)
    m = on.shape[-1]
    rows, cols, planes = grid.n_tau + 2, spec.n_bins + 2, spec.planes(m)
    if planes * rows * cols > TRANSFER_MAX_KEYS:
        raise ValueError(f"disk_transfer: planes (n_tau + 2) (n_bins + 2) = {planes * rows * cols} keys exceed {TRANSFER_MAX_KEYS}")
    return _keyed_sum(on, spec.split_orders, k_tau, rows, k_g, cols, weight)


def impulse_response(tf):
    """A transfer function summed over g: (..., n_tau + 2), the echo's light per delay row (both underflows included)."""
    return np.asarray(tf, dtype=np.float64).sum(axis=-1)


def reverberation_line(tf):
    """A transfer function summed over tau: (..., n_bins + 2), the broadened line of the same emissivity."""
    return np.asarray(tf, dtype=np.float64).sum(axis=-2)


def lag_frequency(tf, grid, freqs, g_lo, g_hi, reflection_fraction=1.0):
    """The lag-frequency spectrum of the band of g columns [g_lo, g_hi) of a transfer function against the flash itself:
    arg(1 + R FT[psi](f)) / (2 pi f), psi the band's response over the delay bins proper divided by its sum, R the
    reflection fraction and FT a plain sum over the bin centres, sum_k psi_k exp(2 pi i f tau_k).  Planes are added.
    -> (len(freqs),) float64; a positive lag is the echo trailing the flash."""
    tf = np.asarray(tf, dtype=np.float64)
    tf = tf.reshape((-1,) + tf.shape[-2:]).sum(axis=0)
    psi = tf[1:-1, int(g_lo):int(g_hi)].sum(axis=1)
    if not psi.sum() > 0.0:
        raise ValueError("lag_frequency: the band holds no light on the delay grid")
    psi = psi / psi.sum()
    f = np.asarray(freqs, dtype=np.float64).ravel()
    ft = (psi[None, :] * np.exp(2j * np.pi * f[:, None] * grid.centres()[None, :])).sum(axis=1)
    return np.angle(1.0 + float(reflection_fraction) * ft) / (2.0 * np.pi * f)


@dataclass
class Lamppost:
    """A point source on the spin axis of a Kerr hole (M, a) at Boyer-Lindquist radius h, at rest and isotropic in the
    local static frame: the lamp-post corona.  Its photons have p_phi = 0 exactly; they are launched from (r = h, theta =
    theta0) with a small theta0 -- the axis itself is a coordinate singularity -- at local angles delta from the outward
    radial direction and integrated with the metric's own 8-D geodesic_equations (metrics.Kerr), host-side float64.
    n_r, n_rays: the size of the tables render_sequence asks for and the rays they are interpolated from."""
    M: float = 1.0
    a: float = 0.0
    h: float = 6.0
    theta0: float = 1e-4                                       # (the source sits h theta0 off the axis: the delays move by that much)
    rtol: float = 1e-10
    n_r: int = 256
    n_rays: int = 128

    def __post_init__(self):
        self.M, self.a, self.h = float(self.M), float(self.a), float(self.h)
        if not (self.M > 0.0 and abs(self.a) <= self.M):
            raise ValueError("Lamppost needs M > 0 and |a| <= M")
        if not self.h > 1.05 * (self.M + np.sqrt(self.M * self.M - self.a * self.a)):
            raise ValueError("Lamppost: h must lie outside the horizon")

    def _metric(self):
        from metrics import Kerr
        return Kerr(M=self.M, a=self.a)

    def lapse(self):
        """sqrt(Delta(h) / (h^2 + a^2)): the source's clock against coordinate time, its photons' E_infinity / E_local."""
        return float(np.sqrt((self.h * self.h - 2.0 * self.M * self.h + self.a * self.a) / (self.h * self.h + self.a * self.a)))

    def initial_state(self, cos_delta):
        """The 8-D state (t, r, theta, phi, p_t, p_r, p_theta, p_phi) of the photon with E = 1 emitted at the local angle
        delta from the outward radial direction, in the zero-angular-momentum frame at (h, theta0) -- the static frame on the
        axis: p^(r) = E_loc cos delta, p^(theta) = E_loc sin delta, p^(phi) = 0."""
        M, a, r, th = self.M, self.a, self.h, self.theta0
        c = float(cos_delta)
        s = np.sqrt(max(1.0 - c * c, 0.0))
        Sigma = r * r + a * a * np.cos(th) ** 2
        Delta = r * r - 2.0 * M * r + a * a
        A = (r * r + a * a) ** 2 - a * a * Delta * np.sin(th) ** 2
        e_loc = np.sqrt(A / (Sigma * Delta))
        return [0.0, r, th, 0.0, -1.0, c * e_loc * np.sqrt(Sigma / Delta), s * e_loc * np.sqrt(Sigma), 0.0]

    def ray(self, cos_delta, r_far, to_equator=True):
        """solve_ivp's result for one photon: integrated until it crosses the equator downwards (to_equator), passes r_far
        outwards, or comes within 2 % of the horizon.  t_events: [equator crossings, r_far crossings, captures]."""
        from scipy.integrate import solve_ivp
        met = self._metric()
        equator = lambda lam, y: y[2] - 0.5 * np.pi
        equator.terminal, equator.direction = bool(to_equator), 1.0
        far = lambda lam, y: y[1] - r_far
        far.terminal, far.direction = True, 1.0
        captured = lambda lam, y: y[1] - 1.02 * met.r_plus
        captured.terminal, captured.direction = True, -1.0
        return solve_ivp(met.geodesic_equations, (0.0, 50.0 * (r_far + self.h)), self.initial_state(cos_delta), method="DOP853",
                         rtol=self.rtol, atol=1e-3 * self.rtol, events=(equator, far, captured))

    def crossing(self, cos_delta, r_far):
        """(r, t) of the photon's first crossing of the equatorial plane, or (nan, nan) if it escapes or is captured first."""
        sol = self.ray(cos_delta, r_far)
        if sol.t_events[0].size == 0:
            return np.nan, np.nan
        y = sol.y_events[0][0]
        return float(y[1]), float(y[0])

    def illumination(self, r_min, r_max, n_rays=None):
        """(cos delta, r, t), each (n_rays,): n_rays photons uniform in cos delta whose equatorial crossings cover [r_min,
        r_max], r ascending.  A coarse fan over all directions brackets the range first."""
        n_rays = int(self.n_rays if n_rays is None else n_rays)
        r_far = 4.0 * max(float(r_max), self.h) + 100.0 * self.M
        coarse = np.linspace(-1.0, 1.0, 131)[1:-1]
        rc = np.array([self.crossing(c, r_far)[0] for c in coarse])
        inner = np.flatnonzero(rc <= r_min)
        if inner.size == 0:
            raise ValueError("Lamppost: no photon reaches the disk inside r_min")
        lo = int(inner[-1])
        outer = np.flatnonzero((rc >= r_max) & (np.arange(rc.size) > lo))
        if outer.size == 0:
            raise ValueError("Lamppost: no photon reaches the disk beyond r_max")
        hi = int(outer[0])
        if np.any(np.isnan(rc[lo:hi + 1])) or np.any(np.diff(rc[lo:hi + 1]) <= 0.0):
            raise ValueError("Lamppost: the crossing radius is not monotone in cos delta over the table's range")
        c = np.linspace(coarse[lo], coarse[hi], n_rays)
        rt = np.array([self.crossing(x, r_far) for x in c])
        if np.any(np.isnan(rt)) or np.any(np.diff(rt[:, 0]) <= 0.0):
            raise ValueError("Lamppost: the crossing radius is not monotone in cos delta over the table's range")
        return c, rt[:, 0], rt[:, 1]

    def tables(self, r_min, r_max, n_r=None, n_rays=None):
        """(delay, emis), each (n_r,) float64, on the uniform nodes of [r_min, r_max]: lamppost_tables of this source."""
        return lamppost_tables(self.M, self.a, self.h, r_min, r_max, self.n_r if n_r is None else n_r, n_rays=n_rays, source=self)

    def t_ref(self, r_obs, theta_obs):
        """The direct flash's arrival time at the camera at (r_obs, theta_obs): the coordinate time of the photon of the same
        family whose polar angle on reaching r = r_obs is theta_obs, found by brentq on cos delta."""
        from scipy.optimize import brentq
        r_obs, theta_obs = float(r_obs), float(theta_obs)
        if not r_obs > self.h:
            raise ValueError("Lamppost.t_ref: the camera must lie outside the source's radius")
        arrival = {}

        def miss(c):
            sol = self.ray(c, r_obs, to_equator=False)
            if sol.t_events[1].size == 0:
                return np.pi                                   # (captured: as far from the axis as an angle gets)
            y = sol.y_events[1][0]
            arrival[c] = float(y[0])
            return float(y[2]) - theta_obs

        hi = 1.0
        if miss(hi) >= 0.0:
            return arrival[hi]                                 # (a camera on the axis itself)
        lo = hi
        while miss(lo) < 0.0:
            hi, lo = lo, lo - 0.05
            if lo <= -1.0:
                raise ValueError("Lamppost.t_ref: no direct ray reaches the camera")
        c = brentq(miss, lo, hi, xtol=1e-14, rtol=1e-14)
        miss(c)
        return arrival[c]


def lamppost_tables(M, a, h, r_min, r_max, n_r, n_rays=None, source=None):
    """The two float64 tables of lt_disk_transfer for a lamp-post corona (Lamppost) on the n_r uniform nodes of [r_min,
    r_max] -> (delay, emis): delay the coordinate time from the source to the disk at the node, interpolated from the
    rays' crossings; emis = g_ld^2 |d cos delta / dr| / (gamma sqrt(g_rr g_phiphi)) at the equator -- the photons the ring
    [r, r + dr] receives per proper area of the orbiting gas, each shifted by g_ld = u^t(r) sqrt(Delta(h) / (h^2 + a^2)) in
    energy and again in rate -- with gamma the Lorentz factor of the Keplerian gas against the zero-angular-momentum
    frame.  The normalisation is free: the disk's exposure sets it.  The interpolation is monotone cubic (pchip) in r."""
    from scipy.interpolate import PchipInterpolator
    src = source if source is not None else Lamppost(M, a, h)
    M, a = src.M, src.a
    r_min, r_max, n_r = float(r_min), float(r_max), int(n_r)
    c, rr, tt = src.illumination(r_min, r_max, n_rays)
    nodes = r_min + np.arange(n_r) * (r_max - r_min) / (n_r - 1)
    nodes[-1] = min(nodes[-1], rr[-1])                        # (rounding of the last node, inside the fan's last crossing)
    delay = PchipInterpolator(rr, tt)(nodes)
    dc_dr = PchipInterpolator(rr, c).derivative()(nodes)
    Delta = nodes * nodes - 2.0 * M * nodes + a * a
    A = (nodes * nodes + a * a) ** 2 - a * a * Delta
    g_rr, g_pp = nodes * nodes / Delta, A / (nodes * nodes)
    v = (omega(M, a, nodes) - 2.0 * M * a * nodes / A) * np.sqrt(g_pp) / np.sqrt(nodes * nodes * Delta / A)
    gamma = 1.0 / np.sqrt(1.0 - v * v)
    g_ld = u_t(M, a, nodes) * src.lapse()
    emis = g_ld * g_ld * np.abs(dc_dr) / (gamma * np.sqrt(g_rr * g_pp))
    return np.ascontiguousarray(delay), np.ascontiguousarray(emis)
