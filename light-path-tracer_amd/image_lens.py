"""Gravitational lensing of a background image -- MI355X backend.

Same public surface as the reference's image_lens.py (function names, arguments,
return values, CLI flags), so `import image_lens` / `python image_lens.py --a 0.9`
keep working.  Coordinates are (y, x); FOV pairs are (horizontal, vertical).

Where the work happens:

  * every per-pixel array is produced on the GPU: `build_alpha_lookup` (lt_pixel_angles),
    `precompute_final_alpha_lookup[_2d]` (the metric's `trace_rays_batch`, i.e.
    lt_trace_batch_*), `render_lensed_image` (lt_shade);
  * `render_frame` / `main()` use the fused path (lt_render): pixel -> ray -> colour in one
    call, nothing per-ray crosses PCIe on the way in;  `main(staged=True)` runs the
    reference's three-call sequence instead, stage by stage on the GPU.

The scalar camera helpers (`_psi_frame`, `pixel_to_angles`, `angles_to_pixel`) are a few
float64 operations and stay on the host.  No CPU tracer exists in this package.
"""
from time import perf_counter

import json
import os
import sys

import numpy as np

import ltrace
from metrics import Kerr, Schwarzschild

WINDING_DTYPE = np.uint16
WINDING_MAX = np.iinfo(WINDING_DTYPE).max
Y_AXIS_REFINE_FRAC = 0.07
TRACE_CHUNK = 4_000_000   # rays per trace_rays_batch call (the reference uses 50 000 for its tqdm bar)


# ---------------------------------------------------------------------------------------------
# camera model (host scalars)
# ---------------------------------------------------------------------------------------------
def _psi_to_bh_direction(psi):
    """psi = (pitch_up, yaw_right) [rad] -> unit vector to the BH in camera axes (+x right, +y down,
    +z forward)."""
    pitch, yaw = psi
    return np.array([np.sin(yaw) * np.cos(pitch), -np.sin(pitch), np.cos(yaw) * np.cos(pitch)], dtype=np.float64)


def _unit(v, fallback):
    n = np.linalg.norm(v)
    if n < 1e-12:
        v = fallback()
        n = np.linalg.norm(v)
    return v / max(n, 1e-12)


def _psi_frame(psi):
    """(d, e_x, e_y, in_front): BH direction and the screen basis around it (Gram-Schmidt of the
    camera's x and y axes against d; e_x / e_y coincide with the image axes at psi = 0)."""
    d = _psi_to_bh_direction(psi)
    x_hat = np.array([1.0, 0.0, 0.0])
    y_hat = np.array([0.0, 1.0, 0.0])
    e_x = _unit(x_hat - (x_hat @ d) * d, lambda: y_hat - (y_hat @ d) * d)
    e_y = _unit(y_hat - (y_hat @ d) * d - (y_hat @ e_x) * e_x, lambda: np.cross(d, e_x))
    return d, e_x, e_y, bool(d[2] > 1e-12)


def _psi_to_cam_projection(psi):
    """(y_cam, x_cam, in_front) of the BH on the pinhole plane; NaNs if it is behind the camera."""
    d, _, _, front = _psi_frame(psi)
    if not front:
        return (np.nan, np.nan, False)
    return (float(d[1] / d[2]), float(d[0] / d[2]), True)


def _focal(image_dimension, fov):
    height, width = image_dimension
    return (width / 2) / np.tan(fov[0] / 2), (height / 2) / np.tan(fov[1] / 2)


def pixel_to_angles(pixel, image_dimension, fov, psi=(0.0, 0.0)):
    """(alpha, theta) of one pixel (y, x): angle from the BH direction and screen azimuth."""
    height, width = image_dimension
    fx, fy = _focal(image_dimension, fov)
    ray = np.array([(pixel[1] - width / 2) / fx, (pixel[0] - height / 2) / fy, 1.0])
    ray /= np.linalg.norm(ray)
    d, e_x, e_y, _ = _psi_frame(psi)
    return (float(np.arccos(np.clip(ray @ d, -1.0, 1.0))), float(np.arctan2(ray @ e_x, ray @ e_y)))


def angles_to_pixel(angles, image_dimension, fov, clip=False, psi=(0.0, 0.0)):
    """Inverse of pixel_to_angles -> (py, px); (-1, -1) (or (0, 0) with clip) behind the camera."""
    alpha, theta = angles
    height, width = image_dimension
    fx, fy = _focal(image_dimension, fov)
    d, e_x, e_y, _ = _psi_frame(psi)
    ray = np.cos(alpha) * d + np.sin(alpha) * (np.sin(theta) * e_x + np.cos(theta) * e_y)
    if ray[2] <= 1e-12:
        return (0, 0) if clip else (-1, -1)
    px = int(np.rint(ray[0] / ray[2] * fx + width / 2))
    py = int(np.rint(ray[1] / ray[2] * fy + height / 2))
    if clip:
        px, py = int(np.clip(px, 0, width - 1)), int(np.clip(py, 0, height - 1))
    return (py, px)


def _camera(image_dimension, fov, psi, r_obs=50.0, theta_obs=np.pi / 2):
    height, width = image_dimension
    return ltrace.Camera(int(width), int(height), float(fov[0]), float(fov[1]), float(psi[0]), float(psi[1]),
                         float(r_obs), float(theta_obs))


# ---------------------------------------------------------------------------------------------
# stage 1: per-pixel alpha
# ---------------------------------------------------------------------------------------------
def build_alpha_lookup(image_dimension, fov, decimals=None, psi=(0.0, 0.0)):
    """(H, W) float32 viewing angle per pixel corner (GPU: lt_pixel_angles)."""
    alpha, _, _ = ltrace.pixel_angles(_camera(image_dimension, fov, psi), want_theta=False)
    if decimals is not None:
        alpha = np.round(alpha.astype(np.float64), decimals).astype(np.float32)
    return alpha


# ---------------------------------------------------------------------------------------------
# stage 2: trace one ray per pixel
# ---------------------------------------------------------------------------------------------
def _empty_lookup(shape):
    return np.full(shape, np.nan, dtype=np.float32), np.zeros(shape, dtype=WINDING_DTYPE)


def precompute_final_alpha_lookup(alpha_lookup, alpha_crit, r_obs, metric, dedup=False):
    """Spherically symmetric metrics: every pixel traced from its alpha alone.
    -> (final_alpha f32, winding u16, total_rays, traced_rays).

    dedup=True traces every DISTINCT float32 alpha once and hands the result to all pixels that share it (the idea of
    the reference's dormant debugging_image_lense.py:634): a pinhole frame has 8-fold symmetry, so at most
    ~N/8 + O(sqrt N) values are distinct.  Same alpha, same ray: the lookups are byte-identical to the full trace; only
    `traced_rays` differs.  Off by default, as in the reference's live function (which traces all N)."""
    alpha = alpha_lookup.ravel().astype(np.float64)
    n = alpha.size
    if n == 0:
        fa, w = _empty_lookup(alpha_lookup.shape)
        return fa, w, n, 0
    inverse = None
    if dedup:
        alpha, inverse = np.unique(alpha, return_inverse=True)
    m = alpha.size
    fa = np.full(m, np.nan, dtype=np.float64)
    w = np.zeros(m, dtype=np.int64)
    for lo in range(0, m, TRACE_CHUNK):
        hi = min(lo + TRACE_CHUNK, m)
        metric.trace_rays_batch(r_obs, alpha[lo:hi], fa[lo:hi], w[lo:hi])
    if inverse is not None:
        fa, w = fa[inverse.ravel()], w[inverse.ravel()]
    return (fa.astype(np.float32).reshape(alpha_lookup.shape),
            np.clip(w, 0, WINDING_MAX).astype(WINDING_DTYPE).reshape(alpha_lookup.shape), n, m)


def precompute_final_alpha_lookup_2d(alpha_lookup, fov, alpha_crit, r_obs, metric,
                                     theta_obs=np.pi / 2, psi=(0.0, 0.0)):
    """Non-spherical metrics: (alpha, theta) per pixel, axis-refine columns, and the reference's
    top/bottom mirror (rows 0..(H+1)//2-1 traced, row j copied to row H-1-j) when theta_obs = pi/2
    and psi_y = 0.  -> (final_alpha f32, winding u16, total_rays, traced_rays)."""
    height, width = alpha_lookup.shape
    _, theta, refine_cols = ltrace.pixel_angles(_camera((height, width), fov, psi), Y_AXIS_REFINE_FRAC)
    mirror = bool(np.isclose(theta_obs, np.pi / 2) and np.isclose(psi[0], 0.0))
    rows = (height + 1) // 2 if mirror else height
    n = rows * width
    print(f"  tracing {n:,} rays " + ("with top/bottom symmetry " if mirror else "")
          + f"({alpha_lookup.size:,} pixels total)")
    fa_out, w_out = _empty_lookup((height, width))
    if n:
        alpha = alpha_lookup[:rows].ravel().astype(np.float64)
        th = np.ascontiguousarray(theta[:rows]).ravel()
        refine = np.broadcast_to(refine_cols[None, :], (rows, width)).ravel()
        fa = np.full(n, np.nan, dtype=np.float64)
        w = np.zeros(n, dtype=np.int64)
        for lo in range(0, n, TRACE_CHUNK):
            hi = min(lo + TRACE_CHUNK, n)
            metric.trace_rays_batch(r_obs, alpha[lo:hi], th[lo:hi], theta_obs,
                                    np.ascontiguousarray(refine[lo:hi]), fa[lo:hi], w[lo:hi])
        fa_out[:rows] = fa.astype(np.float32).reshape(rows, width)
        w_out[:rows] = np.clip(w, 0, WINDING_MAX).astype(WINDING_DTYPE).reshape(rows, width)
    if mirror and height // 2 > 0:
        half = height // 2
        fa_out[height - half:] = fa_out[:half][::-1]
        w_out[height - half:] = w_out[:half][::-1]
    return fa_out, w_out, int(alpha_lookup.size), int(n)


# ---------------------------------------------------------------------------------------------
# stage 3: colouring
# ---------------------------------------------------------------------------------------------
WINDING_COLORS = np.array([
    [0.0, 0.2, 1.0],   # blue
    [0.0, 0.7, 1.0],   # sky blue
    [0.0, 1.0, 0.4],   # green
    [1.0, 1.0, 0.0],   # yellow
    [1.0, 0.4, 0.0],   # orange
], dtype=np.float32)


def render_lensed_image(source_image, alpha_lookup, final_alpha_lookup, winding_lookup, alpha_crit, fov,
                        render_loop_around=False, psi=(0.0, 0.0)):
    """Output image from the lookups (GPU: lt_shade): captured -> black, exit angle beyond pi/2 ->
    WINDING_COLORS[min(winding, 4)], otherwise the background pixel the exit direction points at
    (magenta outside the frame, or wrapped with render_loop_around).  `alpha_lookup` and `alpha_crit`
    are accepted for signature compatibility; like the reference, nothing reads them."""
    src = np.asarray(source_image)
    out = ltrace.shade(_camera(src.shape[:2], fov, psi), src.astype(np.float32, copy=False),
                       final_alpha_lookup, winding_lookup, loop_around=render_loop_around)
    return out.astype(src.dtype, copy=False) if src.dtype.kind == "f" else out


def render_frame(source_image, metric, r_obs, fov, psi=(0.0, 0.0), theta_obs=np.pi / 2, integrator=None,
                 precision=None, schedule=None, tb_symmetry=False, render_loop_around=False,
                 want=("fa", "winding", "rgb"), gpus=1, devices=None, disk=None, samples=None, adaptive=None, contrast=None):
    """Fused path (lt_render): all three stages in one GPU call.  source_image None -> shadow render
    (escaped = white).  Returns dict with 'fa', 'winding', 'rgb', ... and 'stats'.
    gpus > 1: the frame's rows are split block-cyclically over that many devices of this node
    (lt_render_multi; the reference's top/bottom mirror needs the whole frame on one device).
    disk: a thin accretion disk (disk.ThinDisk or ltrace.Disk) -> lt_render_disk on one GPU, every row traced, plus
    'disk' (H, W, 3) (r_hit, phi_hit, g); a spherically symmetric metric is traced as Kerr with a = 0.
    An optically thin disk (disk.TransparentDisk: anything with a max_images) -> lt_render_disk_images instead, plus
    'disk_images' (H, W, max_images, 3) (r_hit, phi_hit, g) of the first hits along the ray and 'disk_hits' (H, W).
    samples: S -> lt_render_aa: S x S rays per pixel resolved on the GPU (anti-aliasing).  source_image is then the
    FINE-size background (H S, W S[, 3]) and the frame is (H, W); the result holds 'rgb', 'rgba', 'cover' (H, W, 4)
    (sub-rays escaped / captured / invalid / on the disk) and 'stats' only, with no disk, a ThinDisk or a
    TransparentDisk; one GPU, every row traced.
    adaptive: S_lo (with samples = S_hi > S_lo) -> lt_render_aa_adaptive: S_lo x S_lo rays for every pixel, S_hi x S_hi
    only for the pixels on an edge (mixed cover, a neighbour of another cover, or a colour step above `contrast`;
    contrast None: the library's default, negative: the colour test off).  source_image is then the PAIR of backgrounds
    (at (H S_lo, W S_lo[, 3]), at (H S_hi, W S_hi[, 3])), and the result gains 'level' (H, W) (the samples per axis each
    pixel got) and stats['refined']."""
    if source_image is None:
        raise ValueError("render_frame needs a background; for a shadow use black_hole_shadow.render_traced")
    source_lo = None
    if adaptive is not None:
        if samples is None:
            raise ValueError("adaptive=S_lo needs samples=S_hi")
        if not (isinstance(source_image, (tuple, list)) and len(source_image) == 2):
            raise ValueError("adaptive: the background is the pair (at the S_lo fine size, at the S_hi fine size)")
        source_lo = np.asarray(source_image[0])
        if source_lo.ndim == 3 and source_lo.shape[2] == 4:
            source_lo = source_lo[..., :3]
        source_image = source_image[1]
    source_image = np.asarray(source_image)
    if source_image.ndim == 3 and source_image.shape[2] == 4:
        # RGBA input (a PNG background): the reference's renderer cannot colour winding pixels of a 4-channel image
        # (it assigns 3-channel WINDING_COLORS, image_lens.py:329-331) and turns black / magenta pixels transparent;
        # the colour planes are what is lensed here
        source_image = source_image[..., :3]
    shape = source_image.shape[:2]
    kerr = not metric.is_spherically_symmetric or disk is not None
    met = ltrace.Metric(ltrace.METRIC_KERR if kerr else ltrace.METRIC_SCHWARZSCHILD, 0, float(metric.M),
                        float(getattr(metric, "a", 0.0)))
    opts = ltrace.default_opts(
        integrator=integrator or getattr(metric, "integrator", "rk4"),
        precision=precision or getattr(metric, "precision", 32),
        schedule=schedule or getattr(metric, "schedule", "direct"),
        tb_symmetry=int(bool(tb_symmetry)), loop_around=int(bool(render_loop_around)),
        axis_refine_frac=Y_AXIS_REFINE_FRAC)
    if samples is not None:
        S = int(samples)
        if gpus and gpus > 1:
            raise ValueError("a supersampled frame renders on one GPU (gpus == 1)")
        if S < 1 or shape[0] % S or shape[1] % S:
            raise ValueError(f"samples={S}: the background must be the fine frame, (H * samples, W * samples); got {shape}")
        cam = _camera((shape[0] // S, shape[1] // S), fov, psi, r_obs, theta_obs)
        d = None if disk is None else (disk.to_lt() if hasattr(disk, "to_lt") else disk)
        max_images = getattr(disk, "max_images", None)
        mode = "plain" if disk is None else ("disk" if max_images is None else "disk_images")
        more = {} if max_images is None else dict(max_images=int(max_images))
        if adaptive is not None:
            S_lo = int(adaptive)
            if S_lo < 1 or source_lo.shape[:2] != (cam.height * S_lo, cam.width * S_lo):
                raise ValueError(f"adaptive={S_lo}: the first background must be (H * adaptive, W * adaptive) = "
                                 f"{(cam.height * max(S_lo, 0), cam.width * max(S_lo, 0))}; got {source_lo.shape[:2]}")
            if contrast is not None:
                more["contrast"] = float(contrast)
            ad = ltrace.default_aa_adaptive(samples_lo=S_lo, samples_hi=S, mode=mode, **more)
            return ltrace.render_aa_adaptive(cam, met, opts, ad, disk=d, background_lo=source_lo, background_hi=source_image,
                                             want=tuple(w for w in tuple(want) + ("cover", "level") if w in ("rgb", "rgba", "cover", "level")))
        aa = ltrace.default_aa(samples=S, mode=mode, **more)
        return ltrace.render_aa(cam, met, opts, aa, disk=d, background=source_image,
                                want=tuple(w for w in tuple(want) + ("cover",) if w in ("rgb", "rgba", "cover")))
    cam = _camera(shape, fov, psi, r_obs, theta_obs)
    if disk is not None:
        if gpus and gpus > 1:
            raise ValueError("the accretion disk renders on one GPU (gpus == 1)")
        d = disk.to_lt() if hasattr(disk, "to_lt") else disk
        max_images = getattr(disk, "max_images", None)
        if max_images is not None:
            out = ltrace.render_disk_images(cam, met, opts, d, max_images=max_images, background=source_image,
                                            want=tuple(want) + ("images", "n_hits"))
            out["disk_images"], out["disk_hits"] = out.pop("images"), out.pop("n_hits")
            return out
        return ltrace.render_disk(cam, met, opts, d, background=source_image, want=tuple(want) + ("disk",))
    if gpus and gpus > 1:
        if tb_symmetry:
            raise ValueError("tb_symmetry (the reference's top/bottom mirror) needs gpus == 1")
        if devices is None and os.environ.get("LT_MULTI_DEVICES"):   # e.g. "0,0": rehearse 2 partitions on one GPU
            devices = [int(x) for x in os.environ["LT_MULTI_DEVICES"].split(",")]
        return ltrace.render_multi(cam, met, opts, gpus, devices=devices, background=source_image, want=want)
    return ltrace.render(cam, met, opts, background=source_image, want=want)


def render_sequence(source_image, metric, r_obs, fov, disk, hotspot, times, shape=None, psi=(0.0, 0.0), theta_obs=np.pi / 2,
                    integrator=None, precision=None, bfield=None, samples=None, diskmap=None, spectrum=None, baselines=None,
                    thermal=None, frequencies=None, bands=None, lamppost=None, transfer=None, atmosphere=None):
    """A moving picture from ONE trace: an optically thin disk (disk.TransparentDisk) with a hot spot (disk.HotSpot) on a
    circular orbit, at the observer times `times`.  The rays are traced once with the light-travel time of every hit
    (lt_trace_disk_hits); each frame is a re-shade of the stored hits (lt_shade_hotspot) over `base`, the lensed
    source_image (None: black, then `shape` = (H, W) gives the size), and the light curve is a reduction over them
    (lt_hotspot_lightcurve, at times[0] + i (times[1] - times[0]): the times must be evenly spaced).
    -> dict(frames (n, H, W[, 3]) float32, rgba (n, H, W, 4) uint8, lightcurve (n, 3) float64, hits, n_hits, stats).
    bfield (disk.BField): the trace also keeps every hit's linear polarization (lt_trace_disk_pol), and the result gains
    pol (H, W, max_images, 4), stokes (n, H, W, 3) float32 (I, Q, U per frame; lt_shade_stokes) and stokes_lightcurve
    (n, 3) float64 (lt_hotspot_lightcurve_stokes); everything else is what it is without a field.
    samples: S (1 ... 8) -> an anti-aliased sequence: the rays of the FINE camera (H S, W S) are traced once, one ray per
    fine pixel, and every frame is re-shaded and resolved S x S -> 1 on the GPU (lt_shade_hotspot_aa; stokes:
    lt_shade_stokes_aa), so only (H, W) frames come back.  source_image, when given, is then the fine image
    (H S, W S[, 3]) as in render_frame, and `shape` stays the output's (H, W).  frames (n, H, W[, 3]), rgba (n, H, W, 4)
    and stokes (n, H, W, 3) have the output's size; hits, n_hits and pol are the FINE records; the result gains
    `samples`.  lightcurve is the fine records' curve in output-pixel units (column 0 divided by S^2, the first moments
    by S^3) and stokes_lightcurve the fine records' divided by S^2.  The fine records take 16 max_images S^2 H W bytes
    (twice that with a field) and are held for the whole sequence.  samples=None: one ray per pixel, as without it.
    diskmap (disk.DiskMap): the moving source is an emissivity table on the disk that turns with it instead of a spot;
    `hotspot` is then None.  Frames come from lt_shade_diskmap (samples: lt_shade_diskmap_aa) and the light curve from
    lt_diskmap_lightcurve, scaled as above; everything else is as with a spot.  A map together with a spot or with a
    field is refused: both are out of scope.  diskmap may also be a disk.DiskMovie, tables that change with time: the same
    keys come back from the lt_*diskmovie* entry points, every image order looking the movie up at its own emission time.
    spectrum (disk.Spectrum): the result gains `spectrum` (n, planes, n_bins + 2) float64, the moving emitter's dynamic
    spectrum over the grid in g (lt_hotspot_spectrum, or lt_diskmap_spectrum with a map), and `disk_spectrum`
    (planes, n_bins + 2), the stationary disk's line profile (lt_disk_spectrum); planes is 1, or max_images with
    spectrum.split_orders.  With `samples` both are the fine records' divided by S^2, as the light curve's first column.
    baselines (disk.Baselines, (u, v) in cycles per OUTPUT pixel): the result gains `visibility` (n, planes, n_baselines)
    complex128, the moving emitter's complex visibilities (lt_hotspot_visibility, or lt_diskmap_visibility with a map),
    and `disk_visibility` (planes, n_baselines), the stationary disk's (lt_disk_visibility); planes is 1, or max_images
    with baselines.split_orders.  Both are in output-pixel units with the phase referred to the frame's centre
    (Baselines.recentre); with `samples` they are computed on the fine records at (u / S, v / S).
    bfield and baselines together: the result also gains `visibility_stokes` (n, planes, 3, n_baselines) complex128, the
    spot's polarized visibilities (I, Q, U; lt_hotspot_visibility_stokes), and `disk_visibility_stokes` (planes, 3,
    n_baselines), the stationary disk's (lt_disk_visibility_stokes), recentred and scaled like `visibility`; their I plane
    is `visibility` / `disk_visibility`, and disk.fractional_polarization gives (Q~ + i U~) / I~.
    thermal (disk.ThermalDisk) with frequencies (up to 1024 float64, > 0): the result gains `thermal_spectrum` (planes,
    n_freq) float64, the stationary disk's thermal continuum at those frequencies (lt_disk_thermal_spectrum; planes is 1, or
    max_images with thermal.split_orders), and `thermal_frequencies`; with `samples` it is the fine records' divided by S^2,
    as `disk_spectrum`.  bands (up to 16 frequencies): the result also gains `thermal_bands` (n_bands, H, W) float32, the
    unclamped band images (lt_shade_thermal; with `samples` the fine images resolved S x S -> 1 per plane by aa.resolve).
    atmosphere (disk.Atmosphere) with thermal: the disk's surface is a scattering atmosphere.  The rays are traced with the
    polarization records of the field (0, 0, 1) (lt_trace_disk_pol; a bfield given as well must point along (0, 0, +-1),
    whose records are the same), and the result gains `thermal_spectrum_stokes` (planes, 3, n_freq) float64
    (lt_disk_thermal_spectrum_stokes) and `thermal_bands_stokes` (n_bands, 3, H, W) float32 (lt_shade_thermal_stokes), the
    Stokes axis (I, Q, U), divided or resolved with `samples` exactly as the thermal entries are, and `pol`.
    `thermal_spectrum` and `thermal_bands` stay the isotropic, unpolarized ones; disk.polarization_degree_angle divides.
    A map is not polarized: atmosphere with diskmap is refused.
    lamppost (disk.Lamppost) with transfer (disk.TransferGrid) and spectrum (the g axis): the result gains `transfer`
    (planes, n_tau + 2, n_bins + 2) float64, the disk's delay-energy response to a flash of that source (lt_disk_transfer;
    planes as the spectrum's; with `samples` the fine records' divided by S^2), `transfer_tau_edges` (n_tau + 1,) and
    `transfer_tables` (3, n_r): the nodes' radii, delay and emis, traced on the host from the disk's inner edge to r_out,
    and `transfer_t_ref`, the direct flash's arrival time at the camera that every delay is counted from.
    One GPU, every row traced; sequences are not adaptively sampled."""
    if (lamppost is None) != (transfer is None):
        raise ValueError("render_sequence: lamppost=Lamppost(...) and transfer=TransferGrid(...) go together")
    if lamppost is not None and spectrum is None:
        raise ValueError("render_sequence: a transfer function needs spectrum=Spectrum(...) for its g axis")
    if thermal is not None and frequencies is None and bands is None:
        raise ValueError("render_sequence: thermal needs frequencies= (the spectrum) or bands= (the band images)")
    if thermal is None and (frequencies is not None or bands is not None):
        raise ValueError("render_sequence: frequencies= and bands= belong to thermal=ThermalDisk(...)")
    if atmosphere is not None and thermal is None:
        raise ValueError("render_sequence: atmosphere= belongs to thermal=ThermalDisk(...)")
    if atmosphere is not None and diskmap is not None:
        raise ValueError("render_sequence: a disk map is not polarized; pass atmosphere=None")
    if atmosphere is not None and bfield is not None and not (bfield.b_r == 0.0 and bfield.b_phi == 0.0 and abs(bfield.b_z) > 0.0):
        raise ValueError("render_sequence: an atmosphere's polarization is that of the field (0, 0, +-1); pass such a bfield or none")
    if diskmap is not None and hotspot is not None:
        raise ValueError("render_sequence: a disk map together with a hot spot is out of scope; pass hotspot=None")
    if diskmap is not None and bfield is not None:
        raise ValueError("render_sequence: a disk map is not polarized; pass bfield=None")
    S = None
    if samples is not None:
        S = int(samples)
        if not 1 <= S <= ltrace.AA_MAX_SAMPLES:
            raise ValueError(f"samples={S}: a sequence takes 1 ... {ltrace.AA_MAX_SAMPLES} samples per axis")
    times = np.asarray(times, dtype=np.float64).ravel()
    if times.size == 0:
        raise ValueError("render_sequence needs at least one time")
    dt = float(times[1] - times[0]) if times.size > 1 else 0.0
    if times.size > 2 and np.max(np.abs(np.diff(times) - dt)) > 1e-9 * max(abs(dt), 1.0):
        raise ValueError("render_sequence: the times must be evenly spaced")
    base = None
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, float(metric.M), float(getattr(metric, "a", 0.0)))
    opts = ltrace.default_opts(integrator=integrator or getattr(metric, "integrator", "rk4"),
                               precision=precision or getattr(metric, "precision", 32), schedule="direct",
                               tb_symmetry=0, axis_refine_frac=Y_AXIS_REFINE_FRAC)
    if source_image is not None:
        source_image = np.asarray(source_image)
        if source_image.ndim == 3 and source_image.shape[2] == 4:
            source_image = source_image[..., :3]
        shape = source_image.shape[:2]
        if S is not None and (shape[0] % S or shape[1] % S):
            raise ValueError(f"samples={S}: the background must be the fine frame, (H * samples, W * samples); got {shape}")
    elif S is not None:
        shape = (int(shape[0]) * S, int(shape[1]) * S)
    cam = _camera(shape, fov, psi, r_obs, theta_obs)      # (with samples: the fine camera)
    if source_image is not None:
        base = ltrace.render(cam, met, opts, background=source_image, want=("rgb",))["rgb"]
    d, spot = disk.to_lt(), hotspot.to_lt() if diskmap is None else None
    m = int(getattr(disk, "max_images", 3))
    field = bfield.to_lt() if bfield is not None else None
    if field is not None or atmosphere is not None:
        normal = field if field is not None else ltrace.default_bfield(b_r=0.0, b_phi=0.0, b_z=1.0)
        traced = ltrace.trace_disk_pol(cam, met, opts, d, normal, max_images=m, want=("hits", "n_hits", "pol"))
    else:
        traced = ltrace.trace_disk_hits(cam, met, opts, d, max_images=m, want=("hits", "n_hits"))
    if diskmap is not None:
        out = _sequence_diskmap(traced, met, d, diskmap, times, dt, base, S, spectrum, baselines)
        _sequence_thermal(out, traced, met, d, thermal, frequencies, bands, S)
        _sequence_transfer(out, traced, met, d, disk, lamppost, transfer, spectrum, r_obs, theta_obs, S)
        return out
    frames, rgba = [], []
    for t in times:
        if S is None:
            f = ltrace.shade_hotspot(traced["hits"], traced["n_hits"], met, d, spot, float(t), base=base)
        else:
            f = ltrace.shade_hotspot_aa(traced["hits"], traced["n_hits"], S, met, d, spot, float(t), base=base)
        frames.append(f["rgb"])
        rgba.append(f["rgba"])
    lc = ltrace.hotspot_lightcurve(traced["hits"], traced["n_hits"], met, d, spot, float(times[0]), dt, times.size)
    if S is not None:
        lc = lc / np.array([S * S, S ** 3, S ** 3], dtype=np.float64)
    out = dict(frames=np.stack(frames), rgba=np.stack(rgba), lightcurve=lc, hits=traced["hits"], n_hits=traced["n_hits"],
               stats=traced["stats"])
    if field is not None:
        rec = (traced["hits"], traced["n_hits"], traced["pol"], met, d, spot, field)
        slc = ltrace.hotspot_lightcurve_stokes(*rec, float(times[0]), dt, times.size)
        if S is None:
            stokes = [ltrace.shade_stokes(*rec, float(t)) for t in times]
        else:
            stokes = [ltrace.shade_stokes_aa(*rec[:3], S, *rec[3:], float(t)) for t in times]
            slc = slc / np.float64(S * S)
        out.update(pol=traced["pol"], stokes=np.stack(stokes), stokes_lightcurve=slc)
    if spectrum is not None:
        sp = spectrum.to_lt()
        dyn = ltrace.hotspot_spectrum(traced["hits"], traced["n_hits"], met, d, spot, sp, float(times[0]), dt, times.size)
        _sequence_spectra(out, traced, met, d, sp, dyn, S)
    if baselines is not None:
        uv = baselines.fine(1 if S is None else S)
        dyn = ltrace.hotspot_visibility(traced["hits"], traced["n_hits"], met, d, spot, uv, baselines.split_orders, float(times[0]), dt,
                                        times.size)
        _sequence_visibilities(out, traced, met, d, baselines, uv, dyn, S)
        if field is not None:
            rec = (traced["hits"], traced["n_hits"], traced["pol"], met, d)
            still = ltrace.disk_visibility_stokes(*rec, field, uv, baselines.split_orders)
            dyn = ltrace.hotspot_visibility_stokes(*rec, spot, field, uv, baselines.split_orders, float(times[0]), dt, times.size)
            k = 1 if S is None else S
            shape = (traced["hits"].shape[0] // k, traced["hits"].shape[1] // k)
            out.update(visibility_stokes=baselines.recentre(dyn, shape, k), disk_visibility_stokes=baselines.recentre(still, shape, k))
    _sequence_thermal(out, traced, met, d, thermal, frequencies, bands, S, atmosphere)
    _sequence_transfer(out, traced, met, d, disk, lamppost, transfer, spectrum, r_obs, theta_obs, S)
    if S is not None:
        out["samples"] = S
    return out


def _sequence_visibilities(out, traced, met, d, baselines, uv, dyn, S):
    """render_sequence's `visibility` (the moving emitter's, dyn) and `disk_visibility`: per output pixel, about the centre."""
    still = ltrace.disk_visibility(traced["hits"], traced["n_hits"], met, d, uv, baselines.split_orders)
    k = 1 if S is None else S
    shape = (traced["hits"].shape[0] // k, traced["hits"].shape[1] // k)
    out.update(visibility=baselines.recentre(dyn, shape, k), disk_visibility=baselines.recentre(still, shape, k))


def _sequence_spectra(out, traced, met, d, sp, dyn, S):
    """render_sequence's `spectrum` (the moving emitter's, dyn) and `disk_spectrum`, in output-pixel units."""
    line = ltrace.disk_spectrum(traced["hits"], traced["n_hits"], met, d, sp)
    scale = np.float64(1 if S is None else S * S)
    out.update(spectrum=dyn / scale, disk_spectrum=line / scale)


def _sequence_thermal(out, traced, met, d, thermal, frequencies, bands, S, atmosphere=None):
    """render_sequence's `thermal_spectrum` (in output-pixel units, as `disk_spectrum`) and `thermal_bands`, and with an
    atmosphere their Stokes forms, scaled and resolved the same way."""
    if thermal is None:
        return
    th = thermal.to_lt()
    if frequencies is not None:
        nu = np.asarray(frequencies, dtype=np.float64).ravel()
        sp = ltrace.thermal_spectrum(traced["hits"], traced["n_hits"], met, d, th, thermal.flux, nu)
        out.update(thermal_spectrum=sp / np.float64(1 if S is None else S * S), thermal_frequencies=nu)
    if bands is not None:
        th.split_orders = 0                                   # (the planes of a band image are its bands)
        img = ltrace.shade_thermal(traced["hits"], traced["n_hits"], met, d, th, thermal.flux, bands)
        if S is not None and img.shape[0]:
            import aa
            img = np.stack([aa.resolve(plane, S) for plane in img])
        out["thermal_bands"] = img
    if atmosphere is None:
        return
    out["pol"] = traced["pol"]
    rec = (traced["hits"], traced["n_hits"], traced["pol"], met, d)
    if frequencies is not None:
        th.split_orders = int(thermal.split_orders)
        sp = ltrace.thermal_spectrum_stokes(*rec, th, thermal.flux, atmosphere.limb, atmosphere.poldeg, nu)
        out["thermal_spectrum_stokes"] = sp / np.float64(1 if S is None else S * S)
    if bands is not None:
        th.split_orders = 0
        img = ltrace.shade_thermal_stokes(*rec, th, thermal.flux, atmosphere.limb, atmosphere.poldeg, bands)
        if S is not None and img.shape[0]:
            import aa
            img = np.stack([np.stack([aa.resolve(plane, S) for plane in band]) for band in img])
        out["thermal_bands_stokes"] = img


def _sequence_transfer(out, traced, met, d, disk, lamppost, transfer, spectrum, r_obs, theta_obs, S):
    """render_sequence's `transfer` (in output-pixel units, as `disk_spectrum`), `transfer_tau_edges` and `transfer_tables`."""
    if lamppost is None:
        return
    if (lamppost.M, lamppost.a) != (float(met.M), float(met.a)):
        raise ValueError("render_sequence: the lamp post's hole (M, a) is not the metric's")
    r_min, r_max = disk.inner_edge(met.M, met.a), float(disk.r_out)
    delay, emis = lamppost.tables(r_min, r_max)
    lt = transfer.to_lt(r_min, r_max, delay.size, lamppost.t_ref(r_obs, theta_obs))
    tf = ltrace.disk_transfer(traced["hits"], traced["n_hits"], met, d, spectrum.to_lt(), lt, delay, emis)
    nodes = r_min + np.arange(delay.size) * (r_max - r_min) / (delay.size - 1)
    out.update(transfer=tf / np.float64(1 if S is None else S * S), transfer_tau_edges=transfer.edges(),
               transfer_tables=np.stack([nodes, delay, emis]), transfer_t_ref=float(lt.t_ref))


def _table_emitter(diskmap):
    """(the emitter's arguments, the entry points frame / supersampled frame / light curve / spectrum / visibility) of a
    disk.DiskMap, or of a disk.DiskMovie: the map's with the movie's clock behind the map's struct."""
    from disk import DiskMovie
    if isinstance(diskmap, DiskMovie):
        dm, mv = diskmap.to_lt()
        return (dm, mv, diskmap.texels), (ltrace.shade_diskmovie, ltrace.shade_diskmovie_aa, ltrace.diskmovie_lightcurve,
                                          ltrace.diskmovie_spectrum, ltrace.diskmovie_visibility)
    return (diskmap.to_lt(), diskmap.texels), (ltrace.shade_diskmap, ltrace.shade_diskmap_aa, ltrace.diskmap_lightcurve,
                                               ltrace.diskmap_spectrum, ltrace.diskmap_visibility)


def _sequence_diskmap(traced, met, d, diskmap, times, dt, base, S, spectrum=None, baselines=None):
    """render_sequence's frames and light curve for a disk map or a disk movie, from the traced records."""
    table, (shade, shade_aa, lightcurve, dyn_spectrum, dyn_visibility) = _table_emitter(diskmap)
    frames, rgba = [], []
    for t in times:
        if S is None:
            f = shade(traced["hits"], traced["n_hits"], met, d, *table, float(t), base=base)
        else:
            f = shade_aa(traced["hits"], traced["n_hits"], S, met, d, *table, float(t), base=base)
        frames.append(f["rgb"])
        rgba.append(f["rgba"])
    lc = lightcurve(traced["hits"], traced["n_hits"], met, d, *table, float(times[0]), dt, times.size)
    if S is not None:
        lc = lc / np.array([S * S, S ** 3, S ** 3], dtype=np.float64)
    out = dict(frames=np.stack(frames), rgba=np.stack(rgba), lightcurve=lc, hits=traced["hits"], n_hits=traced["n_hits"],
               stats=traced["stats"])
    if spectrum is not None:
        sp = spectrum.to_lt()
        dyn = dyn_spectrum(traced["hits"], traced["n_hits"], met, d, *table, sp, float(times[0]), dt, times.size)
        _sequence_spectra(out, traced, met, d, sp, dyn, S)
    if baselines is not None:
        uv = baselines.fine(1 if S is None else S)
        dyn = dyn_visibility(traced["hits"], traced["n_hits"], met, d, *table, uv, baselines.split_orders, float(times[0]), dt, times.size)
        _sequence_visibilities(out, traced, met, d, baselines, uv, dyn, S)
    if S is not None:
        out["samples"] = S
    return out


def spectrum_from_args(args):
    """The disk.Spectrum of --spectrum G_MIN G_MAX N_BINS [--spectrum-orders], or None; refused without a sequence."""
    from disk import Spectrum
    if args.spectrum is None:
        if args.spectrum_orders:
            raise ValueError("--spectrum-orders needs --spectrum G_MIN G_MAX N_BINS")
        return None
    if args.hotspot is None and args.bfield is None and args.disk_map is None:
        raise ValueError("--spectrum bins the stored hits of a sequence; use it with --hotspot or --disk-map (and --disk-images N)")
    if args.spectrum[2] != int(args.spectrum[2]):
        raise ValueError("--spectrum: N_BINS must be a whole number")
    return Spectrum(args.spectrum[0], args.spectrum[1], int(args.spectrum[2]), split_orders=args.spectrum_orders)


def thermal_from_args(args, disk=None, M=1.0, a=0.0):
    """(disk.ThermalDisk, frequencies or None, bands or None) of --thermal T_MAX [F_COL] with --thermal-frequencies NU_MIN
    NU_MAX N (log-spaced) and / or --thermal-bands NU ..., or None: the Novikov-Thorne disk of (M, a) from the ISCO to the
    disk's outer edge.  Refused without a sequence and without the optically thin disk, as --spectrum is."""
    from disk import ThermalDisk, THERMAL_MAX_BANDS, THERMAL_MAX_FREQS
    if args.thermal is None:
        if args.thermal_frequencies is not None or args.thermal_bands is not None:
            raise ValueError("--thermal-frequencies / --thermal-bands need --thermal T_MAX [F_COL]")
        return None
    if args.hotspot is None and args.bfield is None and args.disk_map is None:
        raise ValueError("--thermal shades the stored hits of a sequence; use it with --hotspot or --disk-map (and --disk-images N)")
    if len(args.thermal) > 2:
        raise ValueError("--thermal takes T_MAX [F_COL]")
    if args.thermal_frequencies is None and args.thermal_bands is None:
        raise ValueError("--thermal needs --thermal-frequencies NU_MIN NU_MAX N and / or --thermal-bands NU ...")
    nu = None
    if args.thermal_frequencies is not None:
        lo, hi, n = args.thermal_frequencies
        if n != int(n) or not 1 <= n <= THERMAL_MAX_FREQS:
            raise ValueError(f"--thermal-frequencies: N must be a whole number, 1 ... {THERMAL_MAX_FREQS}")
        if not (0.0 < lo <= hi and np.isfinite(hi)):
            raise ValueError("--thermal-frequencies: 0 < NU_MIN <= NU_MAX, both finite")
        nu = np.exp(np.linspace(np.log(lo), np.log(hi), int(n)))
        nu[0], nu[-1] = (lo, hi) if n > 1 else (lo, lo)
    bands = None
    if args.thermal_bands is not None:
        bands = np.asarray(args.thermal_bands, dtype=np.float64)
        if bands.size > THERMAL_MAX_BANDS or not np.all((bands > 0.0) & np.isfinite(bands)):
            raise ValueError(f"--thermal-bands: 1 ... {THERMAL_MAX_BANDS} frequencies, each finite and > 0")
    if disk is None:
        return None, nu, bands                                # (checked only: the table needs the disk's outer edge)
    if not hasattr(disk, "max_images"):
        raise ValueError("--thermal needs --disk-images N")
    t_max, f_col = float(args.thermal[0]), float(args.thermal[1]) if len(args.thermal) == 2 else 1.0
    return ThermalDisk.novikov_thorne(M, a, disk.r_out, t_max=t_max, f_col=f_col), nu, bands


def atmosphere_from_args(args):
    """disk.Atmosphere of --thermal-atmosphere chandrasekhar|isotropic, or None.  Refused without --thermal, with a map (which
    is not polarized) and with a --bfield that does not point along the disk's normal."""
    from disk import Atmosphere
    if args.thermal_atmosphere is None:
        return None
    if args.thermal is None:
        raise ValueError("--thermal-atmosphere needs --thermal T_MAX [F_COL]")
    if args.disk_map is not None:
        raise ValueError("--thermal-atmosphere: a map is not polarized; use it with --hotspot or --bfield 0 0 1")
    if args.bfield is not None and not (args.bfield[0] == 0.0 and args.bfield[1] == 0.0 and args.bfield[2] != 0.0):
        raise ValueError("--thermal-atmosphere: the atmosphere's polarization is that of --bfield 0 0 1; use that field or none")
    return Atmosphere.chandrasekhar() if args.thermal_atmosphere == "chandrasekhar" else Atmosphere.isotropic()


def transfer_from_args(args, disk=None, M=1.0, a=0.0):
    """(disk.Lamppost, disk.TransferGrid) of --lamppost H --transfer TAU_MIN TAU_MAX N, or None: the g axis is --spectrum's.
    Refused without a sequence, without --spectrum and without the optically thin disk."""
    from disk import Lamppost, TransferGrid
    if args.lamppost is None and args.transfer is None:
        return None
    if args.lamppost is None or args.transfer is None:
        raise ValueError("--lamppost H and --transfer TAU_MIN TAU_MAX N go together")
    if args.hotspot is None and args.bfield is None and args.disk_map is None:
        raise ValueError("--transfer bins the stored hits of a sequence; use it with --hotspot or --disk-map (and --disk-images N)")
    if args.spectrum is None:
        raise ValueError("--transfer needs --spectrum G_MIN G_MAX N_BINS for its g axis")
    if args.transfer[2] != int(args.transfer[2]):
        raise ValueError("--transfer: N must be a whole number")
    grid = TransferGrid(args.transfer[0], args.transfer[1], int(args.transfer[2]))
    if disk is None:
        return None, grid                                      # (checked only: the source needs the hole)
    if not hasattr(disk, "max_images"):
        raise ValueError("--transfer needs --disk-images N")
    return Lamppost(M, a, args.lamppost * M), grid


def baselines_from_args(args):
    """The disk.Baselines of --visibility N U_MAX ANGLE_DEG [--visibility-orders], or None; refused without a sequence."""
    from disk import Baselines
    if args.visibility is None:
        if args.visibility_orders:
            raise ValueError("--visibility-orders needs --visibility N U_MAX ANGLE_DEG")
        return None
    if args.hotspot is None and args.bfield is None and args.disk_map is None:
        raise ValueError("--visibility transforms the stored hits of a sequence; use it with --hotspot or --disk-map (and --disk-images N)")
    if args.visibility[0] != int(args.visibility[0]):
        raise ValueError("--visibility: N must be a whole number")
    return Baselines.radial(int(args.visibility[0]), args.visibility[1], args.visibility[2], split_orders=args.visibility_orders)


def diskmap_from_args(args, disk, M, a):
    """The disk.DiskMap of --disk-map PATH.npy|spiral and its --disk-map-* options; the range defaults to the disk's edges.
    A 3-D array, or --disk-map flare, is a disk.DiskMovie on the clock of --disk-map-frames T0 DT [hold|loop]."""
    from disk import DiskMap, DiskMovie, flare_movie, spiral_map
    r_min, r_max = args.disk_map_range if args.disk_map_range is not None else (disk.inner_edge(M, a), disk.r_out)
    common = dict(r_min=float(r_min), r_max=float(r_max), rotation=args.disk_map_rotation, omega_p=args.disk_map_omega,
                  exposure=args.disk_map_exposure)
    clock = movie_clock_from_args(args)
    if args.disk_map == "spiral":
        texels = spiral_map(256, 1024, r_min=r_min, r_max=r_max)
    elif args.disk_map == "flare":
        if clock is None:
            raise ValueError("--disk-map flare is a movie and needs its clock: --disk-map-frames T0 DT [hold|loop]")
        t0, dt, boundary = clock
        # 32 frames: a clump at 0.4 of the way out that outshines the quiescent disk threefold at frame 12 and lasts some five frames
        return flare_movie(32, 256, 1024, r_s=r_min + 0.4 * (r_max - r_min), phi_s=0.0, sigma=0.08 * (r_max - r_min), t_peak=t0 + 12 * dt,
                           t_width=2 * dt, dt_frame=dt, t0=t0, floor=0.05, amplitude=10.0, boundary=boundary, M=M, a=a, **common)
    else:
        texels = np.load(args.disk_map, allow_pickle=False)
    if texels.ndim == 3:
        if clock is None:
            raise ValueError(f"--disk-map: {texels.shape} is a movie of {texels.shape[0]} frames and needs its clock: "
                             "--disk-map-frames T0 DT [hold|loop]")
        return DiskMovie(texels, t0=clock[0], dt_frame=clock[1], boundary=clock[2], **common)
    if clock is not None:
        raise ValueError("--disk-map-frames is the clock of a movie: a 3-D array (n_frames, n_r, n_phi), or --disk-map flare")
    return DiskMap(texels, **common)


def movie_clock_from_args(args):
    """(t0, dt_frame, boundary) of --disk-map-frames T0 DT [hold|loop], or None."""
    f = args.disk_map_frames
    if f is None:
        return None
    if len(f) not in (2, 3) or (len(f) == 3 and f[2] not in ("hold", "loop")):
        raise ValueError("--disk-map-frames takes T0 DT [hold|loop]")
    try:
        t0, dt = float(f[0]), float(f[1])
    except ValueError:
        raise ValueError("--disk-map-frames takes T0 DT [hold|loop]: T0 and DT are numbers") from None
    if not (np.isfinite(t0) and np.isfinite(dt) and dt > 0.0):
        raise ValueError("--disk-map-frames: T0 and DT must be finite, DT > 0")
    return t0, dt, f[2] if len(f) == 3 else "hold"


def main_sequence(args, disk):
    """--hotspot R PHI0 SIGMA --times T0 DT N: numbered PNGs next to --output and the light curve as .npy.
    --disk-map PATH.npy|spiral (with --disk-map-range / -rotation / -omega / -exposure): the same for an emissivity table
    that turns with the disk, in the spot's place.  A 3-D array (n_frames, n_r, n_phi) or --disk-map flare, with
    --disk-map-frames T0 DT [hold|loop]: the same for a movie, tables that change with time.
    --samples S: the sequence supersampled, S x S rays per pixel traced once and every frame resolved on the GPU.
    --bfield BR BPHI BZ [--pol-frac P]: also the Stokes frames (I, Q, U) as numbered .npy and the Stokes light curve;
    without --hotspot the spot is dark and the frames show the disk alone.
    --spectrum G_MIN G_MAX N_BINS [--spectrum-orders]: also the moving emitter's dynamic spectrum, the disk's line profile
    and the grid's edges as .npy.
    --visibility N U_MAX ANGLE_DEG [--visibility-orders]: also the complex visibilities of the moving emitter and of the disk
    on N baselines of 0 ... U_MAX cycles per pixel along ANGLE_DEG, and the baselines, as .npy; together with --bfield also
    the polarized visibilities (I, Q, U per baseline) of the spot and of the disk.
    --thermal T_MAX [F_COL] with --thermal-frequencies NU_MIN NU_MAX N and / or --thermal-bands NU ...: also the disk's thermal
    continuum of a Novikov-Thorne flux profile -- its spectrum at N log-spaced frequencies with the frequencies, and the
    unclamped band images -- as .npy.  --thermal-atmosphere chandrasekhar|isotropic: also the continuum of a scattering
    atmosphere -- the Stokes spectrum, the polarization degree and angle per frequency and the Stokes band images -- as .npy.
    --lamppost H --transfer TAU_MIN TAU_MAX N (with --spectrum for the g axis): also the disk's delay-energy response to a
    flash of a source on the axis at r = H M, the delay grid's edges and the two radial tables, as .npy."""
    from disk import BField, HotSpot
    spec = spectrum_from_args(args)
    base_lines = baselines_from_args(args)
    thermal_from_args(args)                                   # (its refusals that need no disk come before the others')
    atmos = atmosphere_from_args(args)
    transfer_from_args(args)
    if args.disk_map is not None and args.hotspot is not None:
        raise ValueError("--disk-map: a map together with --hotspot is out of scope; use one of them")
    if args.disk_map is not None and args.bfield is not None:
        raise ValueError("--disk-map: a map is not polarized; use it without --bfield")
    if not args.synthetic:
        raise ValueError("--hotspot / --bfield / --disk-map render over a black sky at the size given by --synthetic W H")
    if disk is None or not hasattr(disk, "max_images"):
        raise ValueError("--hotspot / --bfield / --disk-map need --disk-images N")
    width, height = int(args.synthetic[0]), int(args.synthetic[1])
    metric = Kerr(M=args.M, a=args.a, integrator=args.integrator, precision=args.precision)
    vfov = np.radians(args.fov_v)
    fov = (2 * np.arctan(np.tan(vfov / 2) * width / height), vfov)
    t0, dt, n = float(args.times[0]), float(args.times[1]), int(args.times[2])
    if args.adaptive is not None:
        raise ValueError("--adaptive: sequences (--hotspot / --bfield / --disk-map) are not adaptively sampled; use --samples S alone")
    dmap = None
    if args.disk_map is not None:
        spot, dmap = None, diskmap_from_args(args, disk, args.M, args.a)
    elif args.hotspot is not None:
        spot = HotSpot(r_spot=args.hotspot[0], phi0=args.hotspot[1], sigma=args.hotspot[2], exposure=args.hotspot_exposure)
    else:
        spot, n = HotSpot(exposure=0.0), 1
    field = BField(*args.bfield, pol_frac=args.pol_frac) if args.bfield is not None else None
    thermal, nu, bands = thermal_from_args(args, disk, args.M, args.a) or (None, None, None)
    lamp, tgrid = transfer_from_args(args, disk, args.M, args.a) or (None, None)
    out = render_sequence(None, metric, args.r_obs * metric.M, fov, disk, spot, t0 + dt * np.arange(n), shape=(height, width),
                          psi=(np.radians(args.psi_y), np.radians(args.psi_x)), theta_obs=np.radians(args.theta_obs), bfield=field,
                          samples=args.samples, diskmap=dmap, spectrum=spec, baselines=base_lines, thermal=thermal, frequencies=nu,
                          bands=bands, lamppost=lamp, transfer=tgrid, atmosphere=atmos)
    stem = args.output[:-4] if args.output.lower().endswith(".png") else args.output
    for i in range(n):
        write_png_rgba8(f"{stem}_{i:04d}.png", out["rgba"][i])
    np.save(stem + "_lightcurve.npy", out["lightcurve"])
    if field is not None:
        for i in range(n):
            np.save(f"{stem}_stokes_{i:04d}.npy", out["stokes"][i])
        np.save(stem + "_stokes_lightcurve.npy", out["stokes_lightcurve"])
        print(f"Polarization: Stokes frames -> {stem}_stokes_0000.npy ..., Stokes light curve -> {stem}_stokes_lightcurve.npy")
    if spec is not None:
        np.save(stem + "_spectrum.npy", out["spectrum"])
        np.save(stem + "_line.npy", out["disk_spectrum"])
        np.save(stem + "_spectrum_edges.npy", spec.edges())
        print(f"Spectrum: {spec.n_bins} bins of g in [{spec.g_min:g}, {spec.g_max:g}) -> {stem}_spectrum.npy (dynamic), {stem}_line.npy (the disk's "
              f"line), {stem}_spectrum_edges.npy")
    if base_lines is not None:
        np.save(stem + "_visibility.npy", out["visibility"])
        np.save(stem + "_disk_visibility.npy", out["disk_visibility"])
        np.save(stem + "_baselines.npy", base_lines.uv)
        if field is not None:
            np.save(stem + "_visibility_stokes.npy", out["visibility_stokes"])
            np.save(stem + "_disk_visibility_stokes.npy", out["disk_visibility_stokes"])
        print(f"Visibilities: {len(base_lines)} baselines up to {args.visibility[1]:g} cycles per pixel at {args.visibility[2]:g} deg -> "
              f"{stem}_visibility.npy (per time), {stem}_disk_visibility.npy (the disk's), {stem}_baselines.npy")
        if field is not None:
            print(f"Polarized visibilities (I, Q, U) -> {stem}_visibility_stokes.npy (per time), {stem}_disk_visibility_stokes.npy (the disk's)")
    if thermal is not None:
        if nu is not None:
            np.save(stem + "_thermal_spectrum.npy", out["thermal_spectrum"])
            np.save(stem + "_thermal_frequencies.npy", out["thermal_frequencies"])
        if bands is not None:
            np.save(stem + "_thermal_bands.npy", out["thermal_bands"])
        print(f"Thermal continuum: Novikov-Thorne disk, t_max {thermal.t_max:g}, f_col {thermal.f_col:g} -> "
              + ", ".join(([f"{stem}_thermal_spectrum.npy, {stem}_thermal_frequencies.npy"] if nu is not None else [])
                          + ([f"{stem}_thermal_bands.npy"] if bands is not None else [])))
        if atmos is not None:
            from disk import polarization_degree_angle
            if nu is not None:
                np.save(stem + "_thermal_spectrum_stokes.npy", out["thermal_spectrum_stokes"])
                np.save(stem + "_thermal_polarization.npy", np.stack(polarization_degree_angle(out["thermal_spectrum_stokes"]), axis=-2))
            if bands is not None:
                np.save(stem + "_thermal_bands_stokes.npy", out["thermal_bands_stokes"])
            print(f"Scattering atmosphere ({args.thermal_atmosphere}), Stokes I, Q, U -> "
                  + ", ".join(([f"{stem}_thermal_spectrum_stokes.npy, {stem}_thermal_polarization.npy (degree, angle per frequency)"]
                               if nu is not None else []) + ([f"{stem}_thermal_bands_stokes.npy"] if bands is not None else [])))
    if lamp is not None:
        np.save(stem + "_transfer.npy", out["transfer"])
        np.save(stem + "_transfer_tau_edges.npy", out["transfer_tau_edges"])
        np.save(stem + "_transfer_tables.npy", out["transfer_tables"])
        print(f"Reverberation: lamp post at h = {lamp.h:g}, {tgrid.n_tau} delay bins in [{tgrid.tau_min:g}, {tgrid.tau_max:g}) x {spec.n_bins} bins "
              f"of g, t_ref {out['transfer_t_ref']:.4f} -> {stem}_transfer.npy, {stem}_transfer_tau_edges.npy, {stem}_transfer_tables.npy")
    if args.samples is not None:
        print(f"Supersampling: {args.samples} x {args.samples} rays per pixel, every frame resolved on the GPU")
    print(f"{'Hot spot' if dmap is None else 'Disk map' if dmap.texels.ndim == 2 else 'Disk movie'}: one trace ({out['stats']['integrate_ms']:.2f} ms), {n} frames -> {stem}_0000.png ..., light curve -> "
          f"{stem}_lightcurve.npy")
    return out


# ---------------------------------------------------------------------------------------------
# benchmark print, CLI
# ---------------------------------------------------------------------------------------------
def print_benchmark_summary(image_dimension, alpha_crit, total_rays, traced_rays, timings):
    height, width = image_dimension
    pixels = width * height
    render_t = max(timings.get("render", 0.0), 1e-12)
    total_t = max(timings.get("total", 0.0), 1e-12)
    print("\nBenchmark summary")
    print(f"  resolution: {width}x{height} ({pixels:,} pixels)")
    print(f"  alpha_crit: {alpha_crit:.6f} rad")
    print(f"  total rays: {total_rays:,}")
    print(f"  traced rays: {traced_rays:,}")
    for key in ("load_image", "build_lookup", "precompute", "render", "save_image", "total"):
        print(f"  {key:<26}{timings.get(key, 0.0):>10.3f} s")
    print(f"  {'render_throughput':<26}{(pixels / render_t) / 1e6:>10.2f} MPix/s")
    print(f"  {'overall_throughput':<26}{(pixels / total_t) / 1e6:>10.2f} MPix/s")
    if "gpu_integrate_ms" in timings:
        print(f"  {'gpu integrate kernel':<26}{timings['gpu_integrate_ms']:>10.3f} ms "
              f"({traced_rays / timings['gpu_integrate_ms'] / 1e3:.1f} Mrays/s)")


def synthetic_background(height, width, seed=0):
    """Seeded RGB texture in [0, 1] (uint8 / 255 like an imread of a JPEG): the reference ships no image."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(height, width, 3), dtype=np.uint8).astype(np.float32) / 255.0


def write_png_rgba8(path, rgba, level=1):
    """Write an (H, W, 4) uint8 array as a PNG (8-bit RGBA, filter 0, one IDAT) with zlib alone.
    mpimg.imsave (image_lens.py:510 of the reference) spends its time converting float RGB to RGBA8 and
    deflating at level 6; here the GPU epilogue already produced the RGBA8 bytes (same truncation,
    bit-exact) and level 1 is enough for a render that is written once.  Decodes to the same pixels."""
    import struct
    import zlib
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    if rgba.ndim != 3 or rgba.shape[2] != 4:
        raise ValueError("rgba must be (H, W, 4) uint8")
    h, w = rgba.shape[:2]
    raw = np.empty((h, 1 + 4 * w), dtype=np.uint8)
    raw[:, 0] = 0                       # filter type None on every scanline
    raw[:, 1:] = rgba.reshape(h, 4 * w)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw.tobytes(), level)))
        f.write(chunk(b"IEND", b""))


def _lookup_cache_key(metric, r_obs, shape, fov, psi, mirror):
    """Everything the lookups depend on: metric and its backend knobs, observer, camera, the mirror quirk, and the build
    of the library that traced them (a new kernel build never reuses an old cache)."""
    return json.dumps({"metric": type(metric).__name__, "M": float(metric.M), "a": float(getattr(metric, "a", 0.0)),
                       "integrator": getattr(metric, "integrator", None), "precision": int(getattr(metric, "precision", 64)),
                       "r_obs": float(r_obs), "shape": [int(shape[0]), int(shape[1])], "fov": [float(fov[0]), float(fov[1])],
                       "psi": [float(psi[0]), float(psi[1])], "mirror": bool(mirror), "build": ltrace.build_id()}, sort_keys=True)


def load_lookup_cache(path, key):
    """(final_alpha, winding) from `path` if it was written for `key`, else None.  The file is ours (np.savez of two arrays
    and a JSON string): loaded without pickle."""
    try:
        with np.load(path, allow_pickle=False) as z:
            if str(z["key"]) == key:
                return z["final_alpha"].copy(), z["winding"].copy()
    except (OSError, KeyError, ValueError):
        pass
    return None


def save_lookup_cache(path, key, final_alpha, winding):
    with open(path, "wb") as f:          # (a file object: np.savez would append ".npz" to a bare name, and the next load would miss it)
        np.savez(f, key=np.array(key), final_alpha=final_alpha, winding=winding)


def main(metric=None, M=1.0, a=0.0, r_obs_mult=100.0, psi=(0.0, 0.0), vertical_fov_deg=40.0,
         image_path="image.jpg", output_path="lensed_image.png", synthetic=None, staged=False,
         integrator=None, precision=None, schedule=None, gpus=1, full_trace=False, dedup_alpha=False,
         lookup_cache=None, theta_obs_deg=90.0, disk=None, samples=None, adaptive=None, contrast=None):
    """`lookup_cache`: path of an .npz (the reference's .gitignore names `lookup_cache.npz`, it never wrote one): the
    final_alpha / winding lookups of this metric, observer and camera are stored there and reused by the next call with
    the same settings -- a new background then costs one colouring pass (lt_shade) instead of a trace.
    `dedup_alpha`: staged path, spherically symmetric metrics: trace distinct alphas only (precompute_final_alpha_lookup).
    `theta_obs_deg`: the observer's inclination (fused path; 90 = equatorial, as the reference).  `disk`: a thin
    accretion disk (disk.ThinDisk, or disk.TransparentDisk for the optically thin one with its higher-order images) in
    the picture (fused path, one GPU, every row traced).  `samples`: S x S rays per pixel, resolved on the GPU (fused
    path, one GPU, every row traced): a synthetic background is generated at the fine size (W S x H S), one read from a
    file is repeated S times along both axes, so the picture has the size asked for / the file's size.  `adaptive`: S_lo
    (with `samples` = S_hi): S_lo x S_lo rays for every pixel and S_hi x S_hi only where the picture has an edge
    (render_frame); the background is generated, or repeated, at both fine sizes.  `contrast`: its colour threshold."""
    import matplotlib.image as mpimg

    if metric is None:
        metric = (Schwarzschild(M=M, precision=precision) if a == 0
                  else Kerr(M=M, a=a, integrator=integrator, precision=precision, schedule=schedule))
    print(f"Metric: {type(metric).__name__} (M={metric.M}, a={getattr(metric, 'a', 0)})")
    timings = {}
    t_total = perf_counter()

    t0 = perf_counter()
    S = 1 if samples is None else int(samples)
    if S < 1:
        raise ValueError("--samples must be at least 1")
    if adaptive is not None and (samples is None or not 1 <= int(adaptive) < S):
        raise ValueError("--adaptive S_LO needs --samples S_HI with 1 <= S_LO < S_HI")
    img_lo = None
    if synthetic:
        img = synthetic_background(int(synthetic[1]) * S, int(synthetic[0]) * S)
        if adaptive is not None:
            img_lo = synthetic_background(int(synthetic[1]) * int(adaptive), int(synthetic[0]) * int(adaptive))
    else:
        img = mpimg.imread(image_path)
        if img.dtype == np.uint8:
            img = img.astype(np.float32) / 255.0
        if img.ndim == 3 and img.shape[2] == 4:
            print("Background has an alpha channel: lensing its RGB planes (see render_frame)")
            img = np.ascontiguousarray(img[..., :3])
        if adaptive is not None:
            img_lo = np.repeat(np.repeat(img, int(adaptive), axis=0), int(adaptive), axis=1)
        if samples is not None:
            img = np.repeat(np.repeat(img, S, axis=0), S, axis=1)
    timings["load_image"] = perf_counter() - t0
    height, width = img.shape[0] // S, img.shape[1] // S
    print(f"Image: {width}x{height}")

    r_obs = r_obs_mult * metric.M
    alpha_crit = metric.alpha_crit(r_obs)
    print(f"r_obs = {r_obs:.1f} M, alpha_crit = {np.degrees(alpha_crit):.4f} deg")
    vfov = np.radians(vertical_fov_deg)
    fov = (2 * np.arctan(np.tan(vfov / 2) * width / height), vfov)
    bh_y, bh_x, front = _psi_to_cam_projection(psi)
    where = ("behind observer" if not front else
             "inside FOV" if abs(bh_y) <= np.tan(fov[1] / 2) and abs(bh_x) <= np.tan(fov[0] / 2) else "outside FOV")
    print(f"BH screen offset: psi_y={np.degrees(psi[0]):.4f} deg, psi_x={np.degrees(psi[1]):.4f} deg ({where})")

    theta_obs = np.radians(theta_obs_deg)
    if (disk is not None or theta_obs_deg != 90.0 or samples is not None) and (staged or lookup_cache):
        raise ValueError("--disk / --theta-obs / --samples / --adaptive need the fused path (no --staged, no --lookup-cache)")
    rgba8 = None
    mirror = (disk is None) and samples is None and (not full_trace) and gpus <= 1 and not metric.is_spherically_symmetric and abs(psi[0]) <= 1e-8
    # (the staged path mirrors whenever the reference does, the fused one unless --full-trace / several GPUs)
    mirrored = (not metric.is_spherically_symmetric and abs(psi[0]) <= 1e-8) if staged else mirror
    cache_key = _lookup_cache_key(metric, r_obs, (height, width), fov, psi, mirrored) if lookup_cache else None
    cached = load_lookup_cache(lookup_cache, cache_key) if lookup_cache else None
    if cached is not None:
        print(f"Lookup cache hit ({lookup_cache}): colouring only")
        fa, wd = cached
        t0 = perf_counter()
        lensed = render_lensed_image(img, None, fa, wd, alpha_crit, fov, False, psi=psi)
        timings["render"] = perf_counter() - t0
        total, traced = height * width, 0
    elif staged:
        print("Building per-pixel " + ("alpha" if metric.is_spherically_symmetric else "(alpha, theta)") + " lookup...")
        t0 = perf_counter()
        alpha_lookup = build_alpha_lookup((height, width), fov, psi=psi)
        timings["build_lookup"] = perf_counter() - t0
        t0 = perf_counter()
        if metric.is_spherically_symmetric:
            fa, wd, total, traced = precompute_final_alpha_lookup(alpha_lookup, alpha_crit, r_obs, metric, dedup=dedup_alpha)
        else:
            fa, wd, total, traced = precompute_final_alpha_lookup_2d(alpha_lookup, fov, alpha_crit, r_obs, metric, psi=psi)
        timings["precompute"] = perf_counter() - t0
        t0 = perf_counter()
        lensed = render_lensed_image(img, alpha_lookup, fa, wd, alpha_crit, fov, False, psi=psi)
        timings["render"] = perf_counter() - t0
        if lookup_cache:
            save_lookup_cache(lookup_cache, cache_key, fa, wd)
    else:
        # The reference traces the top half of the frame and mirrors it whenever the observer is equatorial and the
        # hole is not offset vertically (image_lens.py:218-220, :272-276 -- off by one row, quirk Q1).  Default: do
        # as the reference does, so that `python image_lens.py --a 0.9` gives the reference's picture; --full-trace
        # (and every multi-GPU render) traces every row instead.
        print(f"Fused GPU render (pixel -> ray -> colour) on {max(gpus, 1)} GPU(s); rows: "
              + ("top half traced, bottom half mirrored as in the reference" if mirror else "every row traced"))
        t0 = perf_counter()
        extra = {} if theta_obs_deg == 90.0 else dict(theta_obs=theta_obs)
        if disk is not None:
            extra["disk"] = disk
            print(f"Accretion disk: r_in = {disk.inner_edge(metric.M, getattr(metric, 'a', 0.0)):.4f} M, "
                  f"r_out = {disk.r_out} M, q = {disk.q}, exposure = {disk.exposure}, theta_obs = {theta_obs_deg} deg"
                  + (f", optically thin: up to {disk.max_images} images per ray" if hasattr(disk, "max_images") else ""))
        if samples is not None:
            extra["samples"] = S
            print(f"Supersampling: {S} x {S} rays per pixel, resolved on the GPU")
        if adaptive is not None:
            extra.update(adaptive=int(adaptive), contrast=contrast)
            print(f"Adaptive: {int(adaptive)} x {int(adaptive)} rays for every pixel, {S} x {S} where the picture has an edge")
        out = render_frame(img if adaptive is None else (img_lo, img), metric, r_obs, fov, psi=psi, tb_symmetry=mirror,
                           want=("rgb", "rgba") + (("fa", "winding") if lookup_cache else ()), gpus=gpus, **extra)
        timings["render"] = perf_counter() - t0
        if lookup_cache:
            save_lookup_cache(lookup_cache, cache_key, np.asarray(out["fa"]), np.asarray(out["winding"]))
        timings["gpu_integrate_ms"] = out["stats"]["integrate_ms"]
        if adaptive is not None:
            print(f"Refined pixels: {out['stats']['refined']:,} of {height * width:,} ({100.0 * out['stats']['refined'] / (height * width):.2f} %)")
        lensed, total, traced = out["rgb"], height * width, out["stats"]["rays"]   # mirrored rows are copies, not rays
        rgba8 = out["rgba"] if lensed.ndim == 3 else None

    t0 = perf_counter()
    if rgba8 is not None and str(output_path).lower().endswith(".png"):
        write_png_rgba8(output_path, rgba8)   # the epilogue kernel's RGBA8 == imsave's conversion of `lensed`
    else:
        mpimg.imsave(output_path, lensed)
    timings["save_image"] = perf_counter() - t0
    timings["total"] = perf_counter() - t_total
    print_benchmark_summary((height, width), alpha_crit, total, traced, timings)
    return lensed


def build_parser():
    """The command line of `python image_lens.py`."""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=float, default=1.0, help="BH mass")
    ap.add_argument("--a", type=float, default=0.0, help="BH spin (|a| <= M, 0 = Schwarzschild)")
    ap.add_argument("--r-obs", type=float, default=100.0, help="Observer distance in units of M (default: 100)")
    ap.add_argument("--psi-y", type=float, default=0.0, help="BH vertical offset in deg (+ = top, - = bottom)")
    ap.add_argument("--psi-x", type=float, default=0.0, help="BH horizontal offset in deg (+ = right, - = left)")
    ap.add_argument("--fov-v", type=float, default=40.0, help="Vertical field of view in deg")
    ap.add_argument("--lookup-cache", default=None, help="path of an .npz holding the final_alpha / winding lookups: written after a "
                                                         "trace, reused by the next call with the same metric, observer and camera")
    ap.add_argument("--dedup-alpha", action="store_true", help="--staged, a = 0: trace every distinct alpha once")
    # backend additions
    ap.add_argument("--image", default="image.jpg", help="background image (default: image.jpg)")
    ap.add_argument("--output", default="lensed_image.png")
    ap.add_argument("--synthetic", type=int, nargs=2, metavar=("W", "H"), help="use a seeded synthetic background")
    ap.add_argument("--staged", action="store_true", help="run the reference's three stages one by one")
    ap.add_argument("--integrator", choices=["rk4", "dp45", "dp45_exact"], default=None)
    ap.add_argument("--precision", type=int, choices=[32, 64], default=None)
    ap.add_argument("--schedule", choices=["direct", "queue"], default=None)
    ap.add_argument("--gpus", type=int, default=1, help="split the frame's rows over this many GPUs of the node")
    ap.add_argument("--full-trace", action="store_true",
                    help="trace every row instead of the reference's top-half trace + mirror (Kerr, equatorial observer)")
    ap.add_argument("--theta-obs", type=float, default=90.0, help="observer inclination in deg (default: 90, equatorial)")
    ap.add_argument("--disk", action="store_true", help="draw a thin Keplerian accretion disk (Kerr; every row traced)")
    ap.add_argument("--disk-rin", type=float, default=None, help="disk inner edge in M (default: the ISCO)")
    ap.add_argument("--disk-rout", type=float, default=20.0, help="disk outer edge in M (default: 20)")
    ap.add_argument("--disk-q", type=float, default=3.0, help="emissivity index q of I ~ (r_in / r)^q (default: 3)")
    ap.add_argument("--disk-exposure", type=float, default=1.0, help="disk brightness scale (default: 1)")
    ap.add_argument("--disk-images", type=int, default=None, metavar="N",
                    help="optically thin disk: add the light of the first N (1 ... 8) images of the disk along each ray, "
                         "the photon ring included (implies --disk)")
    ap.add_argument("--samples", type=int, default=None, metavar="S",
                    help="anti-aliasing: trace S x S rays per pixel (1 ... 8) and resolve them on the GPU; with --synthetic "
                         "the background is generated at the fine size, a background file is repeated S times per axis; with --hotspot / "
                         "--bfield the sequence is traced once at the fine size and every frame resolved on the GPU")
    ap.add_argument("--adaptive", type=int, default=None, metavar="S_LO",
                    help="with --samples S_HI: trace S_LO x S_LO rays (1 ... 4) for every pixel and S_HI x S_HI only for the "
                         "pixels on an edge (of the shadow, the disk, the photon ring)")
    ap.add_argument("--contrast", type=float, default=None, metavar="T",
                    help="--adaptive: refine a pixel whose colour differs from a neighbour's by more than T in a channel "
                         "(default 0.0625; negative: off)")
    ap.add_argument("--hotspot", type=float, nargs=3, default=None, metavar=("R", "PHI0", "SIGMA"),
                    help="with --disk-images: a bright spot on the circular orbit at R (azimuth PHI0 rad at t = 0, width SIGMA), "
                         "re-shaded per --times from one trace; writes numbered PNGs and the light curve as .npy")
    ap.add_argument("--times", type=float, nargs=3, default=(0.0, 10.0, 8), metavar=("T0", "DT", "N"),
                    help="--hotspot: N observer times from T0 in steps of DT (in M)")
    ap.add_argument("--hotspot-exposure", type=float, default=1.0, help="--hotspot: brightness scale of the spot (default: 1)")
    ap.add_argument("--bfield", type=float, nargs=3, default=None, metavar=("BR", "BPHI", "BZ"),
                    help="with --disk-images: the magnetic field's direction in the disk material's frame; writes the Stokes "
                         "frames (I, Q, U) as numbered .npy and the Stokes light curve, with --hotspot or without it")
    ap.add_argument("--pol-frac", type=float, default=0.7, help="--bfield: polarization fraction in [0, 1] (default: 0.7)")
    ap.add_argument("--disk-map", default=None, metavar="PATH.npy|spiral|flare",
                    help="with --disk-images: an emissivity table (n_r, n_phi) on the disk that turns with it, from a .npy file or "
                         "the built-in two-armed spiral; re-shaded per --times from one trace like --hotspot, with --samples or without.  "
                         "A 3-D array (n_frames, n_r, n_phi), or the built-in flare, is a movie and needs --disk-map-frames")
    ap.add_argument("--disk-map-frames", nargs="+", default=None, metavar="T0 DT [hold|loop]",
                    help="--disk-map with a movie: frame q is at coordinate time T0 + q DT; beyond the movie its end frames are held "
                         "(default) or it loops")
    ap.add_argument("--disk-map-range", type=float, nargs=2, default=None, metavar=("RMIN", "RMAX"),
                    help="--disk-map: the annulus the table covers, in M (default: the disk's edges)")
    ap.add_argument("--disk-map-rotation", choices=["kepler", "rigid"], default="kepler",
                    help="--disk-map: every radius turns at the disk's own rate (kepler, the pattern shears) or all at --disk-map-omega")
    ap.add_argument("--disk-map-omega", type=float, default=0.0, metavar="W", help="--disk-map-rotation rigid: the pattern speed (1 / M)")
    ap.add_argument("--disk-map-exposure", type=float, default=1.0, metavar="X", help="--disk-map: brightness scale of the map (default: 1)")
    ap.add_argument("--spectrum", type=float, nargs=3, default=None, metavar=("G_MIN", "G_MAX", "N_BINS"),
                    help="with --hotspot / --disk-map: bin the stored hits by g = E_obs / E_rest on a linear grid of N_BINS (1 ... 512) bins; "
                         "writes the dynamic spectrum, the disk's line profile and the bin edges as .npy")
    ap.add_argument("--spectrum-orders", action="store_true", help="--spectrum: one plane per image order instead of one for all")
    ap.add_argument("--visibility", type=float, nargs=3, default=None, metavar=("N", "U_MAX", "ANGLE_DEG"),
                    help="with --hotspot / --disk-map: the complex visibilities of the stored hits on N (1 ... 1024) baselines of "
                         "0 ... U_MAX (<= 0.5) cycles per pixel along ANGLE_DEG, about the frame's centre; writes them per time, the "
                         "disk's own and the baselines as .npy; with --bfield also the polarized ones (I, Q, U per baseline)")
    ap.add_argument("--visibility-orders", action="store_true", help="--visibility: one plane per image order instead of one for all")
    ap.add_argument("--thermal", type=float, nargs="+", default=None, metavar="T_MAX [F_COL]",
                    help="with --hotspot / --disk-map: the disk's thermal continuum from the stored hits, a Novikov-Thorne flux profile "
                         "from the ISCO to the disk's outer edge with peak temperature T_MAX (as a frequency, k T / h) and "
                         "colour-correction factor F_COL (default: 1)")
    ap.add_argument("--thermal-frequencies", type=float, nargs=3, default=None, metavar=("NU_MIN", "NU_MAX", "N"),
                    help="--thermal: the spectrum at N (1 ... 1024) log-spaced frequencies; writes it and the frequencies as .npy")
    ap.add_argument("--thermal-bands", type=float, nargs="+", default=None, metavar="NU",
                    help="--thermal: the unclamped image at each of up to 16 frequencies; writes them as one .npy (n_bands, H, W)")
    ap.add_argument("--thermal-atmosphere", choices=("chandrasekhar", "isotropic"), default=None,
                    help="--thermal: the disk's surface is a scattering atmosphere: also writes the Stokes spectrum (planes, 3, N), the "
                         "polarization degree and angle per frequency and the Stokes band images (n_bands, 3, H, W) as .npy")
    ap.add_argument("--lamppost", type=float, default=None, metavar="H",
                    help="with --transfer: a point source on the spin axis at r = H (in M) that flashes once, the lamp-post corona")
    ap.add_argument("--transfer", type=float, nargs=3, default=None, metavar=("TAU_MIN", "TAU_MAX", "N"),
                    help="with --lamppost, --spectrum and --hotspot / --disk-map: the disk's delay-energy transfer function from the stored "
                         "hits on N (1 ... 1024) delay bins by --spectrum's g bins (--spectrum-orders: per image order; at most 32768 "
                         "keys in all); writes it, the delay edges and the radial tables (radius, delay, emissivity) as .npy")
    return ap


if __name__ == "__main__":
    args = build_parser().parse_args()
    disk = None
    if args.disk_images is not None:
        from disk import TransparentDisk
        disk = TransparentDisk(r_in=args.disk_rin, r_out=args.disk_rout, q=args.disk_q, exposure=args.disk_exposure,
                               max_images=args.disk_images)
    elif args.disk:
        from disk import ThinDisk
        disk = ThinDisk(r_in=args.disk_rin, r_out=args.disk_rout, q=args.disk_q, exposure=args.disk_exposure)
    spectrum_from_args(args)                                  # (refuses --spectrum without a sequence)
    baselines_from_args(args)                                 # (and --visibility)
    thermal_from_args(args)                                   # (and --thermal)
    transfer_from_args(args)                                  # (and --lamppost / --transfer)
    if args.hotspot is not None or args.bfield is not None or args.disk_map is not None:
        main_sequence(args, disk)
        sys.exit(0)
    main(M=args.M, a=args.a, r_obs_mult=args.r_obs, psi=(np.radians(args.psi_y), np.radians(args.psi_x)),
         vertical_fov_deg=args.fov_v, image_path=args.image, output_path=args.output, synthetic=args.synthetic,
         staged=args.staged, integrator=args.integrator, precision=args.precision, schedule=args.schedule,
         gpus=args.gpus, full_trace=args.full_trace, dedup_alpha=args.dedup_alpha, lookup_cache=args.lookup_cache,
         theta_obs_deg=args.theta_obs, disk=disk, samples=args.samples, adaptive=args.adaptive, contrast=args.contrast)
