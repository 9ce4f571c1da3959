"""Supersampled frames: the numpy statement of the resolve rule of lt_render_aa (include/ltrace.h, "supersampled
frames"), written independently of the kernel so that the tests can check the kernel against it and callers can
resolve a fine frame they rendered themselves.

A fine frame is the frame of the same camera with width W S and height H S; fine pixel (y S + j, x S + i) is
sub-sample (j, i) of output pixel (y, x).  The resolved colour is the mean of the S^2 float32 colours, added in float64
in row-major order (j outer, i inner) from 0.0, divided by float64(S S) and rounded to float32.
"""
import numpy as np

PLAIN, DISK, DISK_IMAGES = 0, 1, 2     # ltrace.AA_*
STATUS_ESCAPED, STATUS_CAPTURED, STATUS_INVALID, STATUS_DISK = 1, -1, 0, 2


def resolve(fine_rgb, samples):
    """(H S, W S[, C]) float32 -> (H, W[, C]) float32 by the rule above: an explicit ordered float64 loop over j, i."""
    fine = np.asarray(fine_rgb)
    if fine.dtype != np.float32:
        raise ValueError("the fine frame's colour is float32")
    S = int(samples)
    if S < 1 or fine.shape[0] % S or fine.shape[1] % S:
        raise ValueError(f"a fine frame of {fine.shape[:2]} pixels is not {S} x {S} samples per pixel")
    acc = np.zeros((fine.shape[0] // S, fine.shape[1] // S) + fine.shape[2:], dtype=np.float64)
    for j in range(S):
        for i in range(S):
            acc = acc + fine[j::S, i::S].astype(np.float64)
    return (acc / np.float64(S * S)).astype(np.float32)


def to_rgba8(rgb):
    """RGBA8 of a float32 colour as the library writes it everywhere: (x * 255) in float32, truncated; alpha 255;
    gray on one channel."""
    rgb = np.asarray(rgb, dtype=np.float32)
    if rgb.ndim == 2:
        rgb = np.repeat(rgb[..., None], 3, axis=2)
    out = np.empty(rgb.shape[:2] + (4,), dtype=np.uint8)
    out[..., :3] = (rgb * np.float32(255.0)).astype(np.uint8)
    out[..., 3] = 255
    return out


def cover(fine_status, fine_n_hits, samples, mode):
    """(H, W, 4) uint8: how many of a pixel's S^2 sub-rays escaped, were captured, were invalid, and hit the disk.
    fine_status (H S, W S) int8 of the mode's own entry point; slot 3 counts status 2 in DISK mode, the rays with
    fine_n_hits > 0 in DISK_IMAGES mode (fine_n_hits (H S, W S); unused otherwise), and is 0 in PLAIN mode."""
    st = np.asarray(fine_status)
    S = int(samples)
    H, W = st.shape[0] // S, st.shape[1] // S
    out = np.zeros((H, W, 4), dtype=np.uint8)
    if mode == DISK_IMAGES:
        on_disk = np.asarray(fine_n_hits) > 0
    elif mode == DISK:
        on_disk = st == STATUS_DISK
    else:
        on_disk = np.zeros(st.shape, dtype=bool)
    for slot, what in enumerate((st == STATUS_ESCAPED, st == STATUS_CAPTURED, st == STATUS_INVALID, on_disk)):
        n = np.zeros((H, W), dtype=np.int64)
        for j in range(S):
            for i in range(S):
                n += what[j::S, i::S]
        out[..., slot] = n
    return out


# ---- adaptive supersampling (include/ltrace.h, "adaptive supersampling") -------------------------------------------
def refine_mask(cover, rgb, samples_lo, mode, contrast):
    """(H, W) bool: the pixels lt_render_aa_adaptive refines, from the base pass's cover (H, W, 4) uint8 and rgb
    (H, W[, C]) float32 (rgb may be None when contrast < 0).  A pixel p is refined when, N(p) being its 3 x 3
    neighbourhood clipped to the frame without p itself,
      mixed     cover[p] has more than one non-zero slot (PLAIN, DISK: slots 0-3; DISK_IMAGES: slots 0-2, or
                0 < cover[p][3] < samples_lo^2);
      edge      some n in N(p) has cover[n] != cover[p] (all four bytes);
      contrast  contrast >= 0 and some n in N(p) and some channel has |rgb[p] - rgb[n]| > contrast in float32."""
    cv = np.asarray(cover)
    if cv.dtype != np.uint8 or cv.ndim != 3 or cv.shape[2] != 4:
        raise ValueError("cover is (H, W, 4) uint8")
    H, W = cv.shape[:2]
    S2 = int(samples_lo) ** 2
    if mode == DISK_IMAGES:
        mask = ((cv[..., :3] != 0).sum(axis=2) > 1) | ((cv[..., 3] > 0) & (cv[..., 3] < S2))
    else:
        mask = (cv != 0).sum(axis=2) > 1
    contrast = np.float32(contrast)
    colour = None
    if contrast >= 0:
        colour = np.asarray(rgb)
        if colour.dtype != np.float32 or colour.shape[:2] != (H, W):
            raise ValueError("rgb is (H, W[, C]) float32 of the cover's frame")
        colour = colour.reshape(H, W, -1)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            # p runs over the pixels whose neighbour (y + dy, x + dx) lies inside the frame
            ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
            yn, xn = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
            hit = np.any(cv[ys, xs] != cv[yn, xn], axis=2)
            if colour is not None:
                hit |= np.any(np.abs(colour[ys, xs] - colour[yn, xn]) > contrast, axis=2)
            mask[ys, xs] |= hit
    return mask


def compose(mask, lo, hi):
    """The adaptive frame's array: hi where mask (H, W) is set, lo elsewhere (arrays of (H, W[, C]), same dtype)."""
    lo, hi, mask = np.asarray(lo), np.asarray(hi), np.asarray(mask, dtype=bool)
    if lo.shape != hi.shape or lo.dtype != hi.dtype or lo.shape[:2] != mask.shape:
        raise ValueError("lo and hi are two frames of the mask's size")
    return np.where(mask.reshape(mask.shape + (1,) * (lo.ndim - 2)), hi, lo)
