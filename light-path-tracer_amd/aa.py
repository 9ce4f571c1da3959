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
