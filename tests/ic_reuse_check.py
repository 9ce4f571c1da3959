"""Renders a fixed sequence of small frames through lt_render_dev on ONE stream -- A, A, B, A, A, with A and B two
cameras -- and prints a digest of every output of every frame, and how many frames reused the ray records of the
stream (lt_ic_reuse_counts).  tests/test_gpu_ic_reuse.py runs it in fresh processes with LT_IC_REUSE=0 and with the
default: the digests must be equal -- reusing the records changes which kernels run, never a result."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-path-tracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np   # noqa: E402
import ltrace        # noqa: E402
import hipmini       # noqa: E402


def main():
    ltrace.require_gpu()
    h = hashlib.sha256()
    fov_v = np.radians(35.0)
    cams = {}
    for name, (W, H, psi_y, psi_x) in dict(A=(203, 117, 0.01, -0.02), B=(203, 117, 0.0, 0.03)).items():
        cams[name] = ltrace.Camera(W, H, 2 * np.arctan(np.tan(fov_v / 2) * W / H), fov_v, psi_y, psi_x, 30.0, 1.2)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    for prec in (32, 64):
        for sched in ("direct", "queue"):
            s = hipmini.Stream()
            o = ltrace.default_opts(precision=prec, schedule=sched)
            o.stream = s.ptr
            for name in "AABAA":
                cam = cams[name]
                shape = (cam.height, cam.width)
                bufs = dict(d_fa=hipmini.DeviceArray(shape, np.float32), d_w=hipmini.DeviceArray(shape, np.uint16),
                            d_status=hipmini.DeviceArray(shape, np.int8), d_steps=hipmini.DeviceArray(shape, np.uint32),
                            d_rgba=hipmini.DeviceArray(shape + (4,), np.uint8))
                ltrace.render_dev(cam, met, o, **{k: v.ptr for k, v in bufs.items()})
                s.synchronize()
                for k in sorted(bufs):
                    h.update(bufs[k].get().tobytes())
            ltrace.release_stream(s.ptr)
    hits, misses = ltrace.ic_reuse_counts()
    print("digest", h.hexdigest(), hits, misses, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
